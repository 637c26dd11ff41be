// api_host.h -- host helpers the translation units of the extern "C" surface share (tl3d_api.hip, api_fuse.hip, api_mesh.hip, api_register.hip),
// and the one scratch mechanism of the calls that need device memory of their own (scratch_carve).  Host code only.
#pragma once
#include "tl3d_internal.h"

#define REQUIRE(cond, code, ...)                           \
    do {                                                   \
        if (!(cond)) return set_err((code), __VA_ARGS__);  \
    } while (0)

namespace tl3d {

inline bool is_device_ptr(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    hipError_t e = hipPointerGetAttributes(&at, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// [a, a + na) and [b, b + nb) share a byte (host and device pointers live in one address space)
inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b || !na || !nb) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// Per-call device staging of caller arrays that may live in host or in device memory.  A device pointer is used as it is; a host
// input gets a temporary and an upload on the context's stream, a host output a temporary that finish() copies back; scratch() is
// a temporary of the call's own.  The destructor waits for the stream before it frees, on every way out of the call, so nothing
// in flight loses its memory; a call that staged nothing never waits here.
class Staging {
  public:
    explicit Staging(tl3d_ctx *ctx) : ctx_(ctx) {}
    Staging(const Staging &) = delete;
    Staging &operator=(const Staging &) = delete;
    ~Staging() {
        if (n_) (void)hipStreamSynchronize(ctx_->stream);
        for (int i = 0; i < n_; ++i) (void)hipFree(tmp_[i].dev);
    }
    template <class T> int in(const T *p, size_t bytes, const T **dev) {
        *dev = p;
        if (is_device_ptr(p)) return TL3D_OK;
        void *d = nullptr;
        const int rc = take(bytes, nullptr, &d);
        if (rc) return rc;
        *dev = (const T *)d;
        if (hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, ctx_->stream) != hipSuccess) return set_err(TL3D_E_HIP, "staging upload (%zu B) failed", bytes);
        return TL3D_OK;
    }
    template <class T> int out(T *p, size_t bytes, T **dev) {
        *dev = p;
        if (is_device_ptr(p) || bytes == 0) return TL3D_OK;
        return take(bytes, p, (void **)dev);
    }
    template <class T> int scratch(size_t bytes, T **dev) { return take(bytes, nullptr, (void **)dev); }
    // rc: what the launchers returned; it wins.  Otherwise the host outputs are copied back, and the stream is waited for when
    // anything was staged (or `wait`: the call promises finished device outputs too)
    int finish(int rc, bool wait = false) {
        if (rc) return rc;
        hipError_t e = hipSuccess;
        for (int i = 0; i < n_ && e == hipSuccess; ++i)
            if (tmp_[i].host_out) e = hipMemcpyAsync(tmp_[i].host_out, tmp_[i].dev, tmp_[i].bytes, hipMemcpyDeviceToHost, ctx_->stream);
        if (e == hipSuccess && (n_ || wait)) e = hipStreamSynchronize(ctx_->stream);
        if (e != hipSuccess) return set_err(TL3D_E_HIP, "staging copy / sync failed: %s", hipGetErrorString(e));
        return TL3D_OK;
    }

  private:
    int take(size_t bytes, void *host_out, void **dev) {
        *dev = nullptr;
        if (n_ == MAX) return set_err(TL3D_E_STATE, "more than %d staged arrays in one call", MAX);
        if (hipMalloc(dev, bytes) != hipSuccess) {
            (void)hipGetLastError();
            *dev = nullptr;
            return set_err(TL3D_E_NOMEM, "staging alloc (%zu B) failed", bytes);
        }
        tmp_[n_++] = {*dev, host_out, bytes};
        return TL3D_OK;
    }
    static constexpr int MAX = 8;
    struct Tmp { void *dev, *host_out; size_t bytes; };
    tl3d_ctx *ctx_;
    Tmp tmp_[MAX];
    int n_ = 0;
};

// A counts / offsets pair of the compaction (compact.h), cut into its halves: [n[0] chunks + 1] for the vertices (or the points),
// then [n[1] chunks + 1] for the triangles; the entry behind a half's chunks takes its total.  One half when n1 < 0.
struct ChunkHalves {
    int n[2];
    unsigned *counts[2];
    unsigned long long *offs[2];
    ChunkHalves(unsigned *c, unsigned long long *o, int n0, int n1 = -1) : n{n0, n1}, counts{c, c + n0 + 1}, offs{o, o + n0 + 1} {}
    int scan(hipStream_t s, int h) const { return launch_scan(s, counts[h], offs[h], n[h], offs[h] + n[h]); }
    // behind the caller's launches: the totals of the halves and, with `info`, its first four report words; one wait for all
    int totals(hipStream_t s, unsigned long long *tot, const unsigned long long *info = nullptr, unsigned long long *h_info = nullptr) const {
        for (int h = 0; h < (n[1] < 0 ? 1 : 2); ++h)
            TL3D_HIP(hipMemcpyAsync(&tot[h], offs[h] + n[h], sizeof(tot[h]), hipMemcpyDeviceToHost, s));
        if (info) TL3D_HIP(hipMemcpyAsync(h_info, info, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        TL3D_HIP(hipStreamSynchronize(s));
        return TL3D_OK;
    }
};

// A call's device scratch: n arrays of bytes[i] bytes, carved at 256-B steps from ONE buffer of the context (tl3d_grid_state::
// scratch[stage]) that grows on demand by free + hipMalloc of the total; on failure the buffer is gone, its capacity 0, and the
// call fails with TL3D_E_NOMEM ("<what> alloc (<total> B) failed").  What an earlier call left in the buffer is garbage: a call
// fills or writes every array before it reads it.  Stage 0 is carved once at the start of a call; stage 1 is a second buffer for
// the one array a call can size only after the host has seen a count (growing stage 0 then would lose what the call has in it).
// hipFree's implicit wait keeps work in flight from losing its memory.  Defined in tl3d_api.hip.
int scratch_carve(tl3d_ctx *ctx, int stage, const size_t *bytes, int n, void **out, const char *what);

// slots of a 64-bit key table that takes max_keys entries at most (keytab.h H3): the smallest power of two >= 1024 and >= 2 * max_keys
inline size_t kt_slots(size_t max_keys) {
    size_t cap = 1024;
    while (cap < 2 * max_keys) cap <<= 1;                  // load <= 0.5
    return cap;
}

// Every key of a 64-bit key table (keytab.h) EMPTY, behind what the stream holds already.  A caller that
// keeps a 32-bit word beside each key carves it too; what it holds, and its fill if it needs one, are the caller's.
inline int kt_reserve(tl3d_ctx *ctx, unsigned long long *keys, size_t slots) {
    TL3D_HIP(hipMemsetAsync(keys, 0xFF, slots * sizeof(unsigned long long), ctx->stream));
    return TL3D_OK;
}

// grow-on-demand device scratch of `need` elements: on failure the buffer is gone and its capacity 0
template <class T> int grow(T **p, size_t *cap, size_t need, const char *what) {
    if (need <= *cap) return TL3D_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    if (hipMalloc(p, need * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(TL3D_E_NOMEM, "%s alloc (%zu B) failed", what, need * sizeof(T));
    }
    *cap = need;
    return TL3D_OK;
}
// two buffers that share one capacity (*cap counts elements of each)
template <class A, class B> int grow_pair(A **a, B **b, size_t *cap, size_t need, const char *what) {
    size_t cap_b = *cap;
    int rc = grow(a, cap, need, what);
    if (!rc) rc = grow(b, &cap_b, need, what);
    if (rc) *cap = 0;
    return rc;
}

// what api_register.hip and api_fuse.hip share with tl3d_api.hip, where each is defined and described (flush_updates: api_fuse.hip)
int check_slot(tl3d_ctx *ctx, int slot, bool need_loaded);
int order_after_lanes(tl3d_ctx *ctx, int slot, bool rewrites_depth, bool rewrites_nmap);
void *pool_take(FramePool &fp);
int flush_updates(tl3d_ctx *ctx);
int fold_free(tl3d_ctx *ctx);
PoseD make_pose_d(const double R[9], const double t[3], bool no_pose);
int make_bp_args(tl3d_ctx *ctx, double scale, uint32_t flags, int subsample, double min_d, double max_d, BpArgs *a);
int validate_grid(const tl3d_config *cfg);
void grid_geometry(Grid &g, const tl3d_config *cfg);
int measure_max_weight(tl3d_ctx *ctx, const int2 *grid, long long *out);
// every call that reads or writes the TSDF grid, re-uses a frame slot, synchronises or time-stamps first issues the deferred updates
#define FLUSH_UPDATES(ctx_)                          \
    do {                                             \
        const int rc_ = tl3d::flush_updates(ctx_);   \
        if (rc_) return rc_;                         \
    } while (0)
#define FLUSH_AND_FOLD(ctx_)                         \
    do {                                             \
        FLUSH_UPDATES(ctx_);                         \
        const int frc_ = tl3d::fold_free(ctx_);      \
        if (frc_) return frc_;                       \
    } while (0)
void registration_release(tl3d_ctx *ctx);   // tl3d_destroy's: everything registration owns in a context (defined in api_register.hip)

}  // namespace tl3d
