// tl3d_api.hip -- the extern "C" surface declared in include/tl3d.h: context, frame slots, grids, launch glue (the mesh calls: api_mesh.hip;
// normal maps, ICP and tracking: api_register.hip; fusion and brick counts: api_fuse.hip), and most of the host helpers api_host.h declares.
#include <dlfcn.h>
#include <stdarg.h>
#include <stdlib.h>
#include <math.h>

#include <mutex>
#include <new>
#include <vector>

#include "api_host.h"

using namespace tl3d;

static thread_local char g_err[512] = "";

namespace tl3d {
int set_err(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace tl3d

// Tuning knobs (TL3D_PREP_STREAMS, TL3D_TSDF_BATCH, ...) are read from the environment only by the experiments flavour of the
// library (csrc/build.sh with TL3D_FLAVOUR=experiments -> libtl3d_exp.so); the shipped library ignores them.
static int env_int(const char *name, int dflt) {
#ifdef TL3D_EXPERIMENTS
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

// The five RCCL entry points the merge needs, resolved at run time; enum values from rccl.h (ncclInt32 = 2, ncclInt64 = 4,
// ncclUint64 = 5, ncclSum = 0).
namespace {
struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, const void *, int) = nullptr;      // ncclUniqueId is passed BY VALUE in C: see rccl_init_rank
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*CommAbort)(void *) = nullptr;            // optional
    const char *(*GetErrorString)(int) = nullptr;
};
struct RcclId { char bytes[TL3D_RCCL_ID_BYTES]; };
Rccl g_rccl;

int rccl_load() {
    if (g_rccl.lib) return TL3D_OK;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
        g_rccl.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (g_rccl.lib) break;
    }
    if (!g_rccl.lib) return set_err(TL3D_E_STATE, "RCCL (librccl.so) could not be loaded: %s", dlerror());
    g_rccl.GetUniqueId = (int (*)(void *))dlsym(g_rccl.lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(void **, int, const void *, int))dlsym(g_rccl.lib, "ncclCommInitRank");
    g_rccl.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(g_rccl.lib, "ncclAllReduce");
    g_rccl.CommDestroy = (int (*)(void *))dlsym(g_rccl.lib, "ncclCommDestroy");
    g_rccl.GetErrorString = (const char *(*)(int))dlsym(g_rccl.lib, "ncclGetErrorString");
    g_rccl.CommAbort = (int (*)(void *))dlsym(g_rccl.lib, "ncclCommAbort");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy) {
        g_rccl.lib = nullptr;
        return set_err(TL3D_E_STATE, "librccl.so lacks the expected entry points");
    }
    return TL3D_OK;
}
const char *rccl_msg(int rc) { return g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error"; }
}  // namespace


// hipMalloc for the large allocations of a grid: if the device is out of memory while the frame-slab cache (pool_release) holds
// some, give that back and try once more
static hipError_t device_malloc_big(void **p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return e;
    (void)hipGetLastError();
    (void)tl3d_release_cached_memory();
    e = hipMalloc(p, bytes);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

namespace tl3d {
int scratch_carve(tl3d_ctx *ctx, int stage, const size_t *bytes, int n, void **out, const char *what) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += (bytes[i] + 255) & ~(size_t)255;
    const int rc = grow(&ctx->scratch[stage], &ctx->scratch_bytes[stage], total, what);
    if (rc) return rc;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        out[i] = ctx->scratch[stage] + off;
        off += (bytes[i] + 255) & ~(size_t)255;
    }
    return TL3D_OK;
}
}  // namespace tl3d

PoseD tl3d::make_pose_d(const double R[9], const double t[3], bool no_pose) {
    PoseD p;
    memset(&p, 0, sizeof(p));
    if (no_pose) {
        p.r[0] = p.r[4] = p.r[8] = 1.0;
        return p;
    }
    for (int i = 0; i < 9; ++i) p.r[i] = R[i];
    for (int i = 0; i < 3; ++i) p.ct[i] = (R[0 + i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2];   // (R^T t)_i, D2R:376
    return p;
}

int tl3d::check_slot(tl3d_ctx *ctx, int slot, bool need_loaded) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(slot >= 0 && slot < ctx->cfg.n_slots, TL3D_E_INVALID, "slot %d out of range [0,%d)", slot, ctx->cfg.n_slots);
    if (need_loaded) REQUIRE(ctx->slots[slot].loaded, TL3D_E_STATE, "slot %d holds no frame", slot);
    return TL3D_OK;
}

static int upload_impl(tl3d_ctx *ctx, int slot, const void *depth_hd, int depth_kind, const uint8_t *bgr_hd, bool wait);
static int bp_check_error(tl3d_ctx *ctx, unsigned long long err);

// ICP lanes read slots[src].depth and slots[tgt].nmap on their own streams.  A call that rewrites one of those buffers on
// the main stream (a new upload into the slot, a rebuilt normal map) is ordered behind every uncollected run that reads it.
int tl3d::order_after_lanes(tl3d_ctx *ctx, int slot, bool rewrites_depth, bool rewrites_nmap) {
    for (int l = 0; l < TL3D_ICP_LANES; ++l) {
        tl3d_ctx::IcpLane &ln = ctx->icp_lanes[l];
        if (!ln.stream || !ln.busy || !ln.ev_done) continue;
        if ((rewrites_depth && ln.src_slot == slot) || (rewrites_nmap && ln.tgt_slot == slot))
            TL3D_HIP(hipStreamWaitEvent(ctx->stream, ln.ev_done, 0));
    }
    if (ctx->icp_batch.busy && ctx->icp_batch.ev_done)      // (coarse: a batch may read any slot)
        TL3D_HIP(hipStreamWaitEvent(ctx->stream, ctx->icp_batch.ev_done, 0));
    return TL3D_OK;
}

// exact largest voxel weight of the TSDF channel (blocks; the deferred updates must have been issued)
int tl3d::measure_max_weight(tl3d_ctx *ctx, const int2 *grid, long long *out) {
    if (!ctx->d_maxw && hipMalloc(&ctx->d_maxw, sizeof(int)) != hipSuccess) return set_err(TL3D_E_NOMEM, "alloc failed");
    // the context's own channel: the pool slots in use + the counts of bricks without records; anything else: a dense array
    int rc = grid == ctx->tsdf ? launch_max_weight(ctx->stream, ctx->grid, ctx->tsdf, ctx->d_maxw)
                               : launch_max_weight_dense(ctx->stream, grid, ctx->nvox, ctx->d_maxw);
    if (rc) return rc;
    int h = 0;
    TL3D_HIP(hipMemcpyAsync(&h, ctx->d_maxw, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    *out = (long long)h;
    return TL3D_OK;
}

// The free-space counters are incremented by the classification kernels on the prep streams and cleared / folded on the main
// stream.  Every main-stream write to them is followed by this marker; the next prep chains wait for it (flush_updates),
// so a count can never land in front of a clear that was issued before it (a reset followed at once by integrate calls).
static int mark_free_cnt_write(tl3d_ctx *ctx) {
    if (!ctx->ev_free && hipEventCreateWithFlags(&ctx->ev_free, hipEventDisableTiming) != hipSuccess) return set_err(TL3D_E_HIP, "event create failed");
    TL3D_HIP(hipEventRecord(ctx->ev_free, ctx->stream));
    ctx->ev_free_recorded = true;
    return TL3D_OK;
}

// pending free-space counts -> records (main stream; the deferred updates must have been issued: their classification
// kernels, which increment the counters on the side streams, are ordered before the main stream by flush_updates)
int tl3d::fold_free(tl3d_ctx *ctx) {
    if (!ctx->free_cnt || !ctx->free_dirty) return TL3D_OK;
    ctx->free_dirty = false;
    const int rc = launch_fold_free(ctx->stream, ctx->grid, ctx->tsdf, ctx->free_cnt);
    if (rc) return rc;
    return mark_free_cnt_write(ctx);
}

int tl3d::validate_grid(const tl3d_config *cfg) {
    REQUIRE((cfg->channels & ~(TL3D_CH_TSDF | TL3D_CH_CENTROID)) == 0 && cfg->channels != 0, TL3D_E_INVALID, "bad channel bits 0x%x", cfg->channels);
    REQUIRE(cfg->nx > 0 && cfg->ny > 0 && cfg->nz > 0 && cfg->nx % TL3D_BRICK == 0 && cfg->ny % TL3D_BRICK == 0 &&
                cfg->nz % TL3D_BRICK == 0,
            TL3D_E_INVALID, "grid dims %dx%dx%d must be positive multiples of %d", cfg->nx, cfg->ny, cfg->nz, TL3D_BRICK);
    REQUIRE((double)cfg->nx * cfg->ny * cfg->nz <= 4294967296.0, TL3D_E_INVALID, "grid larger than 2^32 voxels");
    REQUIRE(cfg->voxel_size > 0, TL3D_E_INVALID, "voxel_size must be positive");
    if (cfg->channels & TL3D_CH_TSDF) REQUIRE(cfg->sdf_trunc > 0, TL3D_E_INVALID, "sdf_trunc must be positive");
    REQUIRE(cfg->pool_bricks_tsdf >= 0 && cfg->pool_bricks_centroid >= 0, TL3D_E_INVALID, "negative brick pool size");
    for (int a = 0; a < 3; ++a)
        REQUIRE(cfg->voxel_offset[a] >= 0 && cfg->voxel_offset[a] % TL3D_BRICK == 0 && cfg->voxel_offset[a] < (1ll << 40), TL3D_E_INVALID,
                "voxel_offset must be non-negative multiples of %d", TL3D_BRICK);
    // the TSDF kernels place a voxel centre at fma((float)(offset + i) + 0.5f, voxel, origin): exact while offset + i < 2^23
    if (cfg->channels & TL3D_CH_TSDF) {
        const int64_t dims[3] = {cfg->nx, cfg->ny, cfg->nz};
        for (int a = 0; a < 3; ++a)
            REQUIRE(cfg->voxel_offset[a] + dims[a] <= (1ll << 23), TL3D_E_INVALID,
                    "a TSDF grid must end within 2^23 voxels of the lattice origin (axis %d: offset %lld + %lld)", a,
                    (long long)cfg->voxel_offset[a], (long long)dims[a]);
    }
    if (cfg->pool_bricks_tsdf > 0 || cfg->pool_bricks_centroid > 0)
        REQUIRE(cfg->ext_tsdf == nullptr && cfg->ext_centroid == nullptr, TL3D_E_INVALID, "a sparse grid (pool_bricks_*) cannot live in caller-owned dense memory");
    return TL3D_OK;
}

// brick tables and cursors of a fresh (or reset) grid, on the main stream: a dense channel's table is the identity and its
// cursor sits at the end of the pool; a sparse channel starts empty
static int reset_brick_tables(tl3d_ctx *ctx) {
    Grid &g = ctx->grid;
    const size_t nbr = ctx->nvox >> 9;
    unsigned cur[4] = {0u, 0u, 0u, 0u};
    if (g.tsdf_cap >= nbr) {
        const int rc = launch_iota(ctx->stream, g.tsdf_tab, (unsigned)nbr);
        if (rc) return rc;
        cur[0] = (unsigned)nbr;
    } else {
        TL3D_HIP(hipMemsetAsync(g.tsdf_tab, 0xff, nbr * sizeof(unsigned), ctx->stream));
    }
    if (g.cen_cap >= nbr) {
        const int rc = launch_iota(ctx->stream, g.cen_tab, (unsigned)nbr);
        if (rc) return rc;
        cur[2] = (unsigned)nbr;
    } else {
        TL3D_HIP(hipMemsetAsync(g.cen_tab, 0xff, nbr * sizeof(unsigned), ctx->stream));
    }
    TL3D_HIP(hipMemcpyAsync(g.cursors, cur, sizeof(cur), hipMemcpyHostToDevice, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));           // `cur` is on this stack; the prep streams do not wait for the main stream
    return TL3D_OK;
}

void tl3d::grid_geometry(Grid &g, const tl3d_config *cfg) {
    g.nx = cfg->nx; g.ny = cfg->ny; g.nz = cfg->nz;
    g.nbx = cfg->nx / 8; g.nby = cfg->ny / 8; g.nbz = cfg->nz / 8;
    g.oxd = cfg->origin[0]; g.oyd = cfg->origin[1]; g.ozd = cfg->origin[2]; g.vsd = cfg->voxel_size;
    g.offx = (double)cfg->voxel_offset[0]; g.offy = (double)cfg->voxel_offset[1]; g.offz = (double)cfg->voxel_offset[2];
    // (a centroid-only grid may sit further out than 2^31; its TSDF-path offsets are never read)
    g.vox = (int)(cfg->voxel_offset[0] & 0x7fffffff); g.voy = (int)(cfg->voxel_offset[1] & 0x7fffffff); g.voz = (int)(cfg->voxel_offset[2] & 0x7fffffff);
    g.clo[0] = g.clo[1] = g.clo[2] = 0;
    g.chi[0] = g.nx; g.chi[1] = g.ny; g.chi[2] = g.nz;
    g.ox = (float)g.oxd; g.oy = (float)g.oyd; g.oz = (float)g.ozd; g.vs = (float)g.vsd;
    g.trunc = (float)cfg->sdf_trunc;
    g.inv_trunc = (cfg->channels & TL3D_CH_TSDF) ? 1.0f / g.trunc : 0.0f;
}

// Frees everything of tl3d_grid_state and leaves the context without a grid.  Nothing on the device may still use the grid: the
// caller has issued the deferred updates and waited for the streams.  Frames, normal maps, ICP state, streams and the camera-sized
// buffers are not touched.
static void release_grid(tl3d_ctx *ctx) {
    tl3d_grid_state &gs = *ctx;
    if (gs.brick_tabs) (void)hipFree(gs.brick_tabs);
    if (gs.own_tsdf && gs.tsdf) (void)hipFree(gs.tsdf);
    if (gs.own_centroid && gs.centroid) (void)hipFree(gs.centroid);
    if (gs.free_cnt) (void)hipFree(gs.free_cnt);
    if (gs.tsdf_scratch_slab) (void)hipFree(gs.tsdf_scratch_slab);
    if (gs.block_counts) (void)hipFree(gs.block_counts);
    if (gs.block_offsets) (void)hipFree(gs.block_offsets);
    if (gs.mesh_counts) (void)hipFree(gs.mesh_counts);
    if (gs.mesh_offsets) (void)hipFree(gs.mesh_offsets);
    if (gs.mesh_first) (void)hipFree(gs.mesh_first);
    if (gs.scratch[0]) (void)hipFree(gs.scratch[0]);
    if (gs.scratch[1]) (void)hipFree(gs.scratch[1]);
    if (gs.cg_slab) (void)hipFree(gs.cg_slab);
    for (int h = 0; h < TSDF_SCRATCHES; ++h)
        if (gs.ev_upd[h]) (void)hipEventDestroy(gs.ev_upd[h]);      // (build_grid creates them anew)
    memset(&gs, 0, sizeof(gs));
    ctx->tc_done_before = ctx->tsdf_batch_no;           // (the caller has waited: no batch still reads a slot's tiles)
    ctx->grid_epoch++;
    ctx->cfg.channels = 0;
    for (int i = 0; i < 3; ++i) ctx->cfg.voxel_offset[i] = 0;
}

static int build_grid(tl3d_ctx *ctx, const tl3d_config *cfg);

// allocates (or borrows) the grid channels of cfg and the TSDF side streams / scratch; ctx->stream must exist.  On failure
// whatever was allocated has been released again: the context has no grid, as before the call.
static int alloc_grid(tl3d_ctx *ctx, const tl3d_config *cfg) {
    const int rc = build_grid(ctx, cfg);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);        // clears of the buffers allocated so far may be in flight
        release_grid(ctx);
    }
    return rc;
}

static int build_grid(tl3d_ctx *ctx, const tl3d_config *cfg) {
    Grid &g = ctx->grid;
    grid_geometry(g, cfg);
    ctx->nvox = (size_t)g.nx * g.ny * g.nz;
    ctx->tsdf_w_upper = 0;
    ctx->tsdf_w_unknown = false;
    {   // brick tables: identity for a dense channel, empty for a sparse one (slots handed out on first touch)
        const size_t nbr = ctx->nvox >> 9;
        ctx->sparse = cfg->pool_bricks_tsdf > 0 || cfg->pool_bricks_centroid > 0;
        g.tsdf_cap = (unsigned)((cfg->pool_bricks_tsdf > 0 && (size_t)cfg->pool_bricks_tsdf < nbr) ? (size_t)cfg->pool_bricks_tsdf : nbr);
        g.cen_cap = (unsigned)((cfg->pool_bricks_centroid > 0 && (size_t)cfg->pool_bricks_centroid < nbr) ? (size_t)cfg->pool_bricks_centroid : nbr);
        if (hipMalloc(&ctx->brick_tabs, (2 * nbr + 64) * sizeof(unsigned)) != hipSuccess) return set_err(TL3D_E_NOMEM, "brick table alloc failed");
        g.tsdf_tab = ctx->brick_tabs;
        g.cen_tab = ctx->brick_tabs + nbr;
        g.cursors = ctx->brick_tabs + 2 * nbr;
        g.free_cnt = nullptr;
        const int trc = reset_brick_tables(ctx);
        if (trc) return trc;
    }
    if (cfg->channels & TL3D_CH_TSDF) {
        if (cfg->ext_tsdf) {
            ctx->tsdf = (int2 *)cfg->ext_tsdf;
            ctx->tsdf_w_unknown = true;                 // caller-owned memory: contents unknown
        } else {
            const size_t pool_b = (size_t)g.tsdf_cap << 12;
            if (device_malloc_big((void **)&ctx->tsdf, pool_b) != hipSuccess) return set_err(TL3D_E_NOMEM, "TSDF record pool alloc (%zu B) failed", pool_b);
            ctx->own_tsdf = true;
            if (hipMemsetAsync(ctx->tsdf, 0, pool_b, ctx->stream) != hipSuccess) return set_err(TL3D_E_HIP, "memset failed");
        }
        {   // Side streams for the prep chains of the batches (descriptors, tiles, pyramid, brick classes, cost order, sub-brick
            // classes): the chains of the next batches run beside the update kernel of batch k.  Three streams, taken in turn, and
            // TSDF_SCRATCHES = 4 batch scratches.  Beside an update kernel a chain's big kernels stretch over a whole update period each,
            // so a chain is three periods long and three are in flight; a fourth stream with six scratches was slower (74.1 k against
            // 76.5 k frames/s: the step is bound by the sum of the work), two streams too (77.3 k against 79.2 k).
            // (A higher stream priority for the chains changes nothing measurable: 55.4k against 55.3k frames/s.)
            ctx->n_prep_streams = env_int("TL3D_PREP_STREAMS", 3);
            if (ctx->n_prep_streams < 1) ctx->n_prep_streams = 1;
            if (ctx->n_prep_streams > 4) ctx->n_prep_streams = 4;
            for (int q = 0; q < ctx->n_prep_streams; ++q)
                if (!ctx->prep_stream[q] && hipStreamCreateWithFlags(&ctx->prep_stream[q], hipStreamNonBlocking) != hipSuccess)
                    return set_err(TL3D_E_HIP, "stream create failed");
        }
        {
            const size_t nbr = (size_t)g.nbx * g.nby * g.nbz;
            ctx->free_dirty = false;
            if (hipMalloc(&ctx->free_cnt, nbr * sizeof(unsigned)) != hipSuccess) return set_err(TL3D_E_NOMEM, "free-space counter alloc failed");
            g.free_cnt = ctx->free_cnt;
            if (hipMemsetAsync(ctx->free_cnt, 0, nbr * sizeof(unsigned), ctx->stream) != hipSuccess) return set_err(TL3D_E_HIP, "memset failed");
            const int mrc = mark_free_cnt_write(ctx);
            if (mrc) return mrc;
        }
        ctx->tsdf_use_u16 = env_int("TL3D_U16_GATHER", 1) != 0;
        ctx->tsdf_pairing = env_int("TL3D_TSDF_PAIR", 1) != 0;
        ctx->tsdf_batch = env_int("TL3D_TSDF_BATCH", 32);
        if (ctx->tsdf_batch < 1) ctx->tsdf_batch = 1;
        if (ctx->tsdf_batch > TL3D_TSDF_MAXBATCH) ctx->tsdf_batch = TL3D_TSDF_MAXBATCH;
        {   // Workgroups of the update kernel (61 vector registers, eight waves per SIMD: a CU holds 8 of them): at most 32 per CU,
            // four times what the chip holds.  The ones that do not fit start one by one as waves retire, each wave on the static
            // first task of its place in the launch (dearest bricks first): the dispatcher hands the dear bricks out better than
            // the tickets do.  Same box, interleaved, three runs each, frames/s by workgroups per CU (profiles/update_residency_ab.txt):
            //            8        12       16       24       32       48       64
            //   plain    100.3 k  106.1 k  108.6 k  111.5 k  112.7 k  112.6 k  112.3 k   (lowest run)
            //   warm     --       110.3 k  --       120.6 k  123.0 k  123.2 k  --        16-bit frames: 117.0 / 122.1 / 122.7 / 122.4 k
            // and a first scan (prep kernels beside every update) the same at 12 to 48: 65.7 to 68.0 k.  Late workgroups that take
            // their first task by ticket instead, so that none waits with an unstarted workgroup: 100.7 k against 107.7 k, not kept.
            // (Round 4 had kept 12 after 77.5 to 78.2 k at 12, 16 and 24 -- with three big prep kernels beside every update, which
            // the caches have since taken out of the steady state.)
            int cus = 0;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus < 1) cus = 256;
            ctx->tsdf_max_blocks = env_int("TL3D_UPDATE_BLOCKS", 32 * cus);
        }
        if (ctx->tsdf_max_blocks < 8) ctx->tsdf_max_blocks = 8;
        ctx->tsdf_single_stream = env_int("TL3D_SINGLE_STREAM", 0) != 0;
        {   // the scratch of the batches in flight (TSDF_SCRATCHES): one allocation; the frame masks start out zero (the update re-arms them)
            const size_t each = (tsdf_batch_scratch_bytes(ctx->cam, g, ctx->tsdf_batch) + 255) & ~(size_t)255;
            void *slab = nullptr;
            if (device_malloc_big(&slab, each * TSDF_SCRATCHES) != hipSuccess) return set_err(TL3D_E_NOMEM, "TSDF scratch alloc (%zu B) failed", each * TSDF_SCRATCHES);
            ctx->tsdf_scratch_slab = slab;
            size_t zoff = 0, zbytes = 0;
            tsdf_batch_scratch_zero_range(ctx->cam, g, ctx->tsdf_batch, &zoff, &zbytes);
            for (int h = 0; h < TSDF_SCRATCHES; ++h) {
                ctx->tsdf_scratch[h] = (char *)slab + each * (size_t)h;
                if (hipMemsetAsync((char *)ctx->tsdf_scratch[h] + zoff, 0, zbytes, ctx->stream) != hipSuccess) return set_err(TL3D_E_HIP, "memset failed");
                if (!ctx->ev_prep[h] && hipEventCreateWithFlags(&ctx->ev_prep[h], hipEventDisableTiming) != hipSuccess) return set_err(TL3D_E_HIP, "event create failed");
            }
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) return set_err(TL3D_E_HIP, "sync failed");     // the prep streams do not wait for this memset
        }
        for (int h = 0; h < TSDF_SCRATCHES; ++h)
            if (hipEventCreateWithFlags(&ctx->ev_upd[h], hipEventDisableTiming) != hipSuccess) return set_err(TL3D_E_HIP, "event create failed");
    }
    if (cfg->channels & TL3D_CH_CENTROID) {
        if (cfg->ext_centroid) {
            ctx->centroid = (unsigned long long *)cfg->ext_centroid;
        } else {
            const size_t pool_b = (size_t)g.cen_cap << 14;
            if (device_malloc_big((void **)&ctx->centroid, pool_b) != hipSuccess) return set_err(TL3D_E_NOMEM, "centroid record pool alloc (%zu B) failed", pool_b);
            ctx->own_centroid = true;
            if (hipMemsetAsync(ctx->centroid, 0, pool_b, ctx->stream) != hipSuccess) return set_err(TL3D_E_HIP, "memset failed");
        }
    }
    ctx->has_core = false;
    for (int i = 0; i < 3; ++i) ctx->lat[i] = (long long)cfg->voxel_offset[i] + (i == 0 ? cfg->nx : i == 1 ? cfg->ny : cfg->nz);
    ctx->cfg.channels = cfg->channels;
    ctx->cfg.nx = cfg->nx; ctx->cfg.ny = cfg->ny; ctx->cfg.nz = cfg->nz;
    for (int i = 0; i < 3; ++i) ctx->cfg.voxel_offset[i] = cfg->voxel_offset[i];
    for (int i = 0; i < 3; ++i) ctx->cfg.origin[i] = cfg->origin[i];
    ctx->cfg.voxel_size = cfg->voxel_size;
    ctx->cfg.sdf_trunc = cfg->sdf_trunc;
    return TL3D_OK;
}

extern "C" {

const char *tl3d_last_error(void) { return g_err; }
int tl3d_version(void) { return TL3D_ABI_VERSION; }

int tl3d_runtime_info(int *hip_compiled, int *hip_runtime, int *hip_driver) {
    REQUIRE(hip_compiled && hip_runtime && hip_driver, TL3D_E_INVALID, "null out pointer");
    *hip_compiled = HIP_VERSION;
    *hip_runtime = *hip_driver = 0;
    if (hipRuntimeGetVersion(hip_runtime) != hipSuccess) (void)hipGetLastError();
    if (hipDriverGetVersion(hip_driver) != hipSuccess) (void)hipGetLastError();
    return TL3D_OK;
}

int tl3d_probe_hw_queues(int device, int n_streams, double spin_ms, double *elapsed_ms) {
    REQUIRE(elapsed_ms != nullptr, TL3D_E_INVALID, "null out pointer");
    REQUIRE(n_streams >= 1 && n_streams <= 256 && spin_ms > 0 && spin_ms <= 50, TL3D_E_INVALID, "bad probe arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return set_err(TL3D_E_NODEVICE, "no HIP device visible");
    }
    REQUIRE(device >= 0 && device < ndev, TL3D_E_INVALID, "device %d out of range [0,%d)", device, ndev);
    TL3D_HIP(hipSetDevice(device));
    return probe_hw_queues(n_streams, spin_ms, elapsed_ms);
}

int tl3d_device_count(int *n) {
    REQUIRE(n != nullptr, TL3D_E_INVALID, "null out pointer");
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) {
        (void)hipGetLastError();
        c = 0;
    }
    *n = c;
    return TL3D_OK;
}

int tl3d_create(const tl3d_config *cfg, int device, tl3d_ctx **out) {
    REQUIRE(cfg && out, TL3D_E_INVALID, "null argument");
    REQUIRE(cfg->abi_version == TL3D_ABI_VERSION, TL3D_E_INVALID, "ABI version %d != %d", cfg->abi_version, TL3D_ABI_VERSION);
    REQUIRE(cfg->width > 0 && cfg->height > 0 && cfg->width <= 32768 && cfg->height <= 32768, TL3D_E_INVALID,
            "bad frame size %dx%d", cfg->width, cfg->height);
    REQUIRE(cfg->fx > 0 && cfg->fy > 0, TL3D_E_INVALID, "focal lengths must be positive");
    REQUIRE(cfg->n_slots >= 1 && cfg->n_slots <= (1 << 20), TL3D_E_INVALID, "n_slots %d out of range", cfg->n_slots);
    if (cfg->channels) {
        const int vrc = validate_grid(cfg);
        if (vrc) return vrc;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return set_err(TL3D_E_NODEVICE, "no HIP device visible (libtl3d has no CPU fallback)");
    }
    REQUIRE(device >= 0 && device < ndev, TL3D_E_INVALID, "device %d out of range [0,%d)", device, ndev);
    TL3D_HIP(hipSetDevice(device));

    tl3d_ctx *ctx = new (std::nothrow) tl3d_ctx();
    REQUIRE(ctx != nullptr, TL3D_E_NOMEM, "host allocation failed");
    memset(ctx, 0, sizeof(*ctx));
    ctx->cfg = *cfg;
    ctx->device = device;
    {   // the per-slot TSDF tile cache is a product feature with an off switch for A/B runs (every look-up a miss): read here, once
        const char *v = getenv("TL3D_TILE_CACHE");
        ctx->tile_cache = !(v && atoi(v) == 0);
        // ... and so is the classification cache beside it (Slot::cls): its switch, and the entries (MIXED + FREE bricks of one
        // frame) a slot's buffer holds.  Default 49 152 = 288 KB per slot: a headline frame (512^3 voxels at 5 mm, 1080 x 1920)
        // lists ~15.4 k MIXED + ~10.2 k FREE bricks, a little over half of that.
        v = getenv("TL3D_CLASS_CACHE");
        ctx->class_cache = !(v && atoi(v) == 0);
        v = getenv("TL3D_CLASS_REFINE");                 // 0: replayed entries stay at level 2 (class_refine_kernel never runs)
        ctx->class_refine = !(v && atoi(v) == 0);
        v = getenv("TL3D_CLASS_CACHE_ENTRIES");
        const long long e = v ? atoll(v) : 49152;
        ctx->cc_entries = (unsigned)(e < 1 ? 1 : e > (1ll << 26) ? (1ll << 26) : e);
    }
    ctx->slots = new (std::nothrow) Slot[cfg->n_slots];
    if (!ctx->slots) { delete ctx; return set_err(TL3D_E_NOMEM, "host allocation failed"); }
    {
        const size_t npx = (size_t)cfg->width * cfg->height;
        const size_t npm = pm_pixels(cfg->width, cfg->height);      // normal maps and averaged depth: phase-major rows of 4 * ceil(W / 4) entries
        Cam tc;
        memset(&tc, 0, sizeof(tc));
        tc.W = cfg->width; tc.H = cfg->height;
        // The TSDF tile cache (Slot::tiles) and, behind it in the same block, the classification cache (Slot::cls): one pool, so
        // that a slot's first fusion costs one slab allocation per 64 slots, as before the second cache.
        ctx->tc_bytes = (tsdf_tile_cache_bytes(tc, nullptr, nullptr) + 16 + 255) & ~(size_t)255;
        ctx->cc_bytes = ctx->class_cache && ctx->tile_cache ? tsdf_class_cache_bytes(ctx->cc_entries) : 0;
        const size_t bytes[7] = {npx * sizeof(float), npx * sizeof(uint16_t), npx * 3, npm * sizeof(float4), npm * sizeof(float), ctx->tc_bytes + ctx->cc_bytes - 16,
                                 npm * sizeof(float4)};
        FramePool *pools[7] = {&ctx->pool_depth, &ctx->pool_u16, &ctx->pool_bgr, &ctx->pool_nmap, &ctx->pool_sdepth, &ctx->pool_tiles, &ctx->pool_imap};
        for (int k = 0; k < 7; ++k) {
            FramePool &fp = *pools[k];
            fp.block = (bytes[k] + 16 + 255) & ~(size_t)255;      // 16 B of slack: a pixel's 3 colour bytes are read as one 4-byte word
            fp.remaining = cfg->n_slots;
            fp.max_slabs = (cfg->n_slots + FRAME_SLAB_BLOCKS - 1) / FRAME_SLAB_BLOCKS;
            fp.slabs = (void **)calloc((size_t)fp.max_slabs, sizeof(void *));
            fp.slab_bytes = (size_t *)calloc((size_t)fp.max_slabs, sizeof(size_t));
            fp.device = device;
            if (!fp.slabs || !fp.slab_bytes) { (void)tl3d_destroy(ctx); return set_err(TL3D_E_NOMEM, "host allocation failed"); }
        }
    }

    Cam &c = ctx->cam;
    c.W = cfg->width; c.H = cfg->height;
    c.fxd = cfg->fx; c.fyd = cfg->fy; c.cxd = cfg->cx; c.cyd = cfg->cy;
    c.fx = (float)cfg->fx; c.fy = (float)cfg->fy; c.cx = (float)cfg->cx; c.cy = (float)cfg->cy;
    Grid &g = ctx->grid;
    memset(&g, 0, sizeof(g));
    auto fail = [&](int code) { tl3d_destroy(ctx); return code; };

    if (cfg->stream) {
        ctx->stream = (hipStream_t)cfg->stream;
        ctx->own_stream = false;
    } else {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return fail(set_err(TL3D_E_HIP, "stream create failed"));
        ctx->own_stream = true;
    }
    if (cfg->channels) {
        const int grc = alloc_grid(ctx, cfg);
        if (grc) return fail(grc);
    }
    // (16 counters of the update kernel, then ClassPlan::stats: the 4 of the classification cache and the 5 of its refinement)
    if (hipMalloc(&ctx->d_counters, 32 * sizeof(unsigned long long)) != hipSuccess) return fail(set_err(TL3D_E_NOMEM, "alloc failed"));
    if (hipMemsetAsync(ctx->d_counters, 0, 32 * sizeof(unsigned long long), ctx->stream) != hipSuccess) return fail(set_err(TL3D_E_HIP, "memset failed"));
    ctx->d_cc_stats = ctx->d_counters + 16;
    if (hipMalloc(&ctx->d_cen_counters, 256 * 8 * sizeof(unsigned long long)) != hipSuccess) return fail(set_err(TL3D_E_NOMEM, "alloc failed"));
    if (hipMemsetAsync(ctx->d_cen_counters, 0, 256 * 8 * sizeof(unsigned long long), ctx->stream) != hipSuccess) return fail(set_err(TL3D_E_HIP, "memset failed"));
    if (hipMalloc(&ctx->bounds_slab, 1024 * 6 * sizeof(float)) != hipSuccess) return fail(set_err(TL3D_E_NOMEM, "alloc failed"));
    {   // projection-factor tables: the two cached maps of the reference (D2R:287-295) are separable, so W + H doubles hold
        // them; computed on the host with the same fp64 expression the kernels used per pixel
        std::vector<double> f((size_t)c.W + c.H);
        for (int u = 0; u < c.W; ++u) f[u] = ((double)u - c.cxd) / c.fxd;
        for (int v = 0; v < c.H; ++v) f[(size_t)c.W + v] = ((double)v - c.cyd) / c.fyd;
        if (hipMalloc(&ctx->bp_factors, f.size() * sizeof(double)) != hipSuccess) return fail(set_err(TL3D_E_NOMEM, "alloc failed"));
        if (hipMemcpy(ctx->bp_factors, f.data(), f.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(set_err(TL3D_E_HIP, "copy failed"));
    }
    for (int i = 0; i < 2; ++i)
        if (hipEventCreate(&ctx->ev[i]) != hipSuccess) return fail(set_err(TL3D_E_HIP, "event create failed"));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(set_err(TL3D_E_HIP, "sync failed"));
    *out = ctx;
    return TL3D_OK;
}

// One block of a frame pool (nullptr when the device is out of memory).  A slab is sized for the slots still without a
// buffer of this kind, at most FRAME_SLAB_BLOCKS of them, so a context never holds more than it was created for.
// Frame slabs outlive their context in a PROCESS-WIDE CACHE (by device and size): a process that reconstructs one sequence after
// another creates a context per sequence, and memory the driver has just taken back comes out of hipMalloc at ~26 GB/s -- the
// second reconstruct() of a 1000-frame 720p sequence spent 0.7 s re-allocating the 25 GB its predecessor had freed, five times its
// whole first run (tools/run_config.py --config 4, round 4).  A released slab is kept (nothing on the device refers to it any
// more: tl3d_destroy has waited for the device) and handed to the next pool that asks for exactly that size; at most
// SLAB_CACHE_LIMIT bytes stay cached, the rest is freed at once; tl3d_release_cached_memory() frees everything (a host that
// shares the GPU with another allocator calls it when it is done with a batch of sequences).
namespace {
struct CachedSlab { int device; size_t bytes; void *p; };
std::mutex g_slab_mutex;
std::vector<CachedSlab> g_slab_cache;
size_t g_slab_cached = 0;
constexpr size_t SLAB_CACHE_LIMIT = (size_t)64 << 30;

void *slab_alloc(int device, size_t bytes) {
    {
        std::lock_guard<std::mutex> lk(g_slab_mutex);
        for (size_t i = g_slab_cache.size(); i-- > 0;)
            if (g_slab_cache[i].device == device && g_slab_cache[i].bytes == bytes) {
                void *p = g_slab_cache[i].p;
                g_slab_cached -= bytes;
                g_slab_cache.erase(g_slab_cache.begin() + (long)i);
                return p;
            }
    }
    void *p = nullptr;
    if (hipMalloc(&p, bytes) == hipSuccess) return p;
    (void)hipGetLastError();
    // out of memory with slabs of other sizes in the cache: give them back and try once more
    if (tl3d_release_cached_memory() == TL3D_OK && hipMalloc(&p, bytes) == hipSuccess) return p;
    (void)hipGetLastError();
    return nullptr;
}

void slab_free(int device, size_t bytes, void *p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_slab_mutex);
        if (g_slab_cached + bytes <= SLAB_CACHE_LIMIT) {
            g_slab_cache.push_back({device, bytes, p});
            g_slab_cached += bytes;
            return;
        }
    }
    (void)hipFree(p);
}
}  // namespace

extern "C++" void *tl3d::pool_take(FramePool &fp) {
    if (fp.cur_left == 0) {
        if (fp.remaining <= 0 || fp.n_slabs >= fp.max_slabs) return nullptr;
        const int nb = fp.remaining < FRAME_SLAB_BLOCKS ? fp.remaining : FRAME_SLAB_BLOCKS;
        void *p = slab_alloc(fp.device, fp.block * (size_t)nb);
        if (!p) return nullptr;
        fp.slab_bytes[fp.n_slabs] = fp.block * (size_t)nb;
        fp.slabs[fp.n_slabs++] = p;
        fp.cur = (char *)p;
        fp.cur_left = nb;
    }
    void *out = fp.cur;
    fp.cur += fp.block;
    --fp.cur_left;
    --fp.remaining;
    return out;
}

// (the caller has waited for the device: nothing in flight refers to the slabs)
static void pool_release(FramePool &fp) {
    for (int i = 0; i < fp.n_slabs; ++i) slab_free(fp.device, fp.slab_bytes[i], fp.slabs[i]);
    free(fp.slabs);
    free(fp.slab_bytes);
    fp.slabs = nullptr;
    fp.slab_bytes = nullptr;
    fp.n_slabs = fp.max_slabs = 0;
}

int tl3d_release_cached_memory(void) {
    std::vector<CachedSlab> take;
    {
        std::lock_guard<std::mutex> lk(g_slab_mutex);
        take.swap(g_slab_cache);
        g_slab_cached = 0;
    }
    int dev0 = -1;
    (void)hipGetDevice(&dev0);
    for (const CachedSlab &c : take) {
        (void)hipSetDevice(c.device);
        (void)hipFree(c.p);
    }
    if (dev0 >= 0) (void)hipSetDevice(dev0);
    return TL3D_OK;
}

int tl3d_destroy(tl3d_ctx *ctx) {
    if (!ctx) return TL3D_OK;
    (void)hipSetDevice(ctx->device);
    (void)flush_updates(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    (void)hipDeviceSynchronize();                           // the frame slabs go to the process-wide cache, not back to the driver: nothing may still read them
    if (ctx->slots) {
        for (int i = 0; i < ctx->cfg.n_slots; ++i) {
            if (ctx->slots[i].ev_upload) (void)hipEventDestroy(ctx->slots[i].ev_upload);
            if (ctx->slots[i].ev_normals) (void)hipEventDestroy(ctx->slots[i].ev_normals);
            if (ctx->slots[i].ev_intensity) (void)hipEventDestroy(ctx->slots[i].ev_intensity);
        }
        delete[] ctx->slots;
    }
    pool_release(ctx->pool_depth);
    pool_release(ctx->pool_u16);
    pool_release(ctx->pool_bgr);
    pool_release(ctx->pool_nmap);
    pool_release(ctx->pool_sdepth);
    pool_release(ctx->pool_tiles);
    pool_release(ctx->pool_imap);
    for (int q = 0; q < 4; ++q)
        if (ctx->prep_stream[q]) (void)hipStreamSynchronize(ctx->prep_stream[q]);
    release_grid(ctx);
    for (int b = 0; b < TSDF_SCRATCHES; ++b)
        if (ctx->ev_prep[b]) (void)hipEventDestroy(ctx->ev_prep[b]);
    for (int q = 0; q < 4; ++q)
        if (ctx->prep_stream[q]) (void)hipStreamDestroy(ctx->prep_stream[q]);
    if (ctx->ray_depth) (void)hipFree(ctx->ray_depth);
    if (ctx->ray_nrm) (void)hipFree(ctx->ray_nrm);
    if (ctx->ray_bgr) (void)hipFree(ctx->ray_bgr);
    if (ctx->bp_state) (void)hipFree(ctx->bp_state);
    if (ctx->bp_factors) (void)hipFree(ctx->bp_factors);
    if (ctx->bp_stage_xyz) (void)hipFree(ctx->bp_stage_xyz);
    if (ctx->bp_stage_rgb) (void)hipFree(ctx->bp_stage_rgb);
    if (ctx->d_counters) (void)hipFree(ctx->d_counters);
    if (ctx->d_cen_frames) (void)hipFree(ctx->d_cen_frames);
    if (ctx->d_cen_counters) (void)hipFree(ctx->d_cen_counters);
    if (ctx->rccl_comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(ctx->rccl_comm);
    if (ctx->d_maxw) (void)hipFree(ctx->d_maxw);
    if (ctx->ev_free) (void)hipEventDestroy(ctx->ev_free);
    registration_release(ctx);
    if (ctx->bounds_slab) (void)hipFree(ctx->bounds_slab);
    for (int i = 0; i < 2; ++i)
        if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    if (ctx->ktimers) {
        for (int i = 0; i < ctx->n_ktimers; ++i) {
            (void)hipEventDestroy(ctx->ktimers[i].a);
            (void)hipEventDestroy(ctx->ktimers[i].b);
        }
        delete[] ctx->ktimers;
    }
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return TL3D_OK;
}

int tl3d_sync(tl3d_ctx *ctx) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    FLUSH_AND_FOLD(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    for (int q = 0; q < 4; ++q)
        if (ctx->prep_stream[q]) TL3D_HIP(hipStreamSynchronize(ctx->prep_stream[q]));
    for (int l = 0; l < TL3D_ICP_LANES; ++l)
        if (ctx->icp_lanes[l].stream) TL3D_HIP(hipStreamSynchronize(ctx->icp_lanes[l].stream));
    if (ctx->icp_batch.stream) TL3D_HIP(hipStreamSynchronize(ctx->icp_batch.stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    ctx->tc_done_before = ctx->tsdf_batch_no;
    if (ctx->bp_async_pending && ctx->bp_state) {
        ctx->bp_async_pending = false;
        unsigned long long err = 0;
        TL3D_HIP(hipMemcpy(&err, ctx->bp_state + 1, sizeof(err), hipMemcpyDeviceToHost));
        const int erc = bp_check_error(ctx, err);
        if (erc) return erc;
    }
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- frames
int tl3d_get_stream(tl3d_ctx *ctx, void **stream) {
    REQUIRE(ctx && stream, TL3D_E_INVALID, "null argument");
    *stream = (void *)ctx->stream;
    return TL3D_OK;
}

int tl3d_upload_frame(tl3d_ctx *ctx, int slot, const void *depth_hd, int depth_kind, const uint8_t *bgr_hd) {
    return upload_impl(ctx, slot, depth_hd, depth_kind, bgr_hd, true);
}

// ---- host helpers of the decode pipeline (no device work) -----------------------------------------------------------------
int tl3d_host_pack_bgr_rows(uint8_t *dst, const uint8_t *const *rows, int height, int width) {
    REQUIRE(dst && rows && height >= 0 && width >= 0, TL3D_E_INVALID, "bad argument");
    for (int y = 0; y < height; ++y) {
        const uint8_t *__restrict__ s = rows[y];
        uint8_t *__restrict__ d = dst + (size_t)y * width * 3;
        REQUIRE(s != nullptr, TL3D_E_INVALID, "null row %d", y);
        for (int x = 0; x < width; ++x) {
            d[3 * x + 0] = s[4 * x + 2];
            d[3 * x + 1] = s[4 * x + 1];
            d[3 * x + 2] = s[4 * x + 0];
        }
    }
    return TL3D_OK;
}

int tl3d_host_copy_rows(uint8_t *dst, const uint8_t *const *rows, int height, size_t row_bytes) {
    REQUIRE(dst && rows && height >= 0, TL3D_E_INVALID, "bad argument");
    for (int y = 0; y < height; ++y) {
        REQUIRE(rows[y] != nullptr, TL3D_E_INVALID, "null row %d", y);
        memcpy(dst + (size_t)y * row_bytes, rows[y], row_bytes);
    }
    return TL3D_OK;
}

}  // extern "C"

// The slot's depth image was rewritten on the main stream (an upload, a ray cast into the slot).  What was derived from the previous
// frame is void: the normal map, the averaged depth, the TSDF tiles (their users are ahead of the writer on the main stream; the
// classification goes when the tiles are rebuilt).  The prep streams wait on ev_upload, not on the whole main stream.
static int slot_rewritten(tl3d_ctx *ctx, Slot &s, bool has_u16, bool has_color) {
    s.has_u16 = has_u16;
    s.has_color = has_color;
    s.loaded = true;
    s.has_normals = false;
    s.has_intensity = false;
    s.smooth_radius = 0;
    s.tc.valid = s.tc.used = false;
    if (!s.ev_upload) TL3D_HIP(hipEventCreateWithFlags(&s.ev_upload, hipEventDisableTiming));
    TL3D_HIP(hipEventRecord(s.ev_upload, ctx->stream));
    return TL3D_OK;
}

static int upload_impl(tl3d_ctx *ctx, int slot, const void *depth_hd, int depth_kind, const uint8_t *bgr_hd, bool wait) {
    int rc = check_slot(ctx, slot, false);
    if (rc) return rc;
    REQUIRE(depth_hd != nullptr, TL3D_E_INVALID, "null depth");
    REQUIRE(depth_kind == TL3D_DEPTH_F32_M || depth_kind == TL3D_DEPTH_U16_MM, TL3D_E_INVALID, "bad depth_kind %d", depth_kind);
    FLUSH_UPDATES(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    rc = order_after_lanes(ctx, slot, true, false);     // an uncollected ICP run may still read this slot's depth
    if (rc) return rc;
    Slot &s = ctx->slots[slot];
    const size_t npx = (size_t)ctx->cam.W * ctx->cam.H;
    if (!s.depth && !(s.depth = (float *)pool_take(ctx->pool_depth))) return set_err(TL3D_E_NOMEM, "frame alloc failed");
    if (depth_kind == TL3D_DEPTH_F32_M) {
        TL3D_HIP(hipMemcpyAsync(s.depth, depth_hd, npx * sizeof(float), hipMemcpyDefault, ctx->stream));
    } else {
        // the millimetre image stays beside its f32 conversion: the TSDF kernels gather from it (half the cache lines
        // under a brick's footprint) and convert with the same IEEE division, every other kernel reads the f32 copy
        if (!s.depth_u16 && !(s.depth_u16 = (uint16_t *)pool_take(ctx->pool_u16))) return set_err(TL3D_E_NOMEM, "frame alloc failed");
        TL3D_HIP(hipMemcpyAsync(s.depth_u16, depth_hd, npx * sizeof(uint16_t), hipMemcpyDefault, ctx->stream));
        rc = launch_u16_to_f32(ctx->stream, s.depth_u16, s.depth, npx);
        if (rc) return rc;
    }
    if (bgr_hd) {
        if (!s.bgr && !(s.bgr = (uint8_t *)pool_take(ctx->pool_bgr))) return set_err(TL3D_E_NOMEM, "frame alloc failed");
        TL3D_HIP(hipMemcpyAsync(s.bgr, bgr_hd, npx * 3, hipMemcpyDefault, ctx->stream));
    }
    rc = slot_rewritten(ctx, s, depth_kind == TL3D_DEPTH_U16_MM, bgr_hd != nullptr);
    if (rc) return rc;
    // pageable host sources are consumed before hipMemcpyAsync returns only for small copies; make the hand-over explicit
    if (wait && (!is_device_ptr(depth_hd) || (bgr_hd && !is_device_ptr(bgr_hd)))) TL3D_HIP(hipStreamSynchronize(ctx->stream));
    return TL3D_OK;
}

extern "C" {

int tl3d_attach_grid(tl3d_ctx *ctx, const tl3d_config *cfg) {
    REQUIRE(ctx && cfg, TL3D_E_INVALID, "null argument");
    REQUIRE(ctx->tsdf == nullptr && ctx->centroid == nullptr, TL3D_E_STATE, "context already has a grid");
    int rc = validate_grid(cfg);
    if (rc) return rc;
    TL3D_HIP(hipSetDevice(ctx->device));
    rc = alloc_grid(ctx, cfg);
    if (rc) return rc;
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    return TL3D_OK;
}

int tl3d_detach_grid(tl3d_ctx *ctx) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(ctx->tsdf != nullptr || ctx->centroid != nullptr, TL3D_E_STATE, "context has no grid");
    FLUSH_UPDATES(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    for (int q = 0; q < 4; ++q)
        if (ctx->prep_stream[q]) TL3D_HIP(hipStreamSynchronize(ctx->prep_stream[q]));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    release_grid(ctx);
    return TL3D_OK;
}

int tl3d_set_block_core(tl3d_ctx *ctx, const int64_t lattice_dims[3], const int32_t lo[3], const int32_t hi[3]) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(ctx->tsdf != nullptr || ctx->centroid != nullptr, TL3D_E_STATE, "context has no grid");
    Grid &g = ctx->grid;
    const int dims[3] = {g.nx, g.ny, g.nz};
    const int64_t off[3] = {ctx->cfg.voxel_offset[0], ctx->cfg.voxel_offset[1], ctx->cfg.voxel_offset[2]};
    if (lattice_dims || lo || hi) {
        REQUIRE(lattice_dims && lo && hi, TL3D_E_INVALID, "lattice_dims, lo and hi are all given or all NULL");
        double nlat = 1.0;
        for (int a = 0; a < 3; ++a) {
            REQUIRE(lo[a] >= 0 && lo[a] < hi[a] && hi[a] <= dims[a] && lo[a] % TL3D_BRICK == 0 && hi[a] % TL3D_BRICK == 0, TL3D_E_INVALID,
                    "core [%d, %d) on axis %d must be a non-empty range of multiples of %d within the grid's %d voxels", lo[a], hi[a], a,
                    TL3D_BRICK, dims[a]);
            REQUIRE(lattice_dims[a] >= off[a] + dims[a], TL3D_E_INVALID, "lattice of %lld voxels on axis %d does not hold the grid (%lld + %d)",
                    (long long)lattice_dims[a], a, (long long)off[a], dims[a]);
            nlat *= (double)lattice_dims[a];
        }
        REQUIRE(nlat < 2305843009213693952.0, TL3D_E_INVALID, "lattice of 2^61 voxels or more: mesh keys would overflow");
    }
    FLUSH_UPDATES(ctx);
    for (int a = 0; a < 3; ++a) {
        g.clo[a] = lattice_dims ? lo[a] : 0;
        g.chi[a] = lattice_dims ? hi[a] : dims[a];
        ctx->lat[a] = lattice_dims ? (long long)lattice_dims[a] : (long long)off[a] + dims[a];
    }
    ctx->has_core = lattice_dims != nullptr;
    ctx->ext_valid = ctx->mesh_valid = false;
    ctx->grid_epoch++;
    return TL3D_OK;
}

int tl3d_pinned_alloc(size_t bytes, void **out) {
    REQUIRE(out != nullptr && bytes > 0, TL3D_E_INVALID, "bad argument");
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(TL3D_E_NOMEM, "pinned allocation of %zu B failed", bytes);
    }
    return TL3D_OK;
}

int tl3d_pinned_free(void *p) {
    if (p && hipHostFree(p) != hipSuccess) return set_err(TL3D_E_HIP, "hipHostFree failed");
    return TL3D_OK;
}

int tl3d_upload_frame_async(tl3d_ctx *ctx, int slot, const void *depth_hd, int depth_kind, const uint8_t *bgr_hd) {
    return upload_impl(ctx, slot, depth_hd, depth_kind, bgr_hd, false);
}

int tl3d_slot_wait(tl3d_ctx *ctx, int slot) {
    int rc = check_slot(ctx, slot, true);
    if (rc) return rc;
    TL3D_HIP(hipSetDevice(ctx->device));
    if (ctx->slots[slot].ev_upload) TL3D_HIP(hipEventSynchronize(ctx->slots[slot].ev_upload));
    return TL3D_OK;
}

int tl3d_download_depth(tl3d_ctx *ctx, int slot, float *out) {
    int rc = check_slot(ctx, slot, true);
    if (rc) return rc;
    REQUIRE(out != nullptr, TL3D_E_INVALID, "null out");
    TL3D_HIP(hipSetDevice(ctx->device));
    TL3D_HIP(hipMemcpyAsync(out, ctx->slots[slot].depth, (size_t)ctx->cam.W * ctx->cam.H * sizeof(float), hipMemcpyDefault, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- depth-frame filter (kernels_depthfilter.hip)
// what both calls check before any device work
static int depth_filter_check(const tl3d_depth_filter_params *p) {
    REQUIRE(isfinite(p->jump_rel) && p->jump_rel > 0, TL3D_E_INVALID, "jump_rel must be finite and positive");
    REQUIRE(p->radius >= 1 && p->radius <= 3, TL3D_E_INVALID, "radius %d outside [1,3]", p->radius);
    const int window = (2 * p->radius + 1) * (2 * p->radius + 1);
    REQUIRE(p->min_support >= 0 && p->min_support <= window - 1, TL3D_E_INVALID, "min_support %d outside [0,%d]", p->min_support, window - 1);
    REQUIRE(p->min_region >= 0, TL3D_E_INVALID, "min_region must not be negative");
    REQUIRE(p->reserved == 0, TL3D_E_INVALID, "reserved must be 0");
    return TL3D_OK;
}

int tl3d_filter_depth(tl3d_ctx *ctx, const void *depth_in, int depth_kind, const tl3d_depth_filter_params *params, void *depth_out,
                      int64_t *counts_out) {
    REQUIRE(ctx && depth_in && params && depth_out && counts_out, TL3D_E_INVALID, "null argument");
    REQUIRE(depth_kind == TL3D_DEPTH_F32_M || depth_kind == TL3D_DEPTH_U16_MM, TL3D_E_INVALID, "bad depth_kind %d", depth_kind);
    int rc = depth_filter_check(params);
    if (rc) return rc;
    const size_t bytes = (size_t)ctx->cam.W * ctx->cam.H * (depth_kind == TL3D_DEPTH_U16_MM ? sizeof(uint16_t) : sizeof(float));
    REQUIRE(depth_out == depth_in || !ranges_overlap(depth_out, bytes, depth_in, bytes), TL3D_E_INVALID, "the output overlaps the input");
    REQUIRE(!ranges_overlap(counts_out, 4 * sizeof(int64_t), depth_in, bytes) && !ranges_overlap(counts_out, 4 * sizeof(int64_t), depth_out, bytes),
            TL3D_E_INVALID, "the counts overlap an image");
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    char *dout = nullptr;
    rc = st.out((char *)depth_out, bytes, &dout);
    if (rc) return rc;
    // the kernels work in place on the output: it starts as the input's bytes (invalid pixels keep theirs)
    if ((const void *)dout != depth_in) TL3D_HIP(hipMemcpyAsync(dout, depth_in, bytes, hipMemcpyDefault, ctx->stream));
    void *img = dout;
    long long counts[4] = {0, 0, 0, 0};
    rc = st.finish(depth_filter_run(ctx, 1, &img, nullptr, &depth_kind, *params, counts), true);
    if (rc) return rc;
    for (int i = 0; i < 4; ++i) counts_out[i] = counts[i];
    return TL3D_OK;
}

int tl3d_filter_depth_slots(tl3d_ctx *ctx, int n, const int32_t *slots, const tl3d_depth_filter_params *params, int64_t *counts_out) {
    REQUIRE(ctx && params && n >= 0 && (slots || n == 0), TL3D_E_INVALID, "null argument or negative n");
    int rc = depth_filter_check(params);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        REQUIRE(slots[i] >= 0 && slots[i] < ctx->cfg.n_slots, TL3D_E_INVALID, "slot %d out of range [0,%d)", slots[i], ctx->cfg.n_slots);
        for (int j = 0; j < i; ++j) REQUIRE(slots[j] != slots[i], TL3D_E_INVALID, "slot %d named twice", slots[i]);
    }
    for (int i = 0; i < n; ++i) REQUIRE(ctx->slots[slots[i]].loaded, TL3D_E_STATE, "slot %d holds no frame", slots[i]);
    if (n == 0) return TL3D_OK;
    // each slot as upload_impl treats a rewrite: behind the deferred updates and the lanes that read it, the kernels on the main
    // stream, then slot_rewritten (normal map, averaged depth, tile and class caches void; ev_upload recorded)
    FLUSH_UPDATES(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    std::vector<void *> img(n);
    std::vector<float *> f32(n);
    std::vector<int> kinds(n);
    std::vector<long long> counts(counts_out ? (size_t)n * 4 : 0);
    for (int i = 0; i < n; ++i) {
        rc = order_after_lanes(ctx, slots[i], true, true);
        if (rc) return rc;
        Slot &s = ctx->slots[slots[i]];
        kinds[i] = s.has_u16 ? TL3D_DEPTH_U16_MM : TL3D_DEPTH_F32_M;
        img[i] = s.has_u16 ? (void *)s.depth_u16 : (void *)s.depth;
        f32[i] = s.has_u16 ? s.depth : nullptr;
    }
    rc = depth_filter_run(ctx, n, img.data(), f32.data(), kinds.data(), *params, counts_out ? counts.data() : nullptr);
    // (after a failed launch too: some of the slots may have been written)
    for (int i = 0; i < n; ++i) {
        Slot &s = ctx->slots[slots[i]];
        const int rrc = slot_rewritten(ctx, s, s.has_u16, s.has_color);
        if (!rc) rc = rrc;
    }
    if (rc) return rc;
    for (size_t i = 0; i < counts.size(); ++i) counts_out[i] = counts[i];
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- back-projection
extern "C++" int tl3d::make_bp_args(tl3d_ctx *ctx, double scale, uint32_t flags, int subsample, double min_d, double max_d, BpArgs *a) {
    REQUIRE(subsample >= 1, TL3D_E_INVALID, "subsample must be >= 1");
    REQUIRE((flags & ~(TL3D_F_SCALE_F64 | TL3D_F_NO_POSE)) == 0, TL3D_E_INVALID, "unknown flags 0x%x", flags);
    a->sub = subsample;
    a->Ws = (ctx->cam.W + subsample - 1) / subsample;
    a->Hs = (ctx->cam.H + subsample - 1) / subsample;
    a->flags = flags;
    a->scale = scale;
    a->min_d = min_d;
    a->max_d = max_d;
    a->zero = 0ull;
    return TL3D_OK;
}

// scratch of the one-launch back-projection (layout: kernels_backproject.hip), + one word at the end for the total.  Zeroed
// here once; every launch leaves it zero again (the tile that finishes last re-arms it), except the error word.
static int bp_ensure_state(tl3d_ctx *ctx, const BpArgs &a) {
    const size_t need = (size_t)bp_state_words(a) + 2;
    if (need <= ctx->bp_state_words) return TL3D_OK;
    if (ctx->bp_state) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(ctx->bp_state);
    }
    ctx->bp_state = nullptr;
    ctx->bp_state_words = 0;
    const size_t words = need * 2;                                  // headroom: a later, larger subsample-1 call re-uses it
    if (hipMalloc(&ctx->bp_state, words * sizeof(unsigned long long)) != hipSuccess) return set_err(TL3D_E_NOMEM, "back-projection scratch alloc failed");
    if (hipMemsetAsync(ctx->bp_state, 0, words * sizeof(unsigned long long), ctx->stream) != hipSuccess) return set_err(TL3D_E_HIP, "memset failed");
    ctx->bp_state_words = words;
    return TL3D_OK;
}

// a look-back time-out leaves the scratch in an unknown state: report it and start from zeroes again
static int bp_check_error(tl3d_ctx *ctx, unsigned long long err) {
    if (err == 0) return TL3D_OK;
    (void)hipMemsetAsync(ctx->bp_state, 0, ctx->bp_state_words * sizeof(unsigned long long), ctx->stream);
    return set_err(TL3D_E_HIP, "back-projection look-back timed out (a predecessor tile never published)");
}

int tl3d_backproject(tl3d_ctx *ctx, int slot, const double R[9], const double t[3], double scale, uint32_t flags,
                     int subsample, double min_depth, double max_depth, float *out_xyz, uint8_t *out_rgb, int64_t cap,
                     int64_t *out_n) {
    int rc = check_slot(ctx, slot, true);
    if (rc) return rc;
    REQUIRE(out_n != nullptr, TL3D_E_INVALID, "null out_n");
    REQUIRE((flags & TL3D_F_NO_POSE) || (R && t), TL3D_E_INVALID, "pose required unless TL3D_F_NO_POSE");
    BpArgs a;
    rc = make_bp_args(ctx, scale, flags, subsample, min_depth, max_depth, &a);
    if (rc) return rc;
    TL3D_HIP(hipSetDevice(ctx->device));
    const Slot &s = ctx->slots[slot];
    rc = bp_ensure_state(ctx, a);
    if (rc) return rc;
    unsigned long long *d_total = ctx->bp_state + (ctx->bp_state_words - 1);
    const PoseD p = make_pose_d(R, t, (flags & TL3D_F_NO_POSE) != 0);
    const bool want = out_xyz && out_rgb;
    const bool direct = want && is_device_ptr(out_xyz) && is_device_ptr(out_rgb);
    const unsigned long long ns = (unsigned long long)a.Ws * (unsigned long long)a.Hs;
    unsigned long long cap_eff = cap < 0 ? 0ull : (unsigned long long)cap;
    float *dxyz = out_xyz;
    uint8_t *drgb = out_rgb;
    if (want && !direct) {
        // host outputs: stage on the device (buffers kept for the life of the context, sized for a full frame)
        const size_t npx = (size_t)ctx->cam.W * ctx->cam.H;
        if (!ctx->bp_stage_xyz && hipMalloc(&ctx->bp_stage_xyz, npx * 3 * sizeof(float)) != hipSuccess) return set_err(TL3D_E_NOMEM, "output staging alloc failed");
        if (!ctx->bp_stage_rgb && hipMalloc(&ctx->bp_stage_rgb, npx * 3) != hipSuccess) return set_err(TL3D_E_NOMEM, "output staging alloc failed");
        dxyz = ctx->bp_stage_xyz;
        drgb = ctx->bp_stage_rgb;
        if (cap_eff > ns) cap_eff = ns;
    }
    // ONE launch: count, ordered offsets (decoupled look-back) and LDS-staged writes; without buffers: the count only.
    // A look-back time-out (static tile order and a predecessor that never got a slot: see launch_bp_fused) is repeated
    // once in dynamic order, which cannot starve.
    unsigned long long h[2] = {0, 0};
    for (int attempt = 0; attempt < 2; ++attempt) {
        rc = launch_bp_fused(ctx->stream, ctx->cam, a, p, s.depth, s.has_color ? s.bgr : nullptr, ctx->bp_factors, ctx->bp_factors + ctx->cam.W,
                             ctx->bp_state, want ? dxyz : nullptr, want ? drgb : nullptr, cap_eff, d_total, attempt == 1);
        if (rc) return rc;
        TL3D_HIP(hipMemcpyAsync(&h[0], d_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        TL3D_HIP(hipMemcpyAsync(&h[1], ctx->bp_state + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        TL3D_HIP(hipStreamSynchronize(ctx->stream));
        rc = bp_check_error(ctx, h[1]);
        if (rc == TL3D_OK) break;
        if (attempt == 1) return rc;
        ctx->stats.bp_lookback_retries++;                               // (never seen so far; tl3d_get_stats shows it if it happens)
    }
    const unsigned long long total = h[0];
    *out_n = (int64_t)total;
    if (!want) return TL3D_OK;                                      // size query
    if ((int64_t)total > cap) return set_err(TL3D_E_CAPACITY, "need %llu points, capacity %lld", total, (long long)cap);
    if (total == 0 || direct) return TL3D_OK;
    TL3D_HIP(hipMemcpyAsync(out_xyz, dxyz, total * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipMemcpyAsync(out_rgb, drgb, total * 3, hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    return TL3D_OK;
}

int tl3d_backproject_device(tl3d_ctx *ctx, int slot, const double R[9], const double t[3], double scale, uint32_t flags,
                            int subsample, double min_depth, double max_depth, float *out_xyz_dev, uint8_t *out_rgb_dev,
                            int64_t cap, int64_t *out_n_dev) {
    int rc = check_slot(ctx, slot, true);
    if (rc) return rc;
    REQUIRE(out_xyz_dev && out_rgb_dev && out_n_dev, TL3D_E_INVALID, "null output pointer");
    REQUIRE(is_device_ptr(out_xyz_dev) && is_device_ptr(out_rgb_dev) && is_device_ptr(out_n_dev), TL3D_E_INVALID,
            "tl3d_backproject_device writes device memory only");
    REQUIRE(cap >= 0, TL3D_E_INVALID, "negative capacity");
    REQUIRE((flags & TL3D_F_NO_POSE) || (R && t), TL3D_E_INVALID, "pose required unless TL3D_F_NO_POSE");
    BpArgs a;
    rc = make_bp_args(ctx, scale, flags, subsample, min_depth, max_depth, &a);
    if (rc) return rc;
    TL3D_HIP(hipSetDevice(ctx->device));
    const Slot &s = ctx->slots[slot];
    rc = bp_ensure_state(ctx, a);
    if (rc) return rc;
    const PoseD p = make_pose_d(R, t, (flags & TL3D_F_NO_POSE) != 0);
    ctx->bp_async_pending = true;                       // tl3d_sync reports a look-back time-out of these launches
    // nobody reads the error word back between these launches: an earlier time-out must not make every later launch give up
    // (the word is cleared IN STREAM ORDER; tl3d_sync still reports a time-out of the last launch), and with a batched
    // registration spinning on the chip the static tile order's "every tile is resident" cannot be taken for granted
    TL3D_HIP(hipMemsetAsync(ctx->bp_state + 1, 0, sizeof(unsigned long long), ctx->stream));
    return launch_bp_fused(ctx->stream, ctx->cam, a, p, s.depth, s.has_color ? s.bgr : nullptr, ctx->bp_factors, ctx->bp_factors + ctx->cam.W,
                           ctx->bp_state, out_xyz_dev, out_rgb_dev, (unsigned long long)cap, reinterpret_cast<unsigned long long *>(out_n_dev),
                           ctx->icp_batch.busy);
}

int tl3d_frames_bounds(tl3d_ctx *ctx, int n_frames, const int32_t *slots, const double *R, const double *t, const double *scales,
                       uint32_t flags, int subsample, double min_depth, double max_depth, double out_min[3], double out_max[3]) {
    REQUIRE(ctx && slots && out_min && out_max, TL3D_E_INVALID, "null argument");
    REQUIRE(n_frames >= 1, TL3D_E_INVALID, "n_frames must be positive");
    REQUIRE((flags & TL3D_F_NO_POSE) || (R && t), TL3D_E_INVALID, "poses required unless TL3D_F_NO_POSE");
    for (int i = 0; i < n_frames; ++i) {
        const int rc = check_slot(ctx, slots[i], true);
        if (rc) return rc;
    }
    BpArgs a;
    int rc = make_bp_args(ctx, scales ? scales[0] : 1.0, flags, subsample, min_depth, max_depth, &a);
    if (rc) return rc;
    TL3D_HIP(hipSetDevice(ctx->device));
    const long long ns = (long long)a.Ws * a.Hs;
    int nb = (int)((ns + 255) / 256);
    if (nb > 64) nb = 64;                                  // 16 frames share the 1024-row slab between two read-backs
    const int per_round = 1024 / nb;
    for (int k = 0; k < 3; ++k) { out_min[k] = INFINITY; out_max[k] = -INFINITY; }
    std::vector<float> h((size_t)1024 * 6);
    for (int i0 = 0; i0 < n_frames; i0 += per_round) {
        const int cnt = n_frames - i0 < per_round ? n_frames - i0 : per_round;
        for (int j = 0; j < cnt; ++j) {
            const int i = i0 + j;
            if (scales) {
                rc = make_bp_args(ctx, scales[i], flags, subsample, min_depth, max_depth, &a);
                if (rc) return rc;
            }
            const PoseD p = make_pose_d(R ? R + (size_t)9 * i : nullptr, t ? t + (size_t)3 * i : nullptr, (flags & TL3D_F_NO_POSE) != 0);
            rc = launch_bp_bounds(ctx->stream, ctx->cam, a, p, ctx->slots[slots[i]].depth, ctx->bp_factors, ctx->bp_factors + ctx->cam.W,
                                  ctx->bounds_slab + (size_t)j * nb * 6, nb);
            if (rc) return rc;
        }
        TL3D_HIP(hipMemcpyAsync(h.data(), ctx->bounds_slab, (size_t)cnt * nb * 6 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        TL3D_HIP(hipStreamSynchronize(ctx->stream));
        for (int b = 0; b < cnt * nb; ++b)
            for (int k = 0; k < 3; ++k) {
                out_min[k] = fmin(out_min[k], (double)h[(size_t)b * 6 + k]);
                out_max[k] = fmax(out_max[k], (double)h[(size_t)b * 6 + 3 + k]);
            }
    }
    return TL3D_OK;
}

int tl3d_frame_bounds(tl3d_ctx *ctx, int slot, const double R[9], const double t[3], double scale, uint32_t flags, int subsample,
                      double min_depth, double max_depth, double out_min[3], double out_max[3], int64_t *out_reserved) {
    const int32_t s = slot;
    if (out_reserved) *out_reserved = 0;
    return tl3d_frames_bounds(ctx, 1, &s, R, t, &scale, flags, subsample, min_depth, max_depth, out_min, out_max);
}

int tl3d_points_bounds(tl3d_ctx *ctx, const float *xyz, int64_t n, double out_min[3], double out_max[3]) {
    REQUIRE(ctx && xyz && out_min && out_max, TL3D_E_INVALID, "null argument");
    REQUIRE(n > 0, TL3D_E_INVALID, "empty point list has no bounds");
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *d;
    int rc = st.in(xyz, (size_t)n * 12, &d);
    if (rc) return rc;
    int nb = (int)((n + 255) / 256);
    if (nb > 1024) nb = 1024;
    rc = launch_bounds(ctx->stream, d, n, ctx->bounds_slab, nb);
    if (rc) return rc;
    std::vector<float> h((size_t)nb * 6);
    TL3D_HIP(hipMemcpyAsync(h.data(), ctx->bounds_slab, h.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    for (int a = 0; a < 3; ++a) { out_min[a] = INFINITY; out_max[a] = -INFINITY; }
    for (int b = 0; b < nb; ++b)
        for (int a = 0; a < 3; ++a) {
            out_min[a] = fmin(out_min[a], (double)h[(size_t)b * 6 + a]);
            out_max[a] = fmax(out_max[a], (double)h[(size_t)b * 6 + 3 + a]);
        }
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- grids
static int grid_sel(tl3d_ctx *ctx, uint32_t channel, void **p, size_t *bytes) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    if (channel == TL3D_CH_TSDF) {
        REQUIRE(ctx->tsdf != nullptr, TL3D_E_STATE, "TSDF channel not enabled");
        *p = ctx->tsdf;
        *bytes = ctx->nvox * sizeof(int2);
    } else if (channel == TL3D_CH_CENTROID) {
        REQUIRE(ctx->centroid != nullptr, TL3D_E_STATE, "centroid channel not enabled");
        *p = ctx->centroid;
        *bytes = ctx->nvox * 32;
    } else {
        return set_err(TL3D_E_INVALID, "channel must be exactly one of TL3D_CH_TSDF / TL3D_CH_CENTROID");
    }
    return TL3D_OK;
}

int tl3d_grid_reset(tl3d_ctx *ctx) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    FLUSH_UPDATES(ctx);
    ctx->grid_epoch++;
    TL3D_HIP(hipSetDevice(ctx->device));
    if (ctx->tsdf) TL3D_HIP(hipMemsetAsync(ctx->tsdf, 0, (size_t)ctx->grid.tsdf_cap << 12, ctx->stream));
    if (ctx->centroid) TL3D_HIP(hipMemsetAsync(ctx->centroid, 0, (size_t)ctx->grid.cen_cap << 14, ctx->stream));
    if (ctx->sparse) {
        const int trc = reset_brick_tables(ctx);
        if (trc) return trc;
    }
    if (ctx->free_cnt) {
        TL3D_HIP(hipMemsetAsync(ctx->free_cnt, 0, (ctx->nvox >> 9) * sizeof(unsigned), ctx->stream));
        const int mrc = mark_free_cnt_write(ctx);
        if (mrc) return mrc;
    }
    ctx->free_dirty = false;
    ctx->tsdf_w_upper = 0;
    ctx->tsdf_w_unknown = false;
    return TL3D_OK;
}

int tl3d_grid_device_ptr(tl3d_ctx *ctx, uint32_t channel, void **ptr, size_t *bytes) {
    REQUIRE(ptr && bytes, TL3D_E_INVALID, "null out pointer");
    if (ctx && channel == TL3D_CH_FREE) {
        REQUIRE(ctx->free_cnt != nullptr, TL3D_E_STATE, "TSDF channel not enabled");
        FLUSH_UPDATES(ctx);                             // the counts as they stand (folded into the records or not: readers add what is pending)
        ctx->free_dirty = true;                         // the caller may write through the pointer (a merge sums them)
        ctx->tsdf_w_unknown = true;
        ctx->grid_epoch++;
        *ptr = ctx->free_cnt;
        *bytes = (ctx->nvox >> 9) * sizeof(unsigned);
        return TL3D_OK;
    }
    if (ctx) REQUIRE(!ctx->sparse, TL3D_E_STATE, "a sparse grid has no dense layout to point at: use tl3d_grid_download / tl3d_grid_pack_bricks");
    if (ctx) {
        FLUSH_AND_FOLD(ctx);
        ctx->grid_epoch++;                  // the caller may write through the pointer (all-reduce)
        if (channel == TL3D_CH_TSDF) ctx->tsdf_w_unknown = true;
    }
    return grid_sel(ctx, channel, ptr, bytes);
}

int tl3d_grid_download(tl3d_ctx *ctx, uint32_t channel, void *out, size_t bytes) {
    void *p;
    size_t nb;
    int rc = grid_sel(ctx, channel, &p, &nb);
    if (rc) return rc;
    FLUSH_AND_FOLD(ctx);
    REQUIRE(out && bytes == nb, TL3D_E_INVALID, "buffer is %zu B, grid channel is %zu B", bytes, nb);
    TL3D_HIP(hipSetDevice(ctx->device));
    if (ctx->sparse) {
        // the dense image of the channel (what a dense grid would hold, free-space counts folded in): bricks gathered through the table
        Staging st(ctx);
        void *dst;
        rc = st.out(out, nb, &dst);
        if (rc) return rc;
        return st.finish(launch_brick_rows(ctx->stream, ctx->grid, 0, channel == TL3D_CH_TSDF, p, nullptr, (long long)(ctx->nvox >> 9), dst, true), true);
    }
    TL3D_HIP(hipMemcpyAsync(out, p, nb, hipMemcpyDefault, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    return TL3D_OK;
}

int tl3d_grid_upload(tl3d_ctx *ctx, uint32_t channel, const void *in, size_t bytes) {
    void *p;
    size_t nb;
    int rc = grid_sel(ctx, channel, &p, &nb);
    if (rc) return rc;
    FLUSH_UPDATES(ctx);
    ctx->grid_epoch++;
    REQUIRE(in && bytes == nb, TL3D_E_INVALID, "buffer is %zu B, grid channel is %zu B", bytes, nb);
    TL3D_HIP(hipSetDevice(ctx->device));
    if (channel == TL3D_CH_TSDF) {
        ctx->tsdf_w_unknown = true;
        if (ctx->free_cnt) {                                  // the upload replaces the channel
            TL3D_HIP(hipMemsetAsync(ctx->free_cnt, 0, (ctx->nvox >> 9) * sizeof(unsigned), ctx->stream));
            const int mrc = mark_free_cnt_write(ctx);
            if (mrc) return mrc;
        }
        ctx->free_dirty = false;
    }
    if (ctx->sparse) {
        // the channel becomes the dense image `in`: bricks that hold anything get records, the others' records are cleared
        Staging st(ctx);
        const void *src;
        rc = st.in(in, nb, &src);
        if (rc) return rc;
        return st.finish(launch_brick_rows(ctx->stream, ctx->grid, 1, channel == TL3D_CH_TSDF, p, nullptr, (long long)(ctx->nvox >> 9), const_cast<void *>(src), false), true);
    }
    TL3D_HIP(hipMemcpyAsync(p, in, nb, hipMemcpyDefault, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    return TL3D_OK;
}

int tl3d_grid_add(tl3d_ctx *ctx, uint32_t channel, const void *other, size_t bytes) {
    void *p;
    size_t nb;
    int rc = grid_sel(ctx, channel, &p, &nb);
    if (rc) return rc;
    FLUSH_AND_FOLD(ctx);
    ctx->grid_epoch++;
    REQUIRE(other && bytes == nb, TL3D_E_INVALID, "buffer is %zu B, grid channel is %zu B", bytes, nb);
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const void *src;
    rc = st.in(other, nb, &src);
    if (rc) return rc;
    if (channel == TL3D_CH_TSDF) {
        // the merged weights must keep the int32 sums in range: largest weight here + largest weight there
        long long wa = ctx->tsdf_w_upper, wb = 0;
        if (ctx->tsdf_w_unknown) rc = measure_max_weight(ctx, ctx->tsdf, &wa);
        if (rc == TL3D_OK) rc = measure_max_weight(ctx, (const int2 *)src, &wb);
        if (rc == TL3D_OK && wa + wb > TL3D_TSDF_MAX_WEIGHT)
            rc = set_err(TL3D_E_STATE, "merging grids with up to %lld + %lld observations per voxel could overflow the int32 TSDF sums (limit %d)",
                         wa, wb, TL3D_TSDF_MAX_WEIGHT);
        if (rc == TL3D_OK) {
            ctx->tsdf_w_upper = wa + wb;
            ctx->tsdf_w_unknown = false;
            if (ctx->sparse && ctx->free_cnt) ctx->free_dirty = true;       // (as unpack: the next read folds the counts of bricks that get records here)
            rc = ctx->sparse ? launch_brick_rows(ctx->stream, ctx->grid, 2, true, p, nullptr, (long long)(ctx->nvox >> 9), const_cast<void *>(src), false)
                             : launch_add_i32(ctx->stream, (int *)p, (const int *)src, nb / 4);
        }
    } else
        rc = ctx->sparse ? launch_brick_rows(ctx->stream, ctx->grid, 2, false, p, nullptr, (long long)(ctx->nvox >> 9), const_cast<void *>(src), false)
                         : launch_add_u64(ctx->stream, (unsigned long long *)p, (const unsigned long long *)src, nb / 8);
    return st.finish(rc);
}

int tl3d_grid_touched_bricks(tl3d_ctx *ctx, uint32_t channels, uint8_t *map_dev, int64_t n_bricks) {
    REQUIRE(ctx && map_dev, TL3D_E_INVALID, "null argument");
    const bool counts_apart = (channels & TL3D_CH_FREE) != 0;      // the free-space counts travel on their own (tl3d.h)
    const bool sub = (channels & TL3D_CH_SUB) != 0;                 // one byte per 4x4x4 sub-brick
    channels &= ~(TL3D_CH_FREE | TL3D_CH_SUB);
    if (channels == 0) channels = (ctx->tsdf ? TL3D_CH_TSDF : 0u) | (ctx->centroid ? TL3D_CH_CENTROID : 0u);
    REQUIRE((channels & ~(TL3D_CH_TSDF | TL3D_CH_CENTROID)) == 0, TL3D_E_INVALID, "bad channel mask 0x%x", channels);
    if (channels & TL3D_CH_TSDF) REQUIRE(ctx->tsdf != nullptr, TL3D_E_STATE, "TSDF channel not enabled");
    if (channels & TL3D_CH_CENTROID) REQUIRE(ctx->centroid != nullptr, TL3D_E_STATE, "centroid channel not enabled");
    REQUIRE(n_bricks == (int64_t)(ctx->nvox >> 9) * (sub ? 8 : 1), TL3D_E_INVALID, "the grid has %zu %sbricks, the map %lld", (ctx->nvox >> 9) * (sub ? 8 : 1), sub ? "sub-" : "",
            (long long)n_bricks);
    REQUIRE(is_device_ptr(map_dev), TL3D_E_INVALID, "the brick map must be device memory");
    if (counts_apart) FLUSH_UPDATES(ctx);
    else FLUSH_AND_FOLD(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    return launch_touched_bricks(ctx->stream, ctx->grid, (channels & TL3D_CH_TSDF) ? ctx->tsdf : nullptr, (channels & TL3D_CH_CENTROID) ? ctx->centroid : nullptr,
                                 (unsigned)(ctx->nvox >> 9), map_dev, sub);
}

static int brick_rows(tl3d_ctx *ctx, uint32_t channel, const uint32_t *bricks_dev, int64_t n, void *packed_dev, bool pack) {
    void *p;
    size_t nb;
    const bool counts_apart = (channel & TL3D_CH_FREE) != 0;       // records only: pending free-space counts stay pending
    const bool sub = (channel & TL3D_CH_SUB) != 0;                  // rows are 4x4x4 sub-bricks, ids = brick * 8 + sub-brick
    channel &= ~(TL3D_CH_FREE | TL3D_CH_SUB);
    int rc = grid_sel(ctx, channel, &p, &nb);
    if (rc) return rc;
    REQUIRE(n >= 0 && n <= (int64_t)(ctx->nvox >> 9) * (sub ? 8 : 1), TL3D_E_INVALID, "brick count %lld out of range", (long long)n);
    if (n == 0) return TL3D_OK;
    REQUIRE(bricks_dev && packed_dev && is_device_ptr(bricks_dev) && is_device_ptr(packed_dev), TL3D_E_INVALID, "brick list and block must be device memory");
    if (counts_apart) FLUSH_UPDATES(ctx);
    else FLUSH_AND_FOLD(ctx);
    ctx->grid_epoch++;
    TL3D_HIP(hipSetDevice(ctx->device));
    if (!pack && channel == TL3D_CH_TSDF) {
        ctx->tsdf_w_unknown = true;                                         // the records now hold what the caller summed
        if (ctx->sparse && ctx->free_cnt) ctx->free_dirty = true;           // a brick that kept its count for want of records may get records now
    }
    return launch_brick_rows(ctx->stream, ctx->grid, pack ? 0 : 1, channel == TL3D_CH_TSDF, p, bricks_dev, n, packed_dev, false, sub);
}

int tl3d_grid_pack_bricks(tl3d_ctx *ctx, uint32_t channel, const uint32_t *bricks_dev, int64_t n, void *packed_dev) {
    return brick_rows(ctx, channel, bricks_dev, n, packed_dev, true);
}

int tl3d_grid_unpack_bricks(tl3d_ctx *ctx, uint32_t channel, const uint32_t *bricks_dev, int64_t n, const void *packed_dev) {
    return brick_rows(ctx, channel, bricks_dev, n, const_cast<void *>(packed_dev), false);
}

int tl3d_grid_max_weight(tl3d_ctx *ctx, int64_t *out) {
    REQUIRE(ctx && out, TL3D_E_INVALID, "null argument");
    REQUIRE(ctx->tsdf != nullptr, TL3D_E_STATE, "TSDF channel not enabled");
    FLUSH_UPDATES(ctx);                                 // (pending free-space counts are added per brick by the kernel: no fold needed)
    TL3D_HIP(hipSetDevice(ctx->device));
    long long w = 0;
    const int rc = measure_max_weight(ctx, ctx->tsdf, &w);
    if (rc) return rc;
    ctx->tsdf_w_upper = w;
    ctx->tsdf_w_unknown = false;
    *out = (int64_t)w;
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- RCCL merge (no torch)
int tl3d_rccl_unique_id(uint8_t id_out[TL3D_RCCL_ID_BYTES]) {
    REQUIRE(id_out != nullptr, TL3D_E_INVALID, "null out pointer");
    int rc = rccl_load();
    if (rc) return rc;
    RcclId id;
    memset(&id, 0, sizeof(id));
    const int nrc = g_rccl.GetUniqueId(&id);
    REQUIRE(nrc == 0, TL3D_E_HIP, "ncclGetUniqueId failed: %s", rccl_msg(nrc));
    memcpy(id_out, id.bytes, TL3D_RCCL_ID_BYTES);
    return TL3D_OK;
}

int tl3d_rccl_init(tl3d_ctx *ctx, int world, int rank, const uint8_t id_in[TL3D_RCCL_ID_BYTES]) {
    REQUIRE(ctx && id_in, TL3D_E_INVALID, "null argument");
    REQUIRE(world >= 1 && rank >= 0 && rank < world, TL3D_E_INVALID, "bad rank %d of %d", rank, world);
    REQUIRE(ctx->rccl_comm == nullptr, TL3D_E_STATE, "context already joined a communicator");
    int rc = rccl_load();
    if (rc) return rc;
    TL3D_HIP(hipSetDevice(ctx->device));
    RcclId id;
    memcpy(id.bytes, id_in, TL3D_RCCL_ID_BYTES);
    // ncclResult_t ncclCommInitRank(ncclComm_t*, int nranks, ncclUniqueId commId /* 128-byte struct BY VALUE */, int rank)
    typedef int (*init_fn)(void **, int, RcclId, int);
    void *comm = nullptr;
    const int nrc = ((init_fn)(void *)g_rccl.CommInitRank)(&comm, world, id, rank);
    REQUIRE(nrc == 0 && comm, TL3D_E_HIP, "ncclCommInitRank failed: %s", rccl_msg(nrc));
    ctx->rccl_comm = comm;
    ctx->rccl_world = world;
    return TL3D_OK;
}

// A rank that fails BETWEEN the collectives of a merge must not simply return: its peers would sit in the next all-reduce for ever.
// The communicator is aborted (the peers' pending and later collectives on it end with an error) and the context forgets it.
static int rccl_abandon(tl3d_ctx *ctx, int code) {
    if (ctx->rccl_comm) {
        if (g_rccl.CommAbort) (void)g_rccl.CommAbort(ctx->rccl_comm);
        else if (g_rccl.CommDestroy) (void)g_rccl.CommDestroy(ctx->rccl_comm);
        ctx->rccl_comm = nullptr;
    }
    return code;
}
#define REQUIRE_OR_ABANDON(cond_, code_, ...) \
    do {                                       \
        if (!(cond_)) return rccl_abandon(ctx, set_err(code_, __VA_ARGS__)); \
    } while (0)

int tl3d_allreduce_grid(tl3d_ctx *ctx, uint32_t channels) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(ctx->rccl_comm != nullptr, TL3D_E_STATE, "call tl3d_rccl_init first");
    if (channels == 0) channels = (ctx->tsdf ? TL3D_CH_TSDF : 0u) | (ctx->centroid ? TL3D_CH_CENTROID : 0u);
    REQUIRE((channels & ~(TL3D_CH_TSDF | TL3D_CH_CENTROID)) == 0, TL3D_E_INVALID, "bad channel mask 0x%x", channels);
    if (channels & TL3D_CH_TSDF) REQUIRE(ctx->tsdf != nullptr, TL3D_E_STATE, "TSDF channel not enabled");
    if (channels & TL3D_CH_CENTROID) REQUIRE(ctx->centroid != nullptr, TL3D_E_STATE, "centroid channel not enabled");
    FLUSH_AND_FOLD(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    ctx->grid_epoch++;
    if (channels & TL3D_CH_TSDF) {
        // int32 headroom over all ranks: the sum of the ranks' largest voxel weights bounds the merged grid's
        long long w = 0;
        int rc = measure_max_weight(ctx, ctx->tsdf, &w);
        if (rc) return rccl_abandon(ctx, rc);
        Staging st(ctx);
        long long *d_w;
        rc = st.scratch(sizeof(long long), &d_w);
        if (rc) return rccl_abandon(ctx, rc);
        hipError_t e = hipMemcpyAsync(d_w, &w, sizeof(w), hipMemcpyHostToDevice, ctx->stream);
        int nrc = e == hipSuccess ? g_rccl.AllReduce(d_w, d_w, 1, 4 /* ncclInt64 */, 0 /* ncclSum */, ctx->rccl_comm, ctx->stream) : -1;
        long long total = 0;
        if (nrc == 0) e = hipMemcpyAsync(&total, d_w, sizeof(total), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        REQUIRE_OR_ABANDON(nrc == 0 && e == hipSuccess, TL3D_E_HIP, "weight all-reduce failed: %s", nrc ? rccl_msg(nrc) : hipGetErrorString(e));
        REQUIRE_OR_ABANDON(total <= TL3D_TSDF_MAX_WEIGHT, TL3D_E_STATE,
                "the merged TSDF grid could hold %lld observations per voxel (limit %d): merge more often or extract between scans", total,
                TL3D_TSDF_MAX_WEIGHT);
        ctx->tsdf_w_upper = total;
        ctx->tsdf_w_unknown = false;
    }
    // Which bricks does ANY rank hold something in?  One byte per brick, MAX all-reduce: every rank gets the same set.  When it
    // is less than half of the grid only those bricks' records travel (packed, summed, unpacked); a frame-sharded run of a
    // few dozen frames per rank touches a few per cent of a 1024^3 grid.
    const size_t nbr = ctx->nvox >> 9;
    std::vector<unsigned char> h_map(nbr);
    std::vector<unsigned> h_idx;
    int rc = TL3D_OK;
    {
        Staging st(ctx);
        unsigned char *d_map;
        rc = st.scratch(nbr, &d_map);
        if (rc) return rccl_abandon(ctx, rc);
        hipError_t e = hipMemsetAsync(d_map, 0, nbr, ctx->stream);
        if (e == hipSuccess)
            rc = launch_touched_bricks(ctx->stream, ctx->grid, (channels & TL3D_CH_TSDF) ? ctx->tsdf : nullptr, (channels & TL3D_CH_CENTROID) ? ctx->centroid : nullptr,
                                       (unsigned)nbr, d_map);
        int nrc = (e == hipSuccess && rc == TL3D_OK) ? g_rccl.AllReduce(d_map, d_map, nbr, 1 /* ncclUint8 */, 2 /* ncclMax */, ctx->rccl_comm, ctx->stream) : -1;
        if (nrc == 0) e = hipMemcpyAsync(h_map.data(), d_map, nbr, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        REQUIRE_OR_ABANDON(rc == TL3D_OK && nrc == 0 && e == hipSuccess, TL3D_E_HIP, "brick-map all-reduce failed: %s", nrc > 0 ? rccl_msg(nrc) : hipGetErrorString(e));
    }
    for (size_t b = 0; b < nbr; ++b)
        if (h_map[b]) h_idx.push_back((unsigned)b);
    const bool sparse = ctx->sparse || h_idx.size() * 2 < nbr;
    if (ctx->sparse && (channels & TL3D_CH_TSDF) && ctx->free_cnt) {
        // bricks without records carry their free-space observations as a count: summed like the records (4 B per brick)
        const int nrc = g_rccl.AllReduce(ctx->free_cnt, ctx->free_cnt, nbr, 3 /* ncclUint32 */, 0, ctx->rccl_comm, ctx->stream);
        REQUIRE_OR_ABANDON(nrc == 0, TL3D_E_HIP, "ncclAllReduce (free-space counts) failed: %s", rccl_msg(nrc));
    }
    ctx->stats.merge_bricks_sent += sparse ? h_idx.size() : nbr;
    ctx->stats.merge_bricks_total += nbr;
    if (!sparse) {
        if (channels & TL3D_CH_TSDF) {
            const int nrc = g_rccl.AllReduce(ctx->tsdf, ctx->tsdf, ctx->nvox * 2, 2 /* ncclInt32 */, 0, ctx->rccl_comm, ctx->stream);
            REQUIRE_OR_ABANDON(nrc == 0, TL3D_E_HIP, "ncclAllReduce (TSDF) failed: %s", rccl_msg(nrc));
        }
        if (channels & TL3D_CH_CENTROID) {
            const int nrc = g_rccl.AllReduce(ctx->centroid, ctx->centroid, ctx->nvox * 4, 5 /* ncclUint64 */, 0, ctx->rccl_comm, ctx->stream);
            REQUIRE_OR_ABANDON(nrc == 0, TL3D_E_HIP, "ncclAllReduce (centroid) failed: %s", rccl_msg(nrc));
        }
        REQUIRE_OR_ABANDON(hipStreamSynchronize(ctx->stream) == hipSuccess, TL3D_E_HIP, "sync failed");
        return TL3D_OK;
    }
    if (h_idx.empty()) {                                 // (the free-space counts' all-reduce may still be in flight)
        REQUIRE_OR_ABANDON(hipStreamSynchronize(ctx->stream) == hipSuccess, TL3D_E_HIP, "sync failed");
        return TL3D_OK;
    }
    Staging st(ctx);
    const unsigned *d_idx;
    void *d_pack;
    const size_t n = h_idx.size();
    const size_t row = (channels & TL3D_CH_CENTROID) ? 16384 : 4096;
    rc = st.in(h_idx.data(), n * sizeof(unsigned), &d_idx);
    if (!rc) rc = st.scratch(n * row, &d_pack);
    if (rc) return rccl_abandon(ctx, rc);
    int nrc = 0;
    if (channels & TL3D_CH_TSDF) {
        rc = launch_brick_rows(ctx->stream, ctx->grid, 0, true, ctx->tsdf, d_idx, (long long)n, d_pack, false);
        if (rc == TL3D_OK) nrc = g_rccl.AllReduce(d_pack, d_pack, n * 1024, 2 /* ncclInt32 */, 0, ctx->rccl_comm, ctx->stream);
        if (rc == TL3D_OK && nrc == 0) rc = launch_brick_rows(ctx->stream, ctx->grid, 1, true, ctx->tsdf, d_idx, (long long)n, d_pack, false);
    }
    if (rc == TL3D_OK && nrc == 0 && (channels & TL3D_CH_CENTROID)) {
        rc = launch_brick_rows(ctx->stream, ctx->grid, 0, false, ctx->centroid, d_idx, (long long)n, d_pack, false);
        if (rc == TL3D_OK) nrc = g_rccl.AllReduce(d_pack, d_pack, n * 2048, 5 /* ncclUint64 */, 0, ctx->rccl_comm, ctx->stream);
        if (rc == TL3D_OK && nrc == 0) rc = launch_brick_rows(ctx->stream, ctx->grid, 1, false, ctx->centroid, d_idx, (long long)n, d_pack, false);
    }
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    REQUIRE_OR_ABANDON(rc == TL3D_OK && nrc == 0 && e == hipSuccess, TL3D_E_HIP, "sparse grid all-reduce failed: %s", nrc ? rccl_msg(nrc) : hipGetErrorString(e));
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- extraction
int tl3d_extract(tl3d_ctx *ctx, int mode, int min_count, int min_weight, double max_abs_tsdf, float *out_xyz,
                 uint8_t *out_rgb, int64_t cap, int64_t *out_n) {
    REQUIRE(ctx && out_n, TL3D_E_INVALID, "null argument");
    REQUIRE(mode == TL3D_EXTRACT_CENTROID || mode == TL3D_EXTRACT_TSDF, TL3D_E_INVALID, "bad mode %d", mode);
    if (mode == TL3D_EXTRACT_CENTROID) REQUIRE(ctx->centroid != nullptr, TL3D_E_STATE, "centroid channel not enabled");
    if (mode == TL3D_EXTRACT_TSDF) REQUIRE(ctx->tsdf != nullptr, TL3D_E_STATE, "TSDF channel not enabled");
    FLUSH_AND_FOLD(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    const int nblocks = chunks_of(ctx->nvox);
    int rc = grow_pair(&ctx->block_counts, &ctx->block_offsets, &ctx->scratch_blocks, (size_t)nblocks + 1, "extraction scratch");
    if (rc) return rc;
    const ChunkHalves ch(ctx->block_counts, ctx->block_offsets, nblocks);
    unsigned long long total = 0;
    const bool reuse = ctx->ext_valid && ctx->ext_epoch == ctx->grid_epoch && ctx->ext_mode == mode && ctx->ext_min_count == min_count &&
                       ctx->ext_min_weight == min_weight && ctx->ext_max_abs == max_abs_tsdf;
    if (reuse) {                                        // the size query just before this call already counted and scanned
        total = ctx->ext_total;
    } else {
        ctx->ext_valid = false;
        rc = launch_extract_count(ctx->stream, ctx->grid, mode, min_count, min_weight, max_abs_tsdf, ctx->tsdf, ctx->centroid, ctx->block_counts, nblocks);
        if (rc) return rc;
        rc = ch.scan(ctx->stream, 0);
        if (!rc) rc = ch.totals(ctx->stream, &total);
        if (rc) return rc;
        ctx->ext_valid = true; ctx->ext_epoch = ctx->grid_epoch; ctx->ext_total = total;
        ctx->ext_mode = mode; ctx->ext_min_count = min_count; ctx->ext_min_weight = min_weight; ctx->ext_max_abs = max_abs_tsdf;
    }
    *out_n = (int64_t)total;
    if (!out_xyz || !out_rgb) return TL3D_OK;
    if ((int64_t)total > cap) return set_err(TL3D_E_CAPACITY, "need %llu points, capacity %lld", total, (long long)cap);
    if (total == 0) return TL3D_OK;
    Staging st(ctx);
    float *dxyz;
    uint8_t *drgb;
    rc = st.out(out_xyz, total * 12, &dxyz);
    if (!rc) rc = st.out(out_rgb, total * 3, &drgb);
    if (rc) return rc;
    rc = launch_extract_write(ctx->stream, ctx->grid, mode, min_count, min_weight, max_abs_tsdf, ctx->tsdf, ctx->centroid,
                              ctx->block_offsets, nblocks, dxyz, drgb, total);
    return st.finish(rc, true);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------- mesh

static int extract_mesh_impl(tl3d_ctx *ctx, int min_weight, float *out_xyz, uint8_t *out_rgb, int64_t vert_cap, uint32_t *out_tri,
                             int64_t tri_cap, int64_t *out_n_vert, int64_t *out_n_tri, int64_t *out_key) {
    REQUIRE(ctx && out_n_vert && out_n_tri, TL3D_E_INVALID, "null argument");
    REQUIRE(ctx->tsdf != nullptr, TL3D_E_STATE, "TSDF channel not enabled");
    FLUSH_AND_FOLD(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    const int nblocks = chunks_of(ctx->nvox);
    int rc = grow_pair(&ctx->mesh_counts, &ctx->mesh_offsets, &ctx->mesh_blocks, 2 * ((size_t)nblocks + 1), "mesh scratch");
    if (!rc) rc = grow(&ctx->mesh_first, &ctx->mesh_first_n, (size_t)ctx->grid.tsdf_cap << 9, "mesh vertex-id scratch");
    if (rc) return rc;
    const ChunkHalves ch(ctx->mesh_counts, ctx->mesh_offsets, nblocks, nblocks);
    unsigned long long nv = 0, nt = 0;
    if (ctx->mesh_valid && ctx->mesh_epoch == ctx->grid_epoch && ctx->mesh_min_weight == min_weight) {
        nv = ctx->mesh_nv;                              // the size query just before this call already counted and scanned
        nt = ctx->mesh_nt;
    } else {
        ctx->mesh_valid = false;
        rc = launch_mesh_count(ctx->stream, ctx->grid, min_weight, ctx->tsdf, ch.counts[0], ch.counts[1], nblocks);
        if (!rc) rc = ch.scan(ctx->stream, 0);
        if (!rc) rc = ch.scan(ctx->stream, 1);
        unsigned long long h[2] = {0, 0};
        if (!rc) rc = ch.totals(ctx->stream, h);
        if (rc) return rc;
        nv = h[0];
        nt = h[1];
        ctx->mesh_valid = true; ctx->mesh_epoch = ctx->grid_epoch; ctx->mesh_min_weight = min_weight;
        ctx->mesh_nv = nv; ctx->mesh_nt = nt;
    }
    *out_n_vert = (int64_t)nv;
    *out_n_tri = (int64_t)nt;
    // uint32 indices, and PLY's int vertex_indices: fewer than 2^31 vertices
    if (nv >= (1ull << 31)) return set_err(TL3D_E_CAPACITY, "mesh has %llu vertices: indices need fewer than 2^31", nv);
    if (!out_xyz || !out_rgb || !out_tri) return TL3D_OK;
    if ((int64_t)nv > vert_cap || (int64_t)nt > tri_cap)
        return set_err(TL3D_E_CAPACITY, "need %llu vertices / %llu triangles, capacities %lld / %lld", nv, nt, (long long)vert_cap,
                       (long long)tri_cap);
    if (nv == 0) return TL3D_OK;                        // (no vertex: no meshed cell either)
    Staging st(ctx);
    float *dxyz;
    uint8_t *drgb;
    uint32_t *dtri;
    int64_t *dkey = nullptr;
    rc = st.out(out_xyz, nv * 12, &dxyz);
    if (!rc) rc = st.out(out_rgb, nv * 3, &drgb);
    if (!rc) rc = st.out(out_tri, nt * 12, &dtri);              // (no triangle: nothing staged, nothing written)
    if (!rc && out_key) rc = st.out(out_key, nv * 8, &dkey);
    if (rc) return rc;
    rc = launch_mesh_write(ctx->stream, ctx->grid, min_weight, ctx->tsdf, ctx->centroid, ch.offs[0], ch.offs[1], nblocks, ctx->mesh_first,
                           dxyz, drgb, nv, dtri, nt, (long long *)dkey, ctx->lat);
    return st.finish(rc, true);
}

extern "C" {

int tl3d_extract_mesh(tl3d_ctx *ctx, int min_weight, float *out_xyz, uint8_t *out_rgb, int64_t vert_cap, uint32_t *out_tri,
                      int64_t tri_cap, int64_t *out_n_vert, int64_t *out_n_tri) {
    return extract_mesh_impl(ctx, min_weight, out_xyz, out_rgb, vert_cap, out_tri, tri_cap, out_n_vert, out_n_tri, nullptr);
}

int tl3d_extract_mesh_keyed(tl3d_ctx *ctx, int min_weight, float *out_xyz, uint8_t *out_rgb, int64_t vert_cap, uint32_t *out_tri,
                            int64_t tri_cap, int64_t *out_key, int64_t *out_n_vert, int64_t *out_n_tri) {
    REQUIRE(ctx && (out_key || !out_xyz), TL3D_E_INVALID, "null key buffer");
    return extract_mesh_impl(ctx, min_weight, out_xyz, out_rgb, vert_cap, out_tri, tri_cap, out_n_vert, out_n_tri, out_key);
}

// ------------------------------------------------------------------------------------------- ray casting
// a device buffer for each output the caller wants on the host (allocated on first use; the camera never changes)
static int ray_target(void *out, void **staging, size_t bytes, void **dev) {
    *dev = nullptr;
    if (!out) return TL3D_OK;
    if (is_device_ptr(out)) {
        *dev = out;
        return TL3D_OK;
    }
    if (!*staging && hipMalloc(staging, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *staging = nullptr;
        return set_err(TL3D_E_NOMEM, "ray-cast staging alloc (%zu B) failed", bytes);
    }
    *dev = *staging;
    return TL3D_OK;
}

int tl3d_raycast(tl3d_ctx *ctx, const double R[9], const double t[3], int min_weight, double z_near, double z_far, int slot,
                 float *depth_out, float *normal_out, uint8_t *bgr_out) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(R && t, TL3D_E_INVALID, "null pose");
    REQUIRE(ctx->tsdf != nullptr, TL3D_E_STATE, "ray casting needs a grid with a TSDF channel");
    REQUIRE(!ctx->has_core && ctx->cfg.voxel_offset[0] == 0 && ctx->cfg.voxel_offset[1] == 0 && ctx->cfg.voxel_offset[2] == 0, TL3D_E_STATE,
            "ray casting needs a whole lattice: this grid is a block (voxel offset or core set)");
    if (slot >= 0) {
        const int src = check_slot(ctx, slot, false);
        if (src) return src;
    }
    FLUSH_AND_FOLD(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    const size_t npx = (size_t)ctx->cam.W * ctx->cam.H;
    void *dd = nullptr, *dn = nullptr, *dc = nullptr;
    int rc = ray_target(depth_out, (void **)&ctx->ray_depth, npx * sizeof(float), &dd);
    if (!rc) rc = ray_target(normal_out, (void **)&ctx->ray_nrm, npx * 3 * sizeof(float), &dn);
    if (!rc) rc = ray_target(bgr_out, (void **)&ctx->ray_bgr, npx * 3, &dc);
    if (rc) return rc;
    float *sd = nullptr;
    uint8_t *sc = nullptr;
    if (slot >= 0) {
        Slot &s = ctx->slots[slot];
        rc = order_after_lanes(ctx, slot, true, true);  // an uncollected ICP run may still read this slot
        if (rc) return rc;
        if (!s.depth && !(s.depth = (float *)pool_take(ctx->pool_depth))) return set_err(TL3D_E_NOMEM, "frame alloc failed");
        sd = s.depth;
        sc = s.bgr;                                      // colour only into a slot that has a colour buffer
    }
    const float zn = (float)(z_near > 0.0 ? z_near : ctx->cfg.min_depth);
    const float zf = (float)(z_far > 0.0 ? z_far : ctx->cfg.max_depth);
    rc = launch_raycast(ctx->stream, ctx->cam, ctx->grid, R, t, min_weight, zn, zf, ctx->tsdf, ctx->centroid, (float *)dd, sd,
                        (float *)dn, (uint8_t *)dc, sc);
    if (rc) return rc;
    if (slot >= 0) {                                     // the slot now holds an f32 frame, as after an upload
        rc = slot_rewritten(ctx, ctx->slots[slot], false, sc != nullptr);
        if (rc) return rc;
    }
    if (depth_out && dd != depth_out) TL3D_HIP(hipMemcpyAsync(depth_out, dd, npx * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (normal_out && dn != normal_out) TL3D_HIP(hipMemcpyAsync(normal_out, dn, npx * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (bgr_out && dc != bgr_out) TL3D_HIP(hipMemcpyAsync(bgr_out, dc, npx * 3, hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- outlier filter
int tl3d_statistical_outlier(tl3d_ctx *ctx, const float *xyz, int64_t n, int nb_neighbors, double std_ratio,
                             double cell_size, uint8_t *keep_out, int64_t *out_kept) {
    REQUIRE(ctx && keep_out && out_kept, TL3D_E_INVALID, "null argument");
    REQUIRE(n >= 0 && (n == 0 || xyz), TL3D_E_INVALID, "bad point list");
    REQUIRE(nb_neighbors >= 1 && nb_neighbors <= 64, TL3D_E_INVALID, "nb_neighbors must be in [1,64]");
    REQUIRE(cell_size > 0, TL3D_E_INVALID, "cell_size must be positive");
    *out_kept = 0;
    if (n == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *dx;
    uint8_t *dk;
    int rc = st.in(xyz, (size_t)n * 12, &dx);
    if (!rc) rc = st.out(keep_out, (size_t)n, &dk);
    if (rc) return rc;
    long long kept = 0;
    rc = st.finish(sor_run(ctx, dx, n, nb_neighbors, std_ratio, cell_size, dk, &kept), true);
    if (rc) return rc;
    *out_kept = kept;
    return TL3D_OK;
}

int tl3d_knn_mean_distance(tl3d_ctx *ctx, const float *xyz, int64_t n, int nb_neighbors, double cell_size, double *mean_out) {
    REQUIRE(ctx && mean_out, TL3D_E_INVALID, "null argument");
    REQUIRE(n >= 0 && (n == 0 || xyz), TL3D_E_INVALID, "bad point list");
    REQUIRE(nb_neighbors >= 1 && nb_neighbors <= 64, TL3D_E_INVALID, "nb_neighbors must be in [1,64]");
    REQUIRE(cell_size > 0, TL3D_E_INVALID, "cell_size must be positive");
    if (n == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *dx;
    double *dm;
    int rc = st.in(xyz, (size_t)n * 12, &dx);
    if (!rc) rc = st.out(mean_out, (size_t)n * sizeof(double), &dm);
    if (rc) return rc;
    return st.finish(sor_mean_distance(ctx, dx, n, nb_neighbors, cell_size, &dm), true);
}

// ------------------------------------------------------------------------------------------- cloud normals
int tl3d_estimate_normals(tl3d_ctx *ctx, const float *xyz, int64_t n, int nb_neighbors, double max_radius, double cell_size,
                          const double *viewpoints, int64_t n_viewpoints, float *normal_out, float *curvature_out, int64_t *out_degenerate) {
    REQUIRE(ctx && xyz && normal_out, TL3D_E_INVALID, "null argument");
    REQUIRE(n >= 0 && n < (1ll << 31), TL3D_E_INVALID, "n %lld: indices need 0 <= n < 2^31", (long long)n);
    REQUIRE(nb_neighbors >= 3 && nb_neighbors <= 64, TL3D_E_INVALID, "nb_neighbors must be in [3,64]");
    REQUIRE(cell_size > 0, TL3D_E_INVALID, "cell_size must be positive");
    REQUIRE(n_viewpoints >= 0 && n_viewpoints < (1ll << 31) && (n_viewpoints == 0 || viewpoints), TL3D_E_INVALID, "bad viewpoint list");
    for (int64_t i = 0; i < 3 * n_viewpoints; ++i) REQUIRE(isfinite(viewpoints[i]), TL3D_E_INVALID, "viewpoint %lld is not finite", (long long)(i / 3));
    const size_t nb_x = (size_t)n * 12, nb_c = (size_t)n * 4;
    REQUIRE(!ranges_overlap(normal_out, nb_x, xyz, nb_x) && !ranges_overlap(curvature_out, nb_c, xyz, nb_x), TL3D_E_INVALID, "an output aliases the input");
    REQUIRE(!ranges_overlap(normal_out, nb_x, curvature_out, nb_c), TL3D_E_INVALID, "the outputs alias each other");
    if (n == 0) {
        if (out_degenerate) *out_degenerate = 0;
        return TL3D_OK;
    }
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *dx;
    float *dn, *dc = nullptr;
    int rc = st.in(xyz, nb_x, &dx);
    if (!rc) rc = st.out(normal_out, nb_x, &dn);
    if (!rc && curvature_out) rc = st.out(curvature_out, nb_c, &dc);
    if (rc) return rc;
    long long deg = 0;
    rc = st.finish(normals_run(ctx, dx, n, nb_neighbors, max_radius, cell_size, viewpoints, n_viewpoints, dn, dc, &deg), true);
    if (rc) return rc;
    if (out_degenerate) *out_degenerate = deg;
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- planar regions of a cloud
int tl3d_segment_planes(tl3d_ctx *ctx, const float *xyz, const float *normal, const float *curvature, int64_t n, const tl3d_plane_params *params,
                        double cell_size, int32_t *plane_id_out, tl3d_plane *planes_out, int64_t plane_cap, int64_t *out_counts) {
    REQUIRE(ctx && xyz && normal && params && plane_id_out && out_counts, TL3D_E_INVALID, "null argument");
    REQUIRE(n >= 0 && n < (1ll << 31), TL3D_E_INVALID, "n %lld: indices need 0 <= n < 2^31", (long long)n);
    REQUIRE(plane_cap >= 0 && (plane_cap == 0 || planes_out), TL3D_E_INVALID, "bad plane capacity");
    REQUIRE(isfinite(params->radius) && params->radius > 0, TL3D_E_INVALID, "radius must be finite and positive");
    REQUIRE(params->min_cos >= 0 && params->min_cos <= 1, TL3D_E_INVALID, "min_cos must be in [0,1]");
    REQUIRE(params->max_offset >= 0, TL3D_E_INVALID, "max_offset must not be negative");
    REQUIRE(params->min_points >= 3, TL3D_E_INVALID, "min_points must be at least 3");
    REQUIRE(params->reserved == 0, TL3D_E_INVALID, "reserved must be 0");
    REQUIRE(cell_size > 0, TL3D_E_INVALID, "cell_size must be positive");
    const size_t nb_x = (size_t)n * 12, nb_c = (size_t)n * 4, nb_p = (size_t)plane_cap * sizeof(tl3d_plane);
    const void *ins[3] = {xyz, normal, curvature};
    const size_t in_b[3] = {nb_x, nb_x, nb_c};
    for (int i = 0; i < 3; ++i)
        REQUIRE(!ranges_overlap(plane_id_out, nb_c, ins[i], in_b[i]) && !ranges_overlap(planes_out, nb_p, ins[i], in_b[i]), TL3D_E_INVALID,
                "an output aliases an input");
    REQUIRE(!ranges_overlap(plane_id_out, nb_c, planes_out, nb_p), TL3D_E_INVALID, "the outputs alias each other");
    if (n == 0) {
        out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
        return TL3D_OK;
    }
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *dx, *dn, *dc = nullptr;
    int32_t *did;
    int rc = st.in(xyz, nb_x, &dx);
    if (!rc) rc = st.in(normal, nb_x, &dn);
    if (!rc && curvature) rc = st.in(curvature, nb_c, &dc);
    if (!rc) rc = st.out(plane_id_out, nb_c, &did);
    if (rc) return rc;
    long long counts[4] = {0, 0, 0, 0};
    bool short_cap = false;
    rc = st.finish(planes_run(ctx, dx, dn, dc, n, *params, cell_size, did, planes_out, plane_cap, counts, &short_cap), true);
    if (rc) return rc;
    for (int i = 0; i < 4; ++i) out_counts[i] = counts[i];
    if (short_cap) return set_err(TL3D_E_CAPACITY, "need %lld planes, capacity %lld", counts[3], (long long)plane_cap);
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- nearest neighbours, distance summary
// what both searches check before any device work
static int nn_check(tl3d_ctx *ctx, const float *query, int64_t n_query, const void *const *ins, const size_t *in_bytes, int n_ins,
                    double *dist_out, int32_t *index_out) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(n_query >= 0 && (n_query == 0 || query), TL3D_E_INVALID, "bad query list");
    const void *outs[2] = {dist_out, index_out};
    const size_t out_b[2] = {(size_t)n_query * sizeof(double), (size_t)n_query * sizeof(int32_t)};
    for (int o = 0; o < 2; ++o) {
        REQUIRE(!ranges_overlap(outs[o], out_b[o], query, (size_t)n_query * 12), TL3D_E_INVALID, "an output aliases an input");
        for (int i = 0; i < n_ins; ++i)
            REQUIRE(!ranges_overlap(outs[o], out_b[o], ins[i], in_bytes[i]), TL3D_E_INVALID, "an output aliases an input");
    }
    REQUIRE(!ranges_overlap(dist_out, out_b[0], index_out, out_b[1]), TL3D_E_INVALID, "the outputs alias each other");
    return TL3D_OK;
}

int tl3d_nearest_points(tl3d_ctx *ctx, const float *query, int64_t n_query, const float *target, int64_t n_target, double cell_size,
                        double max_dist, double *dist_out, int32_t *index_out) {
    REQUIRE(n_target >= 0 && (n_target == 0 || target), TL3D_E_INVALID, "bad target list");
    REQUIRE(n_target < (1ll << 31), TL3D_E_INVALID, "n_target %lld: indices need fewer than 2^31 points", (long long)n_target);
    const void *ins[1] = {target};
    const size_t in_b[1] = {(size_t)n_target * 12};
    int rc = nn_check(ctx, query, n_query, ins, in_b, 1, dist_out, index_out);
    if (rc) return rc;
    if (n_query == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *dq, *dt = nullptr;
    double *dd = nullptr;
    int32_t *di = nullptr;
    rc = st.in(query, (size_t)n_query * 12, &dq);
    if (!rc && n_target) rc = st.in(target, (size_t)n_target * 12, &dt);
    if (!rc && dist_out) rc = st.out(dist_out, (size_t)n_query * sizeof(double), &dd);
    if (!rc && index_out) rc = st.out(index_out, (size_t)n_query * sizeof(int32_t), &di);
    if (rc) return rc;
    return st.finish(nearest_points_run(ctx, dq, n_query, dt, n_target, cell_size, max_dist, dd, di), true);
}

int tl3d_nearest_triangles(tl3d_ctx *ctx, const float *query, int64_t n_query, const float *xyz, int64_t n_vert, const uint32_t *tri,
                           int64_t n_tri, double cell_size, double max_dist, double *dist_out, int32_t *tri_out) {
    REQUIRE(n_tri >= 0 && n_vert >= 0, TL3D_E_INVALID, "negative size (n_tri %lld, n_vert %lld)", (long long)n_tri, (long long)n_vert);
    REQUIRE(n_vert < (1ll << 31) && n_tri < (1ll << 31), TL3D_E_INVALID, "n_vert %lld, n_tri %lld: indices need fewer than 2^31 of each",
            (long long)n_vert, (long long)n_tri);
    REQUIRE((n_tri == 0 || tri) && (n_vert == 0 || xyz), TL3D_E_INVALID, "null mesh array");
    const void *ins[2] = {xyz, tri};
    const size_t in_b[2] = {(size_t)n_vert * 12, (size_t)n_tri * 12};
    int rc = nn_check(ctx, query, n_query, ins, in_b, 2, dist_out, tri_out);
    if (rc) return rc;
    if (n_query == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *dq, *dx = nullptr;
    const uint32_t *dt = nullptr;
    double *dd = nullptr;
    int32_t *di = nullptr;
    rc = st.in(query, (size_t)n_query * 12, &dq);
    if (!rc && n_vert) rc = st.in(xyz, (size_t)n_vert * 12, &dx);
    if (!rc && n_tri) rc = st.in(tri, (size_t)n_tri * 12, &dt);
    if (!rc && dist_out) rc = st.out(dist_out, (size_t)n_query * sizeof(double), &dd);
    if (!rc && tri_out) rc = st.out(tri_out, (size_t)n_query * sizeof(int32_t), &di);
    if (rc) return rc;
    return st.finish(nearest_triangles_run(ctx, dq, n_query, dx, n_vert, dt, n_tri, cell_size, max_dist, dd, di), true);
}

int tl3d_distance_summary(tl3d_ctx *ctx, const double *dist, int64_t n, const double *thresholds, int n_thresholds, tl3d_distance_stats *out) {
    REQUIRE(ctx && out, TL3D_E_INVALID, "null argument");
    REQUIRE(n >= 0 && (n == 0 || dist), TL3D_E_INVALID, "bad distance list");
    REQUIRE(n_thresholds >= 0 && n_thresholds <= 8 && (n_thresholds == 0 || thresholds), TL3D_E_INVALID, "n_thresholds %d outside [0, 8]", n_thresholds);
    memset(out, 0, sizeof(*out));
    out->n = n;
    if (n == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const double *dd;
    int rc = st.in(dist, (size_t)n * sizeof(double), &dd);
    if (rc) return rc;
    return st.finish(distance_summary_run(ctx, dd, n, thresholds, n_thresholds, out), true);
}

int tl3d_set_nearest_query_order(tl3d_ctx *ctx, int cell_order) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    ctx->nn_input_order = cell_order == 0;
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- measurement
int tl3d_set_profile(tl3d_ctx *ctx, int count_records, int time_kernels) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    FLUSH_UPDATES(ctx);
    ctx->count_records = count_records != 0;
    ctx->time_kernels = time_kernels != 0;
    return TL3D_OK;
}

int tl3d_set_normal_smoothing(tl3d_ctx *ctx, int radius) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(radius >= 0 && radius <= 8, TL3D_E_INVALID, "smoothing radius %d out of range [0, 8]", radius);
    ctx->normal_radius = radius;
    return TL3D_OK;
}

int tl3d_set_tsdf_pairing(tl3d_ctx *ctx, int on) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    FLUSH_UPDATES(ctx);
    ctx->tsdf_pairing = on != 0;
    return TL3D_OK;
}

int tl3d_get_stats(tl3d_ctx *ctx, tl3d_stats *out) {
    REQUIRE(ctx && out, TL3D_E_INVALID, "null argument");
    FLUSH_UPDATES(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    unsigned long long h[16];
    std::vector<unsigned long long> hc(256 * 8);
    TL3D_HIP(hipMemcpyAsync(h, ctx->d_counters, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipMemcpyAsync(hc.data(), ctx->d_cen_counters, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    h[0] = h[1] = 0;
    unsigned long long cen_updates = 0;
    for (int i = 0; i < 256; ++i) { h[0] += hc[(size_t)i * 8]; h[1] += hc[(size_t)i * 8 + 1]; cen_updates += hc[(size_t)i * 8 + 2]; }
    for (int i = 0; i < ctx->ktimers_used; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ctx->ktimers[i].a, ctx->ktimers[i].b) == hipSuccess) {
            ctx->stats.tsdf_kernel_ms += ms;
            ctx->stats.tsdf_kernel_timed += (uint64_t)ctx->ktimers[i].launches;
        }
    }
    ctx->ktimers_used = 0;
    ctx->stats.centroid_points = h[0];
    ctx->stats.centroid_dropped = h[1];
    ctx->stats.centroid_record_updates = cen_updates;
    ctx->stats.tsdf_records_read = h[2];
    ctx->stats.tsdf_records_written = h[3];
    ctx->stats.tsdf_bricks_visited = h[4];
    ctx->stats.tsdf_bricks_free = h[5];
    ctx->stats.tsdf_bricks_free_counted = h[6];
    ctx->stats.tsdf_batch_bricks = h[7];
#ifdef TL3D_EXPERIMENTS
    if (h[14]) fprintf(stderr, "[tl3d exp] update kernel, per wave (s_memtime ticks): setup %.0f  pair loop %.0f  record update %.0f  lifetime %.0f;  bricks per wave %.2f, pairs per brick %.1f, steps per pair %.3f, waves %llu; longest wave %.0f x launches\n",
                       (double)h[8] / h[14], (double)h[9] / h[14], (double)h[10] / h[14], (double)h[11] / h[14], (double)h[12] / h[14],
                       h[12] ? (double)(h[13] & 0xffffffffull) / h[12] : 0.0, (h[13] & 0xffffffffull) ? (double)(h[13] >> 32) / (double)(h[13] & 0xffffffffull) : 0.0,
                       h[14], (double)h[15]);
    if (h[14]) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus < 1) cus = 256;
        tsdf_debug_print_spans(ctx->tsdf_max_blocks * 4, 8 * cus);
    }
#endif
    if (ctx->brick_tabs) {
        unsigned cur[4] = {0, 0, 0, 0};
        TL3D_HIP(hipMemcpy(cur, ctx->grid.cursors, sizeof(cur), hipMemcpyDeviceToHost));
        ctx->stats.pool_slots_tsdf = ctx->tsdf ? (cur[0] < ctx->grid.tsdf_cap ? cur[0] : ctx->grid.tsdf_cap) : 0;
        ctx->stats.pool_slots_centroid = ctx->centroid ? (cur[2] < ctx->grid.cen_cap ? cur[2] : ctx->grid.cen_cap) : 0;
        ctx->stats.pool_refused = (uint64_t)cur[1] + cur[3];
    }
    *out = ctx->stats;
    return TL3D_OK;
}

int tl3d_reset_stats(tl3d_ctx *ctx) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    FLUSH_UPDATES(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    TL3D_HIP(hipMemsetAsync(ctx->d_counters, 0, 16 * sizeof(unsigned long long), ctx->stream));
    TL3D_HIP(hipMemsetAsync(ctx->d_cen_counters, 0, 256 * 8 * sizeof(unsigned long long), ctx->stream));
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    ctx->ktimers_used = 0;
    return TL3D_OK;
}

int tl3d_event_record(tl3d_ctx *ctx, int which) {
    REQUIRE(ctx != nullptr && (which == 0 || which == 1), TL3D_E_INVALID, "bad argument");
    FLUSH_UPDATES(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    TL3D_HIP(hipEventRecord(ctx->ev[which], ctx->stream));
    return TL3D_OK;
}

int tl3d_event_elapsed_ms(tl3d_ctx *ctx, float *ms) {
    REQUIRE(ctx && ms, TL3D_E_INVALID, "null argument");
    TL3D_HIP(hipSetDevice(ctx->device));
    TL3D_HIP(hipEventSynchronize(ctx->ev[1]));
    TL3D_HIP(hipEventElapsedTime(ms, ctx->ev[0], ctx->ev[1]));
    return TL3D_OK;
}

}  // extern "C"
