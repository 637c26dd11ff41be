// api_register.hip -- the registration calls of the extern "C" surface (include/tl3d.h): normal maps, the ICP lanes, the batched ICP,
// the evaluation of pairs, tracking against the TSDF.  Host code only; what the calls share stands once, at the top.
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "api_host.h"

using namespace tl3d;

// ------------------------------------------------------------------------------------------- what the calls share
// The slots of a pair: both in range (TL3D_E_INVALID), both loaded, the target with a normal map (TL3D_E_STATE).  pair: its place
// in the caller's list, for the message (0 where the call takes one pair).
static int check_pair(tl3d_ctx *ctx, int src, int tgt, int pair) {
    const int n = ctx->cfg.n_slots;
    REQUIRE(src >= 0 && src < n && tgt >= 0 && tgt < n, TL3D_E_INVALID, "pair %d: slots (%d, %d) out of range [0,%d)", pair, src, tgt, n);
    REQUIRE(ctx->slots[src].loaded && ctx->slots[tgt].loaded, TL3D_E_STATE, "pair %d: slot %d or %d holds no frame", pair, src, tgt);
    REQUIRE(ctx->slots[tgt].has_normals, TL3D_E_STATE, "target slot %d has no normal map (call tl3d_build_normals)", tgt);
    return TL3D_OK;
}

// What the kernels read of a pair (the four fields IcpRun, IcpBatchPair and IcpEvalPair have in common): the source's depth -- the
// window-averaged one, in phase-major rows, when the slot's normals were built smoothed -- the target's normal map, the scale in f32
template <class P> static void describe_pair(P *p, const Slot &ss, const Slot &st, double scale) {
    p->depth_src = ss.smooth_radius > 0 ? ss.sdepth : ss.depth;
    p->src_pm = ss.smooth_radius > 0 ? 1 : 0;
    p->nmap_tgt = st.nmap;
    p->scale = (float)scale;
}

// A float4 map kept in phase-major rows (tl3d_internal.h: pm_index; normal maps, intensity maps) as the row-major [H][W][4] image a
// caller gets, into host or device memory; waits for the stream.
static int download_pm_map(tl3d_ctx *ctx, const float4 *map, float *out) {
    TL3D_HIP(hipSetDevice(ctx->device));
    if (is_device_ptr(out)) {
        const int rc2 = launch_nmap_rowmajor(ctx->stream, ctx->cam, map, (float4 *)out);
        if (rc2) return rc2;
        TL3D_HIP(hipStreamSynchronize(ctx->stream));
        return TL3D_OK;
    }
    const int W = ctx->cam.W, H = ctx->cam.H, w4 = pm_w4(W);
    float4 *tmp = (float4 *)malloc(pm_pixels(W, H) * sizeof(float4));
    REQUIRE(tmp != nullptr, TL3D_E_NOMEM, "host allocation failed");
    hipError_t e = hipMemcpyAsync(tmp, map, pm_pixels(W, H) * sizeof(float4), hipMemcpyDefault, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { free(tmp); TL3D_HIP(e); }
    float4 *o4 = (float4 *)out;
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) o4[(size_t)v * W + u] = tmp[pm_index(u, v, w4)];
    free(tmp);
    return TL3D_OK;
}

// The checks of a level.  Every call refuses iters outside [0,1000], stride < 1 and a max_dist that is not positive (NaN included);
// `refuse` adds what only some calls refuse: max_dist >= 1e18 (infinity included), estimate_scale.
enum : unsigned { LV_FINITE_GATE = 1, LV_NO_SCALE = 2 };
static int check_level(const tl3d_icp_params &p, unsigned refuse) {
    REQUIRE(p.iters >= 0 && p.iters <= 1000, TL3D_E_INVALID, "iters out of range");
    REQUIRE(p.stride >= 1, TL3D_E_INVALID, "stride must be >= 1");
    REQUIRE(p.max_dist > 0, TL3D_E_INVALID, "max_dist must be positive");
    REQUIRE(!(refuse & LV_FINITE_GATE) || p.max_dist < 1e18, TL3D_E_INVALID, "max_dist must be finite");
    REQUIRE(!(refuse & LV_NO_SCALE) || !p.estimate_scale, TL3D_E_INVALID, "tracking does not estimate the scale (estimate_scale must be 0)");
    return TL3D_OK;
}

// a level as the kernels take it: the gate squared in f32, the sampled extent of the stride (ceil)
static IcpLevel make_level(const Cam &cam, const tl3d_icp_params &p) {
    const int Ws = (cam.W + p.stride - 1) / p.stride, Hs = (cam.H + p.stride - 1) / p.stride;
    return IcpLevel{(float)p.max_dist * (float)p.max_dist, p.stride, Ws, Hs, p.iters, p.estimate_scale ? 1 : 0, p.damping, p.eps, p.eig_rel};
}

// the final state of a run as the caller gets it; the sums of one pass as the caller gets them
static void read_result(const IcpState &h, tl3d_icp_result *out) {
    const double e = h.sums[ICP_SUM_E], n_corr = h.sums[ICP_SUM_CORR], n_src = h.sums[ICP_SUM_SRC];
    memcpy(out->T, h.T, sizeof(out->T));
    out->n_corr = (int64_t)n_corr;
    out->n_src = (int64_t)n_src;
    out->fitness = n_src > 0 ? n_corr / n_src : 0.0;
    out->rmse = n_corr > 0 ? sqrt(e / n_corr) : 0.0;
    out->iters_run = h.iters_run;
    out->status = h.status;
    out->scale = h.scale;
}
static void read_eval(const double *s, tl3d_icp_eval *o) {
    memcpy(o->A, s, 21 * sizeof(double));
    memcpy(o->b, s + 21, 6 * sizeof(double));
    o->e = s[ICP_SUM_E];
    o->n_corr = (int64_t)s[ICP_SUM_CORR];
    o->n_src = (int64_t)s[ICP_SUM_SRC];
}

// ---- the buffers: each struct is freed as a whole and left all zero, which is also how a failed first-use allocation leaves it
static void icp_lane_free(tl3d_ctx::IcpLane &ln) {
    if (ln.slab) (void)hipFree(ln.slab);
    if (ln.ticket) (void)hipFree(ln.ticket);
    if (ln.state) (void)hipFree(ln.state);
    for (int g = 0; g < 4; ++g)
        if (ln.graphs[g]) (void)hipGraphExecDestroy(ln.graphs[g]);
    if (ln.host) (void)hipHostFree(ln.host);
    if (ln.run) (void)hipFree(ln.run);
    if (ln.run_host) (void)hipHostFree(ln.run_host);
    if (ln.ev_done) (void)hipEventDestroy(ln.ev_done);
    if (ln.stream) (void)hipStreamDestroy(ln.stream);
    memset(&ln, 0, sizeof(ln));
}

static void icp_batch_free(tl3d_ctx::IcpBatch &b) {
    if (b.pairs) (void)hipFree(b.pairs);
    if (b.states) (void)hipFree(b.states);
    if (b.sync) (void)hipFree(b.sync);
    if (b.ctl) (void)hipFree(b.ctl);
    if (b.slab) (void)hipFree(b.slab);
    if (b.dbg) (void)hipFree(b.dbg);
    if (b.stage) (void)hipFree(b.stage);
    if (b.pairs_host) (void)hipHostFree(b.pairs_host);
    if (b.states_host) (void)hipHostFree(b.states_host);
    if (b.ctl_host) (void)hipHostFree(b.ctl_host);
    free(b.req_pairs);
    if (b.ev_ready) (void)hipEventDestroy(b.ev_ready);
    if (b.ev_done) (void)hipEventDestroy(b.ev_done);
    if (b.stream) (void)hipStreamDestroy(b.stream);
    memset(&b, 0, sizeof(b));
}

static void track_free(tl3d_ctx::Track &tr) {
    if (tr.state) (void)hipFree(tr.state);
    if (tr.host) (void)hipHostFree(tr.host);
    if (tr.slab) (void)hipFree(tr.slab);
    memset(&tr, 0, sizeof(tr));
}

static void cloud_free(tl3d_ctx::Cloud &cl) {
    if (cl.state) (void)hipFree(cl.state);
    if (cl.host) (void)hipHostFree(cl.host);
    memset(&cl, 0, sizeof(cl));
}

namespace tl3d {
void registration_release(tl3d_ctx *ctx) {
    cloud_free(ctx->cloud);
    for (int l = 0; l < TL3D_ICP_LANES; ++l) {
        tl3d_ctx::IcpLane &ln = ctx->icp_lanes[l];
        if (ln.stream) (void)hipStreamSynchronize(ln.stream);
        icp_lane_free(ln);
    }
    if (ctx->icp_batch.stream) (void)hipStreamSynchronize(ctx->icp_batch.stream);
    icp_batch_free(ctx->icp_batch);
    if (ctx->icp_eval.pairs) (void)hipFree(ctx->icp_eval.pairs);
    if (ctx->icp_eval.slab) (void)hipFree(ctx->icp_eval.slab);
    if (ctx->icp_eval.sums) (void)hipFree(ctx->icp_eval.sums);
    track_free(ctx->track);
    if (ctx->rgbd.pairs) (void)hipFree(ctx->rgbd.pairs);
    if (ctx->rgbd.states) (void)hipFree(ctx->rgbd.states);
    if (ctx->rgbd.slab) (void)hipFree(ctx->rgbd.slab);
}
}  // namespace tl3d

extern "C" {

// ------------------------------------------------------------------------------------------- normal maps
int tl3d_build_normals(tl3d_ctx *ctx, int slot, double scale, double depth_jump) {
    int rc = check_slot(ctx, slot, true);
    if (rc) return rc;
    TL3D_HIP(hipSetDevice(ctx->device));
    Slot &s = ctx->slots[slot];
    if (!s.nmap && !(s.nmap = (float4 *)pool_take(ctx->pool_nmap))) return set_err(TL3D_E_NOMEM, "normal map alloc failed");
    rc = order_after_lanes(ctx, slot, false, true);     // an uncollected ICP run may still read this slot's normal map
    if (rc) return rc;
    const int radius = ctx->normal_radius;
    if (radius > 0 && !s.sdepth && !(s.sdepth = (float *)pool_take(ctx->pool_sdepth))) return set_err(TL3D_E_NOMEM, "smoothed depth alloc failed");
    if (radius > 0 || s.smooth_radius > 0) {
        rc = order_after_lanes(ctx, slot, true, false);  // ... or this slot's (smoothed) depth as its source
        if (rc) return rc;
    }
    rc = launch_normals(ctx->stream, ctx->cam, s.depth, (float)scale, (float)ctx->cfg.min_depth, (float)ctx->cfg.max_depth,
                        (float)depth_jump, radius, s.sdepth, s.nmap);
    if (rc) return rc;
    s.smooth_radius = radius;
    s.has_normals = true;
    if (!s.ev_normals) TL3D_HIP(hipEventCreateWithFlags(&s.ev_normals, hipEventDisableTiming));
    TL3D_HIP(hipEventRecord(s.ev_normals, ctx->stream));      // ICP lanes wait on this, not on the whole main stream
    return TL3D_OK;
}

int tl3d_download_normals(tl3d_ctx *ctx, int slot, float *out) {
    int rc = check_slot(ctx, slot, true);
    if (rc) return rc;
    REQUIRE(out != nullptr, TL3D_E_INVALID, "null out");
    REQUIRE(ctx->slots[slot].has_normals, TL3D_E_STATE, "slot %d has no normal map (call tl3d_build_normals)", slot);
    return download_pm_map(ctx, ctx->slots[slot].nmap, out);
}

int tl3d_build_normals_many(tl3d_ctx *ctx, int n, const int32_t *slots, const double *scales, double depth_jump) {
    REQUIRE(ctx && slots, TL3D_E_INVALID, "null argument");
    for (int i = 0; i < n; ++i) {
        const int rc = tl3d_build_normals(ctx, slots[i], scales ? scales[i] : 1.0, depth_jump);
        if (rc) return rc;
    }
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- ICP lanes: one kernel per iteration
// all or nothing: a lane whose stream exists has every buffer (a half-built lane would launch kernels on null pointers)
static int icp_lane_init(tl3d_ctx *ctx, int lane) {
    tl3d_ctx::IcpLane &ln = ctx->icp_lanes[lane];
    if (ln.stream) return TL3D_OK;
    bool ok = hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipMalloc(&ln.slab, (size_t)ICP_MAX_BLOCKS * ICP_SLAB * sizeof(double)) == hipSuccess;
    ok = ok && hipMalloc(&ln.ticket, 64) == hipSuccess;
    ok = ok && hipMalloc(&ln.state, sizeof(IcpState)) == hipSuccess;
    ok = ok && hipHostMalloc(&ln.host, sizeof(IcpState), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipMalloc(&ln.run, sizeof(IcpRun)) == hipSuccess;
    ok = ok && hipHostMalloc(&ln.run_host, sizeof(IcpRun), hipHostMallocDefault) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&ln.ev_done, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        icp_lane_free(ln);
        return set_err(TL3D_E_NOMEM, "ICP lane %d: stream / buffer allocation failed", lane);
    }
    for (int g = 0; g < 4; ++g) ln.graph_iters[g] = -1;      // (the rest of a lane without a stream is zero: tl3d_create, icp_lane_free)
    ln.src_slot = ln.tgt_slot = -1;
    return TL3D_OK;
}

int tl3d_icp_enqueue(tl3d_ctx *ctx, int lane, int slot_src, double scale_src, int slot_tgt, const double T_init[16],
                     const tl3d_icp_params *prm) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(lane >= 0 && lane < TL3D_ICP_LANES, TL3D_E_INVALID, "lane %d out of range [0,%d)", lane, TL3D_ICP_LANES);
    REQUIRE(prm != nullptr, TL3D_E_INVALID, "null argument");
    int rc = check_level(*prm, 0);                      // any positive max_dist, infinity included: the evaluation and the tracking refuse >= 1e18
    if (!rc) rc = check_pair(ctx, slot_src, slot_tgt, 0);
    if (rc) return rc;
    TL3D_HIP(hipSetDevice(ctx->device));
    rc = icp_lane_init(ctx, lane);
    if (rc) return rc;
    tl3d_ctx::IcpLane &ln = ctx->icp_lanes[lane];
    REQUIRE(!ln.busy, TL3D_E_STATE, "ICP lane %d still holds an uncollected run", lane);
    // order this run after the frames it reads became valid on the main stream
    Slot &ss = ctx->slots[slot_src], &st = ctx->slots[slot_tgt];
    if (ss.ev_upload) TL3D_HIP(hipStreamWaitEvent(ln.stream, ss.ev_upload, 0));
    if (st.ev_upload) TL3D_HIP(hipStreamWaitEvent(ln.stream, st.ev_upload, 0));
    if (st.ev_normals) TL3D_HIP(hipStreamWaitEvent(ln.stream, st.ev_normals, 0));
    if (ss.smooth_radius > 0 && ss.ev_normals) TL3D_HIP(hipStreamWaitEvent(ln.stream, ss.ev_normals, 0));     // the averaged depth is written with the source's normal map
    IcpState *h = ln.host;
    memset(h, 0, sizeof(*h));
    if (T_init) memcpy(h->T, T_init, sizeof(h->T));
    else h->T[0] = h->T[5] = h->T[10] = h->T[15] = 1.0;
    h->scale = scale_src;
    const IcpLevel L = make_level(ctx->cam, *prm);
    IcpRun *r = ln.run_host;
    describe_pair(r, ss, st, scale_src);
    r->mind = (float)ctx->cfg.min_depth;
    r->maxd = (float)ctx->cfg.max_depth;
    r->md2 = L.md2; r->stride = L.stride; r->Ws = L.Ws; r->Hs = L.Hs; r->est_scale = L.est_scale;
    r->damping = L.damping; r->eps = L.eps; r->eig_rel = L.eig_rel;
    // The chain's launch arguments never change (everything per-run sits behind ln.run / ln.state / pinned buffers), so
    // it is captured once per iteration count and replayed: one host call per registration instead of ~25.
    int gi = -1;
    for (int g = 0; g < 4; ++g)
        if (ln.graphs[g] && ln.graph_iters[g] == prm->iters) gi = g;
    if (gi < 0) {
        gi = ln.graph_next;
        ln.graph_next = (ln.graph_next + 1) & 3;
        if (ln.graphs[gi]) { (void)hipGraphExecDestroy(ln.graphs[gi]); ln.graphs[gi] = nullptr; }
        hipGraph_t g = nullptr;
        TL3D_HIP(hipStreamBeginCapture(ln.stream, hipStreamCaptureModeThreadLocal));
        hipError_t ce = hipMemcpyAsync(ln.run, ln.run_host, sizeof(IcpRun), hipMemcpyHostToDevice, ln.stream);
        if (ce == hipSuccess) ce = hipMemcpyAsync(ln.state, ln.host, sizeof(IcpState), hipMemcpyHostToDevice, ln.stream);
        if (ce == hipSuccess) ce = hipMemsetAsync(ln.ticket, 0, 64, ln.stream);      // polled words are re-armed by every replay
        int lrc = TL3D_OK;
        for (int it = 0; ce == hipSuccess && lrc == TL3D_OK && it <= prm->iters; ++it)
            lrc = launch_icp_iteration(ln.stream, ctx->cam, ln.run, it == prm->iters, ln.slab, ln.state, ICP_MAX_BLOCKS, ln.ticket);
        if (ce == hipSuccess && lrc == TL3D_OK) ce = hipMemcpyAsync(ln.host, ln.state, sizeof(IcpState), hipMemcpyDeviceToHost, ln.stream);
        hipError_t ee = hipStreamEndCapture(ln.stream, &g);
        if (ce != hipSuccess || ee != hipSuccess || lrc != TL3D_OK || !g) {
            if (g) (void)hipGraphDestroy(g);
            return set_err(TL3D_E_HIP, "ICP graph capture failed: %s", hipGetErrorString(ce != hipSuccess ? ce : ee));
        }
        hipError_t ie = hipGraphInstantiate(&ln.graphs[gi], g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (ie != hipSuccess) { ln.graphs[gi] = nullptr; return set_err(TL3D_E_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(ie)); }
        ln.graph_iters[gi] = prm->iters;
    }
    TL3D_HIP(hipGraphLaunch(ln.graphs[gi], ln.stream));
    TL3D_HIP(hipEventRecord(ln.ev_done, ln.stream));
    ln.busy = true;
    ln.src_slot = slot_src;
    ln.tgt_slot = slot_tgt;
    return TL3D_OK;
}

int tl3d_icp_collect(tl3d_ctx *ctx, int lane, tl3d_icp_result *out) {
    REQUIRE(ctx && out, TL3D_E_INVALID, "null argument");
    REQUIRE(lane >= 0 && lane < TL3D_ICP_LANES, TL3D_E_INVALID, "lane %d out of range [0,%d)", lane, TL3D_ICP_LANES);
    tl3d_ctx::IcpLane &ln = ctx->icp_lanes[lane];
    REQUIRE(ln.stream && ln.busy, TL3D_E_STATE, "ICP lane %d holds no run", lane);
    TL3D_HIP(hipSetDevice(ctx->device));
    TL3D_HIP(hipStreamSynchronize(ln.stream));
    ln.busy = false;
    read_result(*ln.host, out);
    return TL3D_OK;
}

int tl3d_icp_p2plane(tl3d_ctx *ctx, int slot_src, double scale_src, int slot_tgt, const double T_init[16],
                     const tl3d_icp_params *prm, tl3d_icp_result *out) {
    REQUIRE(out != nullptr, TL3D_E_INVALID, "null argument");
    const int rc = tl3d_icp_enqueue(ctx, 0, slot_src, scale_src, slot_tgt, T_init, prm);
    return rc ? rc : tl3d_icp_collect(ctx, 0, out);
}

// ---- batched registration: all pairs, all levels, all iterations in one launch (icp_batch_kernel) ----------------------
static int icp_batch_reserve(tl3d_ctx *ctx, int n_pairs, size_t slab_doubles) {
    tl3d_ctx::IcpBatch &b = ctx->icp_batch;
    bool ok = true;
    if (!b.stream) {
        ok = hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&b.ev_ready, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&b.ev_done, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipMalloc(&b.ctl, 64) == hipSuccess;
        ok = ok && hipHostMalloc(&b.ctl_host, 64, hipHostMallocDefault) == hipSuccess;
    }
    if (ok && n_pairs > b.cap_pairs) {
        const int cap = n_pairs < 64 ? 64 : n_pairs;
        if (b.pairs) (void)hipFree(b.pairs);
        if (b.states) (void)hipFree(b.states);
        if (b.sync) (void)hipFree(b.sync);
        if (b.pairs_host) (void)hipHostFree(b.pairs_host);
        if (b.states_host) (void)hipHostFree(b.states_host);
        b.pairs = nullptr; b.states = nullptr; b.sync = nullptr; b.pairs_host = nullptr; b.states_host = nullptr;
        b.cap_pairs = 0;
        ok = hipMalloc(&b.pairs, (size_t)cap * sizeof(IcpBatchPair)) == hipSuccess;
        ok = ok && hipMalloc(&b.states, (size_t)cap * sizeof(IcpState)) == hipSuccess;
        int rows = (cap + 63) / 64;
        if (rows < 68) rows = 68;                            // neighbours' lines 4352 B apart at least
        ok = ok && hipMalloc(&b.sync, (size_t)2 * 64 * rows * 64) == hipSuccess;
        if (ok) b.sync_rows = rows;
        ok = ok && hipHostMalloc(&b.pairs_host, (size_t)cap * sizeof(IcpBatchPair), hipHostMallocDefault) == hipSuccess;
        ok = ok && hipHostMalloc(&b.states_host, (size_t)cap * sizeof(IcpState), hipHostMallocDefault) == hipSuccess;
        if (ok) b.cap_pairs = cap;
    }
    if (ok && slab_doubles > b.cap_slab) {
        if (b.slab) (void)hipFree(b.slab);
        b.slab = nullptr;
        b.cap_slab = 0;
        ok = hipMalloc(&b.slab, slab_doubles * sizeof(double)) == hipSuccess;
        if (ok) b.cap_slab = slab_doubles;
    }
    if (!ok) {
        (void)hipGetLastError();
        icp_batch_free(b);
        return set_err(TL3D_E_NOMEM, "ICP batch: stream / buffer allocation failed");
    }
    return TL3D_OK;
}

int tl3d_icp_batch_enqueue(tl3d_ctx *ctx, const tl3d_icp_pair *pairs, int n_pairs, const tl3d_icp_params *levels, int n_levels) {
    REQUIRE(ctx && pairs && levels, TL3D_E_INVALID, "null argument");
    REQUIRE(n_pairs >= 1 && n_pairs <= (1 << 20), TL3D_E_INVALID, "n_pairs %d out of range", n_pairs);
    REQUIRE(n_levels >= 1 && n_levels <= TL3D_ICP_MAX_LEVELS, TL3D_E_INVALID, "n_levels %d out of range [1,%d]", n_levels, TL3D_ICP_MAX_LEVELS);
    REQUIRE(!ctx->icp_batch.busy, TL3D_E_STATE, "an ICP batch is still uncollected");
    IcpBatchArgs a;
    memset(&a, 0, sizeof(a));
    long long ns_max = 1;
    for (int l = 0; l < n_levels; ++l) {
        const int rc = check_level(levels[l], 0);       // any positive max_dist, infinity included: the evaluation and the tracking refuse >= 1e18
        if (rc) return rc;
        a.lv[l] = make_level(ctx->cam, levels[l]);
        const long long ns = (long long)a.lv[l].Ws * a.lv[l].Hs;
        if (ns > ns_max) ns_max = ns;
    }
    for (int i = 0; i < n_pairs; ++i) {
        const int rc = check_pair(ctx, pairs[i].slot_src, pairs[i].slot_tgt, i);
        if (rc) return rc;
    }
    // workgroups per pair: a function of the level geometry only, so a pair's sums (and pose) do not depend on the batch it is in
    long long members = (ns_max + ICP_BATCH_SAMPLES_PER_MEMBER - 1) / ICP_BATCH_SAMPLES_PER_MEMBER;
    if (members > ICP_BATCH_MEMBERS_CAP) members = ICP_BATCH_MEMBERS_CAP;
#ifdef TL3D_EXPERIMENTS
    if (const char *e = getenv("TL3D_ICP_MEMBERS")) {
        const long long m = atoll(e);
        if (m >= 1 && m <= ICP_BATCH_MAX_MEMBERS) members = m;
    }
#endif
    TL3D_HIP(hipSetDevice(ctx->device));
    int rc = icp_batch_reserve(ctx, n_pairs, (size_t)n_pairs * (size_t)members * ICP_SLAB);
    if (rc) return rc;
    tl3d_ctx::IcpBatch &b = ctx->icp_batch;
    if (n_pairs > b.req_cap) {
        free(b.req_pairs);
        b.req_pairs = (tl3d_icp_pair *)malloc((size_t)n_pairs * sizeof(tl3d_icp_pair));
        b.req_cap = b.req_pairs ? n_pairs : 0;
        REQUIRE(b.req_pairs != nullptr, TL3D_E_NOMEM, "host allocation failed");
    }
    memcpy(b.req_pairs, pairs, (size_t)n_pairs * sizeof(tl3d_icp_pair));
    memcpy(b.req_levels, levels, (size_t)n_levels * sizeof(tl3d_icp_params));
    b.req_n_levels = n_levels;
    for (int i = 0; i < n_pairs; ++i) {
        describe_pair(&b.pairs_host[i], ctx->slots[pairs[i].slot_src], ctx->slots[pairs[i].slot_tgt], pairs[i].scale_src);
        IcpState &h = b.states_host[i];
        memset(&h, 0, sizeof(h));
        memcpy(h.T, pairs[i].T_init, sizeof(h.T));
        h.scale = pairs[i].scale_src;
    }
    // uploads and normal maps are issued on the main stream: everything issued there so far precedes the batch
    TL3D_HIP(hipEventRecord(b.ev_ready, ctx->stream));
    TL3D_HIP(hipStreamWaitEvent(b.stream, b.ev_ready, 0));
    TL3D_HIP(hipMemcpyAsync(b.pairs, b.pairs_host, (size_t)n_pairs * sizeof(IcpBatchPair), hipMemcpyHostToDevice, b.stream));
    TL3D_HIP(hipMemcpyAsync(b.states, b.states_host, (size_t)n_pairs * sizeof(IcpState), hipMemcpyHostToDevice, b.stream));
    TL3D_HIP(hipMemsetAsync(b.sync, 0, (size_t)2 * 64 * b.sync_rows * 64, b.stream));
    TL3D_HIP(hipMemsetAsync(b.ctl, 0, 64, b.stream));
    a.pairs = b.pairs;
    a.states = b.states;
    a.sync = b.sync;
    a.slab = b.slab;
    a.ctl = b.ctl;
    a.n_pairs = n_pairs;
    a.members = (int)members;
    a.n_levels = n_levels;
    a.sync_rows = b.sync_rows;
    a.mind = (float)ctx->cfg.min_depth;
    a.maxd = (float)ctx->cfg.max_depth;
#ifdef TL3D_EXPERIMENTS
    if (getenv("TL3D_ICP_TRACE")) {                        // per-pass timestamps of pair 0
        if (b.dbg) (void)hipFree(b.dbg);
        b.dbg = nullptr;
        TL3D_HIP(hipMalloc(&b.dbg, (size_t)members * 16 * 8 * sizeof(unsigned long long)));
        TL3D_HIP(hipMemsetAsync(b.dbg, 0, (size_t)members * 16 * 8 * sizeof(unsigned long long), b.stream));
        b.dbg_members = (int)members;
        a.dbg = b.dbg;
    }
    if (getenv("TL3D_ICP_STAGES")) {
        if (b.stage) (void)hipFree(b.stage);
        b.stage = nullptr;
        b.stage_n = (size_t)n_pairs * members;
        TL3D_HIP(hipMalloc(&b.stage, b.stage_n * 16));
        TL3D_HIP(hipMemsetAsync(b.stage, 0, b.stage_n * 16, b.stream));
        a.stage = b.stage;
    }
#endif
    rc = launch_icp_batch(b.stream, ctx->cam, a);
    if (rc) return rc;
    TL3D_HIP(hipMemcpyAsync(b.states_host, b.states, (size_t)n_pairs * sizeof(IcpState), hipMemcpyDeviceToHost, b.stream));
    TL3D_HIP(hipMemcpyAsync(b.ctl_host, b.ctl, 64, hipMemcpyDeviceToHost, b.stream));
    TL3D_HIP(hipEventRecord(b.ev_done, b.stream));
    b.n_pairs = n_pairs;
    b.busy = true;
    return TL3D_OK;
}

// The batch of the last enqueue, registered by the per-iteration kernel: up to TL3D_ICP_LANES pairs side by side, level
// after level; a pair's next level starts from the pose (and scale) its previous level ended with, and a pair stops when a
// level fails or ends with fewer than 8 correspondences -- the rule icp_batch_kernel applies between its levels.
static int icp_batch_fallback(tl3d_ctx *ctx, tl3d_icp_result *out, int n_out) {
    tl3d_ctx::IcpBatch &b = ctx->icp_batch;
    for (int l = 0; l < TL3D_ICP_LANES; ++l)
        REQUIRE(!ctx->icp_lanes[l].busy, TL3D_E_STATE, "the batched registration timed out and ICP lane %d holds an uncollected run: cannot fall back", l);
    std::vector<char> over((size_t)n_out, 0);
    for (int i = 0; i < n_out; ++i) {
        memset(&out[i], 0, sizeof(out[i]));
        memcpy(out[i].T, b.req_pairs[i].T_init, sizeof(out[i].T));
        out[i].scale = b.req_pairs[i].scale_src;
    }
    for (int lv = 0; lv < b.req_n_levels; ++lv)
        for (int i0 = 0; i0 < n_out; i0 += TL3D_ICP_LANES) {
            const int m = n_out - i0 < TL3D_ICP_LANES ? n_out - i0 : TL3D_ICP_LANES;
            for (int k = 0; k < m; ++k) {
                const int i = i0 + k;
                if (over[i]) continue;
                const int rc = tl3d_icp_enqueue(ctx, k, b.req_pairs[i].slot_src, out[i].scale, b.req_pairs[i].slot_tgt, out[i].T, &b.req_levels[lv]);
                if (rc) return rc;
            }
            for (int k = 0; k < m; ++k) {
                const int i = i0 + k;
                if (over[i]) continue;
                const int rc = tl3d_icp_collect(ctx, k, &out[i]);
                if (rc) return rc;
                if (out[i].status == 2 || out[i].n_corr < 8) over[i] = 1;
            }
        }
    ctx->stats.icp_batch_fallback_pairs += (uint64_t)n_out;
    return TL3D_OK;
}

int tl3d_icp_batch_collect(tl3d_ctx *ctx, tl3d_icp_result *out, int n_out) {
    REQUIRE(ctx && out, TL3D_E_INVALID, "null argument");
    tl3d_ctx::IcpBatch &b = ctx->icp_batch;
    REQUIRE(b.stream && b.busy, TL3D_E_STATE, "no ICP batch in flight");
    REQUIRE(n_out == b.n_pairs, TL3D_E_INVALID, "the batch in flight has %d pairs, not %d", b.n_pairs, n_out);
    TL3D_HIP(hipSetDevice(ctx->device));
    TL3D_HIP(hipStreamSynchronize(b.stream));
    b.busy = false;
#ifdef TL3D_EXPERIMENTS
    if (b.dbg && getenv("TL3D_ICP_TRACE")) {
        std::vector<unsigned long long> h((size_t)b.dbg_members * 16 * 8);
        TL3D_HIP(hipMemcpy(h.data(), b.dbg, h.size() * 8, hipMemcpyDeviceToHost));
        FILE *f = fopen(getenv("TL3D_ICP_TRACE"), "w");
        if (f) {
            unsigned long long t0 = ~0ull;
            for (size_t i = 0; i < h.size(); ++i)
                if ((i & 7) < 7 && h[i] && h[i] < t0) t0 = h[i];
            for (int m = 0; m < b.dbg_members; ++m)
                for (int g = 0; g < 16; ++g) {
                    const unsigned long long *r = &h[((size_t)m * 16 + g) * 8];
                    if (!r[0]) continue;
                    fprintf(f, "%d %d %llu", m, g, r[7]);
                    for (int k = 0; k < 7; ++k) fprintf(f, " %lld", r[k] ? (long long)(r[k] - t0) : -1ll);
                    fprintf(f, "\n");
                }
            fclose(f);
        }
    }
    if (b.stage && b.ctl_host[1] != 0 && getenv("TL3D_ICP_STAGES")) {
        std::vector<unsigned> h(b.stage_n * 4);
        TL3D_HIP(hipMemcpy(h.data(), b.stage, h.size() * 4, hipMemcpyDeviceToHost));
        const size_t mem = b.stage_n / (size_t)b.n_pairs;
        size_t hist[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < b.stage_n; ++i) hist[h[i * 4] & 3u]++;
        fprintf(stderr, "stages: never started %zu, started %zu, accumulated %zu, arrived %zu\n", hist[0], hist[1], hist[2], hist[3]);
        const size_t p0 = b.ctl_host[4];
        for (size_t m = 0; m < mem; ++m) {
            const unsigned *r = &h[(p0 * mem + m) * 4];
            fprintf(stderr, "  pair %zu ticket-member %zu: stage %u pass %u block %u arrived-as %u hwid %08x\n", p0, m, r[0] & 15u, r[0] >> 4, r[1], r[2], r[3]);
        }
    }
#endif
    bool timed_out = b.ctl_host[1] != 0;
#ifdef TL3D_EXPERIMENTS
    if (getenv("TL3D_ICP_FORCE_TIMEOUT")) timed_out = true;              // rehearsal of the fallback below
#endif
    if (timed_out) {
        // A wait inside the launch ran into its time bound (the waits need a pair's other workgroups to be running; other
        // work on the chip can, in principle, keep them off it).  The launch has ended; its results are discarded and the
        // whole batch is registered again by the per-iteration kernel on the ICP lanes, which waits for nobody inside a
        // launch: same levels, same chaining rule.
        ctx->stats.icp_batch_timeouts++;
        fprintf(stderr, "libtl3d: batched registration timed out inside its launch (pair %u member %u pass %u level %u iteration %u: %u of its "
                        "workgroups had arrived, %u workgroups started); re-registering %d pairs on the per-iteration kernel\n",
                b.ctl_host[4], b.ctl_host[5], b.ctl_host[6], b.ctl_host[10], b.ctl_host[11], b.ctl_host[8], b.ctl_host[0], n_out);
        return icp_batch_fallback(ctx, out, n_out);
    }
    for (int i = 0; i < n_out; ++i) read_result(b.states_host[i], &out[i]);
    return TL3D_OK;
}

// ---- pairs scored at given poses: one pass each, no update (kernels_icp_eval.hip) ---------------------------------------
int tl3d_icp_evaluate_pairs(tl3d_ctx *ctx, const tl3d_icp_pair *pairs, int n_pairs, int stride, double max_dist, tl3d_icp_eval *out) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(n_pairs >= 0, TL3D_E_INVALID, "n_pairs %d is negative", n_pairs);
    const tl3d_icp_params lv = {0, stride, max_dist};     // one pass at one stride; the rest 0
    int rc = check_level(lv, LV_FINITE_GATE);           // max_dist below 1e18: the lanes and the batch take any positive one
    if (rc) return rc;
    REQUIRE(n_pairs == 0 || (pairs && out), TL3D_E_INVALID, "null argument");
    REQUIRE(!ctx->icp_batch.busy, TL3D_E_STATE, "an ICP batch is still uncollected");
    for (int i = 0; i < n_pairs; ++i) {
        rc = check_pair(ctx, pairs[i].slot_src, pairs[i].slot_tgt, i);
        if (rc) return rc;
    }
    if (n_pairs == 0) return TL3D_OK;
    const IcpLevel L = make_level(ctx->cam, lv);
    const int members = icp_eval_members(L.Ws, L.Hs);
    size_t chunk = ICP_EVAL_SLAB_DOUBLES / ((size_t)members * ICP_EVAL_SUMS);
    if (chunk < 1) chunk = 1;
    if (chunk > 32768) chunk = 32768;                      // the pair is the launch's grid.y
    if (chunk > (size_t)n_pairs) chunk = (size_t)n_pairs;
    TL3D_HIP(hipSetDevice(ctx->device));
    tl3d_ctx::IcpEval &b = ctx->icp_eval;
    int grc = chunk <= b.cap_pairs ? TL3D_OK : grow_pair(&b.pairs, &b.sums, &b.cap_pairs, chunk < 64 ? 64 : chunk, "ICP evaluation");
    if (!grc) grc = grow(&b.slab, &b.cap_slab, chunk * members * ICP_EVAL_SUMS, "ICP evaluation slab");
    if (grc) return grc;
    std::vector<IcpEvalPair> hp(chunk);
    std::vector<double> hs(chunk * ICP_EVAL_SUMS);
    // the main stream: behind every upload and normal map issued so far
    for (size_t i0 = 0; i0 < (size_t)n_pairs; i0 += chunk) {
        const size_t m = (size_t)n_pairs - i0 < chunk ? (size_t)n_pairs - i0 : chunk;
        for (size_t k = 0; k < m; ++k) {
            const tl3d_icp_pair &p = pairs[i0 + k];
            describe_pair(&hp[k], ctx->slots[p.slot_src], ctx->slots[p.slot_tgt], p.scale_src);
            for (int j = 0; j < 12; ++j) hp[k].T[j] = (float)p.T_init[j];
        }
        TL3D_HIP(hipMemcpyAsync(b.pairs, hp.data(), m * sizeof(IcpEvalPair), hipMemcpyHostToDevice, ctx->stream));
        rc = launch_icp_eval(ctx->stream, ctx->cam, b.pairs, (int)m, members, (float)ctx->cfg.min_depth, (float)ctx->cfg.max_depth, L.md2, L.stride,
                             L.Ws, L.Hs, b.slab, *b.sums);
        if (rc) return rc;
        TL3D_HIP(hipMemcpyAsync(hs.data(), b.sums, m * ICP_EVAL_SUMS * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        TL3D_HIP(hipStreamSynchronize(ctx->stream));
        for (size_t k = 0; k < m; ++k) read_eval(&hs[k * ICP_EVAL_SUMS], &out[i0 + k]);
    }
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- tracking against the TSDF
// the checks, the flush and the buffers both tracking calls share; on return the main stream is behind every upload into the slot
static int track_prepare(tl3d_ctx *ctx, int slot, const double R[9], const double t[3]) {
    REQUIRE(R && t, TL3D_E_INVALID, "null pose");
    int rc = check_slot(ctx, slot, false);                  // (and ctx)
    if (rc) return rc;
    REQUIRE(ctx->tsdf != nullptr, TL3D_E_STATE, "tracking needs a grid with a TSDF channel");
    REQUIRE(!ctx->has_core && ctx->cfg.voxel_offset[0] == 0 && ctx->cfg.voxel_offset[1] == 0 && ctx->cfg.voxel_offset[2] == 0, TL3D_E_STATE,
            "tracking needs a whole lattice: this grid is a block (voxel offset or core set)");
    REQUIRE(ctx->slots[slot].loaded, TL3D_E_STATE, "slot %d holds no frame", slot);
    REQUIRE(!ctx->icp_batch.busy, TL3D_E_STATE, "an ICP batch is still uncollected");
    FLUSH_AND_FOLD(ctx);
    TL3D_HIP(hipSetDevice(ctx->device));
    tl3d_ctx::Track &tr = ctx->track;
    if (!tr.state) {                                        // all or nothing, as icp_lane_init
        bool ok = hipMalloc(&tr.state, sizeof(IcpState)) == hipSuccess;
        ok = ok && hipHostMalloc(&tr.host, sizeof(IcpState), hipHostMallocDefault) == hipSuccess;
        ok = ok && hipMalloc(&tr.slab, (size_t)track_members(ctx->cam.W, ctx->cam.H) * TRACK_SUMS * sizeof(double)) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            track_free(tr);
            return set_err(TL3D_E_NOMEM, "tracking: buffer allocation failed");
        }
    }
    IcpState *h = tr.host;
    memset(h, 0, sizeof(*h));
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) h->T[4 * i + j] = R[3 * i + j];
        h->T[4 * i + 3] = t[i];
    }
    h->T[15] = 1.0;
    TL3D_HIP(hipMemcpyAsync(tr.state, h, sizeof(IcpState), hipMemcpyHostToDevice, ctx->stream));
    return TL3D_OK;
}

// one pass and the step behind it (the sums in member order; STEP_ITERATE: solve and pose update too)
static int track_pass_step(tl3d_ctx *ctx, int slot, double scale, int min_weight, const tl3d_icp_params &p, StepKind kind) {
    tl3d_ctx::Track &tr = ctx->track;
    int rc = launch_track_pass(ctx->stream, ctx->cam, ctx->grid, ctx->slots[slot].depth, (float)scale, (float)ctx->cfg.min_depth,
                               (float)ctx->cfg.max_depth, min_weight, p.stride, p.max_dist, ctx->tsdf, tr.state, kind, tr.slab);
    if (rc) return rc;
    const IcpLevel L = make_level(ctx->cam, p);
    return launch_track_step(ctx->stream, tr.slab, track_members(L.Ws, L.Hs), tr.state, p.damping, p.eps, p.eig_rel, kind);
}

static int track_collect(tl3d_ctx *ctx) {
    tl3d_ctx::Track &tr = ctx->track;
    TL3D_HIP(hipMemcpyAsync(tr.host, tr.state, sizeof(IcpState), hipMemcpyDeviceToHost, ctx->stream));
    TL3D_HIP(hipStreamSynchronize(ctx->stream));
    return TL3D_OK;
}

int tl3d_track_evaluate(tl3d_ctx *ctx, int slot, double scale, const double R[9], const double t[3], int min_weight, int stride,
                        double max_dist, tl3d_icp_eval *out) {
    REQUIRE(out != nullptr, TL3D_E_INVALID, "null argument");
    const tl3d_icp_params lv = {0, stride, max_dist};     // one pass at one stride; the rest 0 (the step of a final pass reads none of it)
    int rc = check_level(lv, LV_FINITE_GATE);           // max_dist below 1e18: the lanes and the batch take any positive one
    if (!rc) rc = track_prepare(ctx, slot, R, t);
    if (!rc) rc = track_pass_step(ctx, slot, scale, min_weight, lv, step_kind(0, 0, true, true));
    if (!rc) rc = track_collect(ctx);
    if (rc) return rc;
    read_eval(ctx->track.host->sums, out);
    return TL3D_OK;
}

int tl3d_track_frame(tl3d_ctx *ctx, int slot, double scale, const double R_init[9], const double t_init[3], int min_weight,
                     const tl3d_icp_params *levels, int n_levels, tl3d_icp_result *out) {
    REQUIRE(out != nullptr, TL3D_E_INVALID, "null argument");
    REQUIRE(n_levels >= 1 && n_levels <= TL3D_ICP_MAX_LEVELS, TL3D_E_INVALID, "n_levels %d outside [1,%d]", n_levels, TL3D_ICP_MAX_LEVELS);
    REQUIRE(levels != nullptr, TL3D_E_INVALID, "null argument");
    int rc = TL3D_OK;
    // max_dist below 1e18 and no estimate_scale: the lanes and the batch take any positive max_dist and estimate the scale
    for (int l = 0; l < n_levels && !rc; ++l) rc = check_level(levels[l], LV_FINITE_GATE | LV_NO_SCALE);
    if (!rc) rc = track_prepare(ctx, slot, R_init, t_init);
    // every launch of every level is enqueued now; launches behind a converged or failed level return at once
    for (int l = 0; l < n_levels && !rc; ++l) {
        for (int it = 0; it <= levels[l].iters && !rc; ++it)
            rc = track_pass_step(ctx, slot, scale, min_weight, levels[l], step_kind(it, levels[l].iters, l == n_levels - 1, false));
    }
    if (!rc) rc = track_collect(ctx);
    if (rc) return rc;
    read_result(*ctx->track.host, out);
    out->scale = scale;                                  // (tracking estimates none: the caller's)
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- joint point-to-plane + photometric
int tl3d_build_intensity_many(tl3d_ctx *ctx, int n, const int32_t *slots, int radius, double depth_jump) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(n >= 0 && (slots || n == 0), TL3D_E_INVALID, "null argument or negative n");
    REQUIRE(radius >= 0 && radius <= 7, TL3D_E_INVALID, "radius %d outside [0,7]", radius);
    REQUIRE(depth_jump > 0, TL3D_E_INVALID, "depth_jump must be positive");
    for (int i = 0; i < n; ++i) {
        const int rc = check_slot(ctx, slots[i], true);
        if (rc) return rc;
        REQUIRE(ctx->slots[slots[i]].has_color, TL3D_E_STATE, "slot %d holds no colour image", slots[i]);
    }
    if (n == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < n; ++i) {
        Slot &s = ctx->slots[slots[i]];
        if (!s.imap && !(s.imap = (float4 *)pool_take(ctx->pool_imap))) return set_err(TL3D_E_NOMEM, "intensity map alloc failed");
        // the main stream: behind the slot's upload and behind every registration that read the previous map (they block)
        const int rc = launch_intensity(ctx->stream, ctx->cam, s.depth, s.bgr, radius, (float)depth_jump, s.imap);
        if (rc) return rc;
        s.has_intensity = true;
        if (!s.ev_intensity) TL3D_HIP(hipEventCreateWithFlags(&s.ev_intensity, hipEventDisableTiming));
        TL3D_HIP(hipEventRecord(s.ev_intensity, ctx->stream));
    }
    return TL3D_OK;
}

int tl3d_download_intensity(tl3d_ctx *ctx, int slot, float *out) {
    int rc = check_slot(ctx, slot, true);
    if (rc) return rc;
    REQUIRE(out != nullptr, TL3D_E_INVALID, "null out");
    REQUIRE(ctx->slots[slot].has_intensity, TL3D_E_STATE, "slot %d has no intensity map (call tl3d_build_intensity_many)", slot);
    return download_pm_map(ctx, ctx->slots[slot].imap, out);
}

// what both calls check of their pairs: check_pair, then colour and intensity maps on both sides
static int rgbd_check_pairs(tl3d_ctx *ctx, const tl3d_icp_pair *pairs, int n_pairs) {
    for (int i = 0; i < n_pairs; ++i) {
        const int rc = check_pair(ctx, pairs[i].slot_src, pairs[i].slot_tgt, i);
        if (rc) return rc;
        const int sl[2] = {pairs[i].slot_src, pairs[i].slot_tgt};
        for (int k = 0; k < 2; ++k) {
            REQUIRE(ctx->slots[sl[k]].has_color, TL3D_E_STATE, "pair %d: slot %d holds no colour image", i, sl[k]);
            REQUIRE(ctx->slots[sl[k]].has_intensity, TL3D_E_STATE, "pair %d: slot %d has no intensity map (call tl3d_build_intensity_many)", i, sl[k]);
        }
    }
    return TL3D_OK;
}

static RgbdLevel rgbd_level(tl3d_ctx *ctx, const tl3d_icp_params &p, double photo_gate) {
    const IcpLevel L = make_level(ctx->cam, p);
    return RgbdLevel{L.md2, (float)photo_gate, (float)ctx->cfg.min_depth, (float)ctx->cfg.max_depth, L.stride, L.Ws, L.Hs, rgbd_members(L.Ws, L.Hs)};
}

// Every pair through `levels` in chunks the scratch holds: states up, every launch of every level, states down, one wait per chunk.
// eval: one final pass at the initial poses and nothing else.  hs: the final states, [n_pairs].
static int rgbd_run(tl3d_ctx *ctx, const tl3d_icp_pair *pairs, int n_pairs, const tl3d_rgbd_level *levels, int n_levels, bool eval,
                    std::vector<RgbdState> &hs) {
    std::vector<RgbdLevel> lv((size_t)n_levels);
    int members_max = 1;
    for (int l = 0; l < n_levels; ++l) {
        lv[l] = rgbd_level(ctx, levels[l].icp, levels[l].photo_gate);
        if (lv[l].members > members_max) members_max = lv[l].members;
    }
    size_t chunk = ICP_EVAL_SLAB_DOUBLES / ((size_t)members_max * RGBD_SUMS);
    if (chunk < 1) chunk = 1;
    if (chunk > 32768) chunk = 32768;                      // the pair is the launch's grid.y
    if (chunk > (size_t)n_pairs) chunk = (size_t)n_pairs;
    TL3D_HIP(hipSetDevice(ctx->device));
    tl3d_ctx::Rgbd &b = ctx->rgbd;
    int rc = chunk <= b.cap_pairs ? TL3D_OK : grow_pair(&b.pairs, &b.states, &b.cap_pairs, chunk < 64 ? 64 : chunk, "RGB-D registration");
    if (!rc) rc = grow(&b.slab, &b.cap_slab, chunk * members_max * RGBD_SUMS, "RGB-D registration slab");
    if (rc) return rc;
    std::vector<RgbdPair> hp(chunk);
    hs.assign((size_t)n_pairs, RgbdState());
    // the main stream: behind every upload, normal map and intensity map issued so far
    for (size_t i0 = 0; i0 < (size_t)n_pairs; i0 += chunk) {
        const size_t m = (size_t)n_pairs - i0 < chunk ? (size_t)n_pairs - i0 : chunk;
        for (size_t k = 0; k < m; ++k) {
            const tl3d_icp_pair &p = pairs[i0 + k];
            const Slot &ss = ctx->slots[p.slot_src], &st = ctx->slots[p.slot_tgt];
            describe_pair(&hp[k], ss, st, p.scale_src);
            hp[k].imap_src = ss.imap;
            hp[k].imap_tgt = st.imap;
            RgbdState &h = hs[i0 + k];
            memset(&h, 0, sizeof(h));
            memcpy(h.icp.T, p.T_init, sizeof(h.icp.T));
            h.icp.scale = p.scale_src;
        }
        TL3D_HIP(hipMemcpyAsync(b.pairs, hp.data(), m * sizeof(RgbdPair), hipMemcpyHostToDevice, ctx->stream));
        TL3D_HIP(hipMemcpyAsync(b.states, &hs[i0], m * sizeof(RgbdState), hipMemcpyHostToDevice, ctx->stream));
        for (int l = 0; l < n_levels && !rc; ++l) {
            const tl3d_icp_params &p = levels[l].icp;
            for (int it = 0; it <= (eval ? 0 : p.iters) && !rc; ++it) {
                const StepKind fin = step_kind(it, p.iters, l == n_levels - 1, eval);
                rc = launch_rgbd_pass(ctx->stream, ctx->cam, b.pairs, (int)m, lv[l], b.states, fin, b.slab);
                if (!rc) rc = launch_rgbd_step(ctx->stream, b.slab, (int)m, lv[l].members, b.states, levels[l].photo_weight, p.damping, p.eps, p.eig_rel, fin);
            }
        }
        if (rc) return rc;
        TL3D_HIP(hipMemcpyAsync(&hs[i0], b.states, m * sizeof(RgbdState), hipMemcpyDeviceToHost, ctx->stream));
        TL3D_HIP(hipStreamSynchronize(ctx->stream));
    }
    return TL3D_OK;
}

int tl3d_rgbd_evaluate_pairs(tl3d_ctx *ctx, const tl3d_icp_pair *pairs, int n_pairs, int stride, double max_dist, double photo_gate,
                             tl3d_rgbd_eval *out) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(n_pairs >= 0, TL3D_E_INVALID, "n_pairs %d is negative", n_pairs);
    tl3d_rgbd_level lv;
    memset(&lv, 0, sizeof(lv));
    lv.icp.stride = stride;
    lv.icp.max_dist = max_dist;
    lv.photo_gate = photo_gate;
    int rc = check_level(lv.icp, LV_FINITE_GATE);
    if (rc) return rc;
    REQUIRE(photo_gate > 0, TL3D_E_INVALID, "photo_gate must be positive");
    REQUIRE(n_pairs == 0 || (pairs && out), TL3D_E_INVALID, "null argument");
    REQUIRE(!ctx->icp_batch.busy, TL3D_E_STATE, "an ICP batch is still uncollected");
    rc = rgbd_check_pairs(ctx, pairs, n_pairs);
    if (rc) return rc;
    if (n_pairs == 0) return TL3D_OK;
    std::vector<RgbdState> hs;
    rc = rgbd_run(ctx, pairs, n_pairs, &lv, 1, true, hs);
    if (rc) return rc;
    for (int i = 0; i < n_pairs; ++i) {
        read_eval(hs[i].icp.sums, &out[i].geo);
        memcpy(out[i].A_p, hs[i].photo, 21 * sizeof(double));
        memcpy(out[i].b_p, hs[i].photo + 21, 6 * sizeof(double));
        out[i].e_p = hs[i].photo[RGBD_SUM_E_P - 32];
        out[i].n_photo = (int64_t)hs[i].photo[RGBD_SUM_PHOTO - 32];
        out[i].n_qualified = (int64_t)hs[i].icp.sums[RGBD_SUM_ELIG];
    }
    return TL3D_OK;
}

int tl3d_rgbd_register_pairs(tl3d_ctx *ctx, const tl3d_icp_pair *pairs, int n_pairs, const tl3d_rgbd_level *levels, int n_levels,
                             tl3d_icp_result *out, tl3d_rgbd_info *info) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(n_pairs >= 0, TL3D_E_INVALID, "n_pairs %d is negative", n_pairs);
    REQUIRE(n_levels >= 1 && n_levels <= TL3D_ICP_MAX_LEVELS, TL3D_E_INVALID, "n_levels %d outside [1,%d]", n_levels, TL3D_ICP_MAX_LEVELS);
    REQUIRE(levels != nullptr, TL3D_E_INVALID, "null argument");
    for (int l = 0; l < n_levels; ++l) {
        REQUIRE(!levels[l].icp.estimate_scale, TL3D_E_INVALID, "the joint registration does not estimate the scale (estimate_scale must be 0)");
        const int rc = check_level(levels[l].icp, LV_FINITE_GATE);
        if (rc) return rc;
        REQUIRE(levels[l].photo_gate > 0, TL3D_E_INVALID, "photo_gate must be positive");
        REQUIRE(levels[l].photo_weight >= 0, TL3D_E_INVALID, "photo_weight must not be negative");
    }
    REQUIRE(n_pairs == 0 || (pairs && out), TL3D_E_INVALID, "null argument");
    REQUIRE(!ctx->icp_batch.busy, TL3D_E_STATE, "an ICP batch is still uncollected");
    int rc = rgbd_check_pairs(ctx, pairs, n_pairs);
    if (rc) return rc;
    if (n_pairs == 0) return TL3D_OK;
    std::vector<RgbdState> hs;
    rc = rgbd_run(ctx, pairs, n_pairs, levels, n_levels, false, hs);
    if (rc) return rc;
    for (int i = 0; i < n_pairs; ++i) {
        read_result(hs[i].icp, &out[i]);
        if (info) {
            const double e_p = hs[i].photo[RGBD_SUM_E_P - 32], n_photo = hs[i].photo[RGBD_SUM_PHOTO - 32];
            info[i].photo_rmse = n_photo > 0 ? sqrt(e_p / n_photo) : 0.0;
            info[i].n_photo = (int64_t)n_photo;
            info[i].n_qualified = (int64_t)hs[i].icp.sums[RGBD_SUM_ELIG];
        }
    }
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- registration of two point clouds
// what both cloud calls check before any device work
static int cloud_check(tl3d_ctx *ctx, const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const double T[16], double scale) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(n_src >= 0 && (n_src == 0 || src), TL3D_E_INVALID, "bad source list");
    REQUIRE(n_tgt >= 0 && (n_tgt == 0 || tgt), TL3D_E_INVALID, "bad target list");
    REQUIRE(n_tgt < (1ll << 31) && n_src < (1ll << 31), TL3D_E_INVALID, "n_src %lld, n_tgt %lld: indices need fewer than 2^31 points of each",
            (long long)n_src, (long long)n_tgt);
    REQUIRE(T != nullptr, TL3D_E_INVALID, "null pose");
    for (int i = 0; i < 16; ++i) REQUIRE(isfinite(T[i]), TL3D_E_INVALID, "the pose has a non-finite entry");
    REQUIRE(isfinite(scale), TL3D_E_INVALID, "the scale is not finite");
    return TL3D_OK;
}

// the buffers, the initial state on its way to the device, the staged arrays, the run and the one read-back: *ctx->cloud.host holds the result
static int cloud_run(tl3d_ctx *ctx, const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const float *nrm, const double T[16],
                     double scale, const tl3d_icp_params *levels, int n_levels, bool evaluate, double cell, int32_t *index_out) {
    REQUIRE(!ctx->icp_batch.busy, TL3D_E_STATE, "an ICP batch is still uncollected");
    TL3D_HIP(hipSetDevice(ctx->device));
    tl3d_ctx::Cloud &cl = ctx->cloud;
    if (!cl.state) {                                        // all or nothing, as icp_lane_init
        bool ok = hipMalloc(&cl.state, sizeof(IcpState)) == hipSuccess;
        ok = ok && hipHostMalloc(&cl.host, sizeof(IcpState), hipHostMallocDefault) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            cloud_free(cl);
            return set_err(TL3D_E_NOMEM, "cloud registration: buffer allocation failed");
        }
    }
    IcpState *h = cl.host;
    memset(h, 0, sizeof(*h));
    memcpy(h->T, T, sizeof(h->T));
    h->T[12] = h->T[13] = h->T[14] = 0.0;
    h->T[15] = 1.0;
    h->scale = scale;
    Staging st(ctx);
    const float *ds, *dt, *dn = nullptr;
    int32_t *di = nullptr;
    int rc = st.in(src, (size_t)n_src * 12, &ds);
    if (!rc) rc = st.in(tgt, (size_t)n_tgt * 12, &dt);
    if (!rc && nrm) rc = st.in(nrm, (size_t)n_tgt * 12, &dn);
    if (!rc && index_out) rc = st.out(index_out, (size_t)n_src * sizeof(int32_t), &di);
    if (rc) return rc;
    TL3D_HIP(hipMemcpyAsync(cl.state, h, sizeof(IcpState), hipMemcpyHostToDevice, ctx->stream));
    rc = cloud_icp_run(ctx, ds, n_src, dt, n_tgt, dn, levels, n_levels, evaluate, cell, cl.state, di);
    if (!rc && hipMemcpyAsync(h, cl.state, sizeof(IcpState), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = set_err(TL3D_E_HIP, "cloud registration: state read-back failed");
    return st.finish(rc, true);
}

int tl3d_cloud_evaluate(tl3d_ctx *ctx, const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const float *tgt_normals,
                        const double T[16], double scale, int stride, double max_dist, double cell_size, int with_scale,
                        tl3d_cloud_eval *out, int32_t *index_out) {
    int rc = cloud_check(ctx, src, n_src, tgt, n_tgt, T, scale);
    if (rc) return rc;
    REQUIRE(out != nullptr, TL3D_E_INVALID, "null argument");
    REQUIRE(stride >= 1, TL3D_E_INVALID, "stride must be >= 1");
    REQUIRE(!(max_dist != max_dist), TL3D_E_INVALID, "max_dist is not a number");
    REQUIRE(!ranges_overlap(index_out, (size_t)n_src * 4, src, (size_t)n_src * 12) && !ranges_overlap(index_out, (size_t)n_src * 4, tgt, (size_t)n_tgt * 12) &&
                !ranges_overlap(index_out, (size_t)n_src * 4, tgt_normals, (size_t)n_tgt * 12),
            TL3D_E_INVALID, "the output aliases an input");
    tl3d_icp_params lv;
    memset(&lv, 0, sizeof(lv));
    lv.stride = stride;
    lv.max_dist = max_dist;
    lv.estimate_scale = with_scale ? 1 : 0;
    if (n_src == 0 || n_tgt == 0) {                         // nothing to search: zero sums, every index -1
        REQUIRE(!ctx->icp_batch.busy, TL3D_E_STATE, "an ICP batch is still uncollected");
        if (index_out && n_src) {
            TL3D_HIP(hipSetDevice(ctx->device));
            Staging st(ctx);
            int32_t *di = nullptr;
            rc = st.out(index_out, (size_t)n_src * sizeof(int32_t), &di);
            if (rc) return rc;
            TL3D_HIP(hipMemsetAsync(di, 0xff, (size_t)n_src * sizeof(int32_t), ctx->stream));
            rc = st.finish(TL3D_OK, true);
            if (rc) return rc;
        }
        memset(out, 0, sizeof(*out));
        out->n_src = (n_src + stride - 1) / stride;
        return TL3D_OK;
    }
    rc = cloud_run(ctx, src, n_src, tgt, n_tgt, tgt_normals, T, scale, &lv, 1, true, cell_size, index_out);
    if (rc) return rc;
    const double *s = ctx->cloud.host->sums;
    int m = 0, k = 0;
    for (int i = 0; i < 6; ++i) {
        for (int j = i; j < 6; ++j) out->A[k++] = s[m++];
        out->A[k++] = s[32 + i];
    }
    out->A[k] = s[38];
    memcpy(out->b, s + 21, 6 * sizeof(double));
    out->b[6] = s[39];
    out->e = s[ICP_SUM_E];
    out->n_corr = (int64_t)s[ICP_SUM_CORR];
    out->n_src = (int64_t)s[ICP_SUM_SRC];
    out->n_no_normal = (int64_t)s[CLOUD_SUM_NO_NORMAL];
    return TL3D_OK;
}

int tl3d_cloud_register(tl3d_ctx *ctx, const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const float *tgt_normals,
                        const double T_init[16], double scale_init, const tl3d_icp_params *levels, int n_levels, double cell_size,
                        tl3d_icp_result *out) {
    int rc = cloud_check(ctx, src, n_src, tgt, n_tgt, T_init, scale_init);
    if (rc) return rc;
    REQUIRE(out != nullptr, TL3D_E_INVALID, "null argument");
    REQUIRE(n_levels >= 1 && n_levels <= TL3D_ICP_MAX_LEVELS, TL3D_E_INVALID, "n_levels %d outside [1,%d]", n_levels, TL3D_ICP_MAX_LEVELS);
    REQUIRE(levels != nullptr, TL3D_E_INVALID, "null argument");
    for (int l = 0; l < n_levels && !rc; ++l) rc = check_level(levels[l], 0);
    if (rc) return rc;
    if (n_src == 0 || n_tgt == 0) {                         // nothing to register: the run fails at its first pass
        REQUIRE(!ctx->icp_batch.busy, TL3D_E_STATE, "an ICP batch is still uncollected");
        memset(out, 0, sizeof(*out));
        memcpy(out->T, T_init, sizeof(out->T));
        out->T[12] = out->T[13] = out->T[14] = 0.0;
        out->T[15] = 1.0;
        out->scale = scale_init;
        out->n_src = (n_src + levels[0].stride - 1) / levels[0].stride;
        out->status = 2;
        return TL3D_OK;
    }
    rc = cloud_run(ctx, src, n_src, tgt, n_tgt, tgt_normals, T_init, scale_init, levels, n_levels, false, cell_size, nullptr);
    if (rc) return rc;
    read_result(*ctx->cloud.host, out);
    return TL3D_OK;
}

// ------------------------------------------------------------------------------------------- global registration
int tl3d_cloud_voxel_subsample(tl3d_ctx *ctx, const float *xyz, int64_t n, double voxel, int32_t *index_out, int64_t *out_n) {
    REQUIRE(ctx && index_out && out_n, TL3D_E_INVALID, "null argument");
    REQUIRE(n >= 0 && n < (1ll << 31) && (n == 0 || xyz), TL3D_E_INVALID, "bad point list (0 <= n < 2^31)");
    REQUIRE(isfinite(voxel) && voxel > 0, TL3D_E_INVALID, "voxel must be finite and positive");
    REQUIRE(!ranges_overlap(index_out, (size_t)n * 4, xyz, (size_t)n * 12), TL3D_E_INVALID, "the output aliases the input");
    if (n == 0) {
        *out_n = 0;
        return TL3D_OK;
    }
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *dx;
    int32_t *di;
    int rc = st.in(xyz, (size_t)n * 12, &dx);
    if (!rc) rc = st.out(index_out, (size_t)n * 4, &di);
    if (rc) return rc;
    long long kept = 0;
    rc = voxel_subsample_run(ctx, dx, n, voxel, kt_slots((size_t)n), di, &kept);
    if (rc) return rc;                                      // (a refusal leaves the caller's array and *out_n as they were)
    if (di != index_out) {                                  // a host output: the kept prefix alone goes back
        TL3D_HIP(hipMemcpyAsync(index_out, di, (size_t)kept * 4, hipMemcpyDeviceToHost, ctx->stream));
        TL3D_HIP(hipStreamSynchronize(ctx->stream));
    }
    *out_n = kept;
    return TL3D_OK;
}

int tl3d_cloud_fpfh(tl3d_ctx *ctx, const float *xyz, const float *normals, int64_t n, int nb_neighbors, double max_radius, double cell_size,
                    float *fpfh_out, int32_t *spfh_out) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(n >= 0 && n < (1ll << 31), TL3D_E_INVALID, "n %lld: indices need 0 <= n < 2^31", (long long)n);
    REQUIRE(n == 0 || (xyz && normals && fpfh_out), TL3D_E_INVALID, "null argument");
    REQUIRE(nb_neighbors >= 4 && nb_neighbors <= 64, TL3D_E_INVALID, "nb_neighbors must be in [4,64]");
    REQUIRE(cell_size > 0 && isfinite(cell_size), TL3D_E_INVALID, "cell_size must be positive");
    REQUIRE(!(max_radius != max_radius), TL3D_E_INVALID, "max_radius is not a number");
    const size_t nb_x = (size_t)n * 12, nb_f = (size_t)n * 33 * 4, nb_s = (size_t)n * 34 * 4;
    const void *ins[2] = {xyz, normals};
    for (int i = 0; i < 2; ++i)
        REQUIRE(!ranges_overlap(fpfh_out, nb_f, ins[i], nb_x) && !ranges_overlap(spfh_out, nb_s, ins[i], nb_x), TL3D_E_INVALID, "an output aliases an input");
    REQUIRE(!ranges_overlap(fpfh_out, nb_f, spfh_out, nb_s), TL3D_E_INVALID, "the outputs alias each other");
    if (n == 0) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *dx, *dn;
    float *df;
    int32_t *dsp = nullptr;
    int rc = st.in(xyz, nb_x, &dx);
    if (!rc) rc = st.in(normals, nb_x, &dn);
    if (!rc) rc = st.out(fpfh_out, nb_f, &df);
    if (!rc && spfh_out) rc = st.out(spfh_out, nb_s, &dsp);
    if (rc) return rc;
    return st.finish(fpfh_run(ctx, dx, dn, n, nb_neighbors, max_radius, cell_size, df, dsp), true);
}

int tl3d_feature_match(tl3d_ctx *ctx, const float *feat_a, int64_t n_a, const float *feat_b, int64_t n_b, int dim, int32_t *index_out,
                       double *dist2_out) {
    REQUIRE(ctx != nullptr, TL3D_E_INVALID, "null ctx");
    REQUIRE(n_a >= 0 && n_b >= 0 && n_a < (1ll << 31) && n_b < (1ll << 31), TL3D_E_INVALID, "n_a %lld, n_b %lld: sizes must be in [0, 2^31)",
            (long long)n_a, (long long)n_b);
    REQUIRE((n_a == 0 || feat_a) && (n_b == 0 || feat_b), TL3D_E_INVALID, "null feature array");
    REQUIRE(dim >= 1 && dim <= 64, TL3D_E_INVALID, "dim must be in [1,64]");
    REQUIRE(n_a == 0 || n_b <= (1ll << 34) / n_a, TL3D_E_INVALID,
            "n_a %lld x n_b %lld exceeds 2^34 feature pairs: the match is brute force, subsample the clouds first", (long long)n_a, (long long)n_b);
    const size_t nb_a = (size_t)n_a * dim * 4, nb_b = (size_t)n_b * dim * 4, nb_i = (size_t)n_a * 4, nb_d = (size_t)n_a * 8;
    REQUIRE(!ranges_overlap(index_out, nb_i, feat_a, nb_a) && !ranges_overlap(index_out, nb_i, feat_b, nb_b) &&
                !ranges_overlap(dist2_out, nb_d, feat_a, nb_a) && !ranges_overlap(dist2_out, nb_d, feat_b, nb_b),
            TL3D_E_INVALID, "an output aliases an input");
    REQUIRE(!ranges_overlap(index_out, nb_i, dist2_out, nb_d), TL3D_E_INVALID, "the outputs alias each other");
    if (n_a == 0 || (!index_out && !dist2_out)) return TL3D_OK;
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *da, *db = nullptr;
    int32_t *di = nullptr;
    double *dd = nullptr;
    int rc = st.in(feat_a, nb_a, &da);
    if (!rc && n_b) rc = st.in(feat_b, nb_b, &db);
    if (!rc && index_out) rc = st.out(index_out, nb_i, &di);
    if (!rc && dist2_out) rc = st.out(dist2_out, nb_d, &dd);
    if (rc) return rc;
    return st.finish(feature_match_run(ctx, da, n_a, db, n_b, dim, di, dd), true);
}

int tl3d_cloud_ransac(tl3d_ctx *ctx, const float *src, int64_t n_src, const float *tgt, int64_t n_tgt, const int32_t *corr, int64_t m,
                      const tl3d_ransac_params *params, tl3d_ransac_result *out, int32_t *count_out) {
    REQUIRE(ctx && params && out, TL3D_E_INVALID, "null argument");
    REQUIRE(n_src >= 0 && (n_src == 0 || src), TL3D_E_INVALID, "bad source list");
    REQUIRE(n_tgt >= 0 && (n_tgt == 0 || tgt), TL3D_E_INVALID, "bad target list");
    REQUIRE(m >= 0 && (m == 0 || corr), TL3D_E_INVALID, "bad correspondence list");
    REQUIRE(m == 0 || (n_src > 0 && n_tgt > 0), TL3D_E_INVALID, "correspondences into an empty cloud");
    REQUIRE(n_src < (1ll << 31) && n_tgt < (1ll << 31) && m < (1ll << 31), TL3D_E_INVALID, "n_src %lld, n_tgt %lld, m %lld: sizes must stay below 2^31",
            (long long)n_src, (long long)n_tgt, (long long)m);
    const int64_t H = params->n_hypotheses;
    REQUIRE(H >= 1 && H <= (1ll << 24), TL3D_E_INVALID, "n_hypotheses must be in [1, 2^24]");
    REQUIRE(isfinite(params->max_dist) && params->max_dist > 0, TL3D_E_INVALID, "max_dist must be finite and positive");
    REQUIRE(params->edge_ratio >= 0 && params->edge_ratio <= 1, TL3D_E_INVALID, "edge_ratio must be in [0,1]");
    REQUIRE(params->reserved == 0, TL3D_E_INVALID, "reserved must be 0");
    const size_t nb_c = (size_t)H * 4;
    REQUIRE(!ranges_overlap(count_out, nb_c, src, (size_t)n_src * 12) && !ranges_overlap(count_out, nb_c, tgt, (size_t)n_tgt * 12) &&
                !ranges_overlap(count_out, nb_c, corr, (size_t)m * 8),
            TL3D_E_INVALID, "the output aliases an input");
    if (m == 0) {                                           // nothing to draw from
        if (count_out) {
            TL3D_HIP(hipSetDevice(ctx->device));
            Staging st(ctx);
            int32_t *dc = nullptr;
            int rc = st.out(count_out, nb_c, &dc);
            if (rc) return rc;
            TL3D_HIP(hipMemsetAsync(dc, 0xff, nb_c, ctx->stream));
            rc = st.finish(TL3D_OK, true);
            if (rc) return rc;
        }
        memset(out, 0, sizeof(*out));
        out->T[0] = out->T[5] = out->T[10] = out->T[15] = 1.0;
        out->best_h = -1;
        out->status = 2;
        return TL3D_OK;
    }
    TL3D_HIP(hipSetDevice(ctx->device));
    Staging st(ctx);
    const float *ds, *dt;
    const int32_t *dcorr;
    int32_t *dc = nullptr;
    int rc = st.in(src, (size_t)n_src * 12, &ds);
    if (!rc) rc = st.in(tgt, (size_t)n_tgt * 12, &dt);
    if (!rc) rc = st.in(corr, (size_t)m * 8, &dcorr);
    if (!rc && count_out) rc = st.out(count_out, nb_c, &dc);
    if (rc) return rc;
    tl3d_ransac_result res;
    memset(&res, 0, sizeof(res));
    rc = st.finish(ransac_run(ctx, ds, n_src, dt, n_tgt, dcorr, m, *params, &res, dc), true);
    if (rc) return rc;
    *out = res;
    return TL3D_OK;
}

}  // extern "C"
