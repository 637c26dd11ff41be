// kernels_icp.hip -- row a10: vertex/normal map and pairwise point-to-plane ICP (projective association).
// The reference has no ICP (its poses come from SIFT + essential matrix, depth_to_reconstruction.py:144-215);
// this replaces that pose source and returns the relative pose in the reference's chaining convention
// (D2R:618-620).  Convention and f32 sequence = oracle/tl3d_oracle.c (orc_normals, icp_pass, solve6, se3_apply).
//
// Device-resident iteration, ONE launch per iteration (icp_iter_kernel): every workgroup accumulates the 6x6 normal
// equations (21 + 6 + 3 sums, fp64) per lane, reduces them with 64-lane wave shuffles, then across its 4 waves through
// LDS, and publishes one 32-double partial (write-through stores, drained, then an agent-scope ticket).  The workgroup whose
// ticket is the last one sums the partials in block order (deterministic), solves the damped system by a 6x6 Jacobi
// eigen-decomposition (unobservable directions dropped), updates T in device memory and re-arms the ticket.  A dependent
// two-kernel chain (reduce, then a one-workgroup solve) cost a second launch boundary and a second ramp per iteration:
// 38 us -> see DESIGN.md section 7.  No host round trip inside the loop: the host replays one captured hipGraph per run
// ((iters+1) kernels + the state copies) and reads the state once.  Bytes per iteration and sampled pixel: 4 (source
// depth) + 16 (target normal+depth gather) = 20 B.
//
// Batched form (icp_batch_kernel, tl3d_icp_batch_*): many pairs, each through all its coarse-to-fine levels and all its
// iterations, in ONE persistent launch; the workgroups that share a pair meet at a per-pair barrier in device memory after every
// pass, and every workgroup works on two (pair, member) slots in turn.  Same accumulate / solve code as the per-iteration
// kernel; what the pipeline uses.
// Maps: normal maps and window-averaged depth live in PHASE-MAJOR ROWS (tl3d_internal.h: pm_index); a raw frame is row-major.
#include "tl3d_internal.h"
#include "icp_sample.h"
#include "reg_solve.h"

namespace tl3d {

// PM: `depth` is kept in phase-major rows (pm_index, tl3d_internal.h: the window-averaged depth), else row-major (the frame itself)
template <bool PM>
__device__ __forceinline__ bool load_vertex(const Cam &cam, const float *__restrict__ depth, int u, int v, float sc,
                                            float mind, float maxd, float p[3]) {
    const float d = depth[PM ? pm_index(u, v, pm_w4(cam.W)) : (size_t)v * cam.W + u] * sc;
    if (!(d > mind && d < maxd)) return false;
    p[0] = (((float)u - cam.cx) / cam.fx) * d;
    p[1] = (((float)v - cam.cy) / cam.fy) * d;
    p[2] = d;
    return true;
}

// Noise-robust normals, first half (oracle: orc_normals_smooth): the depth averaged over the (2 radius + 1)^2 window of every pixel
// -- over the pixels that are valid and within `jump` of the centre pixel, summed in row-major order in f32 (the oracle's order);
// out stays in the units of `depth`, 0 = invalid centre.  1 mm of depth noise turns central differences over one pixel (0.6 mm
// apart at 1 m, f = 1719) into noise; normals_kernel then takes its tangent vectors `radius` pixels to either side of this map.
__global__ __launch_bounds__(256) void smooth_depth_kernel(Cam cam, const float *__restrict__ depth, float sc, float mind, float maxd, float jump,
                                                           int radius, float *__restrict__ out) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u >= cam.W || v >= cam.H) return;
    const float d0 = depth[(size_t)v * cam.W + u] * sc;
    float res = 0.0f;
    if (d0 > mind && d0 < maxd) {
        // mean of the INVERSE depth (linear in the pixel coordinates on a plane, however oblique: a plain mean of the depth is
        // biased on a floor seen at a grazing angle, 0.06 mm per frame of drift on config 4) over the centre and the pixel PAIRS
        // (u + du, v + dv), (u - du, v - dv) that are both in the image, valid and within the jump of the centre -- a symmetric
        // set: the mean of a linear function over it is its centre value, at the edge of a surface too.  The oracle's order.
        float sum = 1.0f / depth[(size_t)v * cam.W + u];
        int n = 1;
        for (int dv = 0; dv <= radius; ++dv)
            for (int du = (dv == 0 ? 1 : -radius); du <= radius; ++du) {
                const int ua = u + du, va = v + dv, ub = u - du, vb = v - dv;
                if (ua < 0 || ua >= cam.W || va < 0 || va >= cam.H || ub < 0 || ub >= cam.W || vb < 0 || vb >= cam.H) continue;
                const float ra = depth[(size_t)va * cam.W + ua], rb = depth[(size_t)vb * cam.W + ub];
                const float da = ra * sc, db = rb * sc;
                if (!(da > mind && da < maxd) || !(db > mind && db < maxd)) continue;
                if (!(fabsf(da - d0) <= jump) || !(fabsf(db - d0) <= jump)) continue;
                sum += 1.0f / ra;
                sum += 1.0f / rb;
                n += 2;
            }
        res = (float)n / sum;
    }
    out[pm_index(u, v, pm_w4(cam.W))] = res;              // phase-major rows: what the registration samples at its stride
}

// step: the tangent vectors come from the pixels `step` to either side (1: plain central differences).  The map is written in
// phase-major rows.
template <bool PM>
__global__ __launch_bounds__(256) void normals_kernel(Cam cam, const float *__restrict__ depth, float sc, float mind,
                                                      float maxd, float jump, int step, float4 *__restrict__ nmap) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u >= cam.W || v >= cam.H) return;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    float p[3], l[3], r[3], up[3], dn[3];
    bool ok = (u >= step && v >= step && u <= cam.W - 1 - step && v <= cam.H - 1 - step);
    ok = ok && load_vertex<PM>(cam, depth, u, v, sc, mind, maxd, p);
    ok = ok && load_vertex<PM>(cam, depth, u - step, v, sc, mind, maxd, l);
    ok = ok && load_vertex<PM>(cam, depth, u + step, v, sc, mind, maxd, r);
    ok = ok && load_vertex<PM>(cam, depth, u, v - step, sc, mind, maxd, up);
    ok = ok && load_vertex<PM>(cam, depth, u, v + step, sc, mind, maxd, dn);
    if (ok) {
        ok = fabsf(l[2] - p[2]) <= jump && fabsf(r[2] - p[2]) <= jump && fabsf(up[2] - p[2]) <= jump &&
             fabsf(dn[2] - p[2]) <= jump;
    }
    if (ok) {
        const float ax = r[0] - l[0], ay = r[1] - l[1], az = r[2] - l[2];
        const float bx = dn[0] - up[0], by = dn[1] - up[1], bz = dn[2] - up[2];
        float nx = fmaf(ay, bz, -(az * by));
        float ny = fmaf(az, bx, -(ax * bz));
        float nz = fmaf(ax, by, -(ay * bx));
        const float len2 = fmaf(nx, nx, fmaf(ny, ny, nz * nz));
        if (len2 > 1e-30f) {
            const float inv = 1.0f / sqrtf(len2);
            nx *= inv; ny *= inv; nz *= inv;
            const float dotv = fmaf(nx, p[0], fmaf(ny, p[1], nz * p[2]));
            if (dotv > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
            o = make_float4(nx, ny, nz, p[2]);
        }
    }
    nmap[pm_index(u, v, pm_w4(cam.W))] = o;
}

// icp_accumulate_core -- a workgroup's share of one pass, sample arithmetic and reduction -- lives in icp_sample.h (shared with
// kernels_icp_eval.hip)

__device__ __forceinline__ void icp_accumulate(const Cam &cam, const IcpRun *__restrict__ run, const IcpState *state,
                                               double (*sm)[ICP_SLAB], double *__restrict__ sm_out) {
    float r[9], t[3];
    r[0] = (float)state->T[0]; r[1] = (float)state->T[1]; r[2] = (float)state->T[2];  t[0] = (float)state->T[3];
    r[3] = (float)state->T[4]; r[4] = (float)state->T[5]; r[5] = (float)state->T[6];  t[1] = (float)state->T[7];
    r[6] = (float)state->T[8]; r[7] = (float)state->T[9]; r[8] = (float)state->T[10]; t[2] = (float)state->T[11];
    const float sc = (float)state->scale;                  // the caller's scale, or the running estimate of a Sim(3) run
    if (run->est_scale)
        icp_accumulate_core<true, false>(cam, run->depth_src, run->nmap_tgt, sc, run->mind, run->maxd, run->md2, run->stride, run->Ws, run->Hs,
                                  r, t, (int)blockIdx.x, (int)gridDim.x, run->src_pm, sm, sm_out);
    else
        icp_accumulate_core<false, false>(cam, run->depth_src, run->nmap_tgt, sc, run->mind, run->maxd, run->md2, run->stride, run->Ws, run->Hs,
                                   r, t, (int)blockIdx.x, (int)gridDim.x, run->src_pm, sm, sm_out);
}

// The last workgroup's part: fixed-order sum of the published partials, solve (reg_solve.h), pose update.
// Returns (thread 0 only) 1 when the run converged, 2 when it failed in this pass, else 0.  T_f32: where thread 0 leaves the
// new pose as the 12 floats a pass uses (LDS; untouched when the pose did not change).
__device__ __forceinline__ int icp_finish(const double *slab, int nblocks, IcpState *state, double damping, double eps, double eig_rel,
                                          int final_pass, double (*part)[ICP_SLAB], double *sums, int est_scale, float *T_f32 = nullptr,
                                          int updates_so_far = -1) {
    const int t = threadIdx.x;
    {   // slab reduction: 8 groups x 32 components, loads batched 8 deep, combined in a fixed order (deterministic).
        // The partials were written by other CUs in THIS launch: agent-scope (sc1) loads, never served from this CU's L1
        const int comp = t & 31, grp = t >> 5;
        double s = 0.0;
        int b = grp;
        for (; b + 56 < nblocks; b += 64) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = __hip_atomic_load(slab + (size_t)(b + 8 * k) * ICP_SLAB + comp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[k];
        }
        for (; b < nblocks; b += 8) s += __hip_atomic_load(slab + (size_t)b * ICP_SLAB + comp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        part[grp][comp] = s;
    }
    if (est_scale && t < 8) {                              // the scale column's 8 sums: member order, one thread each
        double s = 0.0;
        for (int b = 0; b < nblocks; ++b) s += __hip_atomic_load(slab + (size_t)b * ICP_SLAB + 32 + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sums[32 + t] = s;
        st_agent(&state->sums[32 + t], s);                 // write-through, as every state word: see the note at sums[t] below
    }
    __syncthreads();
    if (t < 32) {
        double s = part[0][t];
#pragma unroll
        for (int g = 1; g < 8; ++g) s += part[g][t];
        sums[t] = s;
        // WRITE-THROUGH (agent scope), not a plain store: in a batched launch the sums of consecutive passes of one pair are written
        // by different workgroups, i.e. from different XCDs, and a plain store sits in its XCD's L2 until that writes it back --
        // the line of pass n - 1 could reach memory AFTER the line of the final pass (both flushed at the end of the launch, in no
        // order): the statistics the host read (rmse, fitness, correspondences) were then those of the last-but-one pose.  Seen as
        // run-to-run differences of rmse / n_corr of the LAST pairs of a batch with bit-identical poses (tools/bench_icp.py, round 4);
        // the pose words have always been written through.
        st_agent(&state->sums[t], s);
    }
    __syncthreads();
    if (final_pass || t >= 64) return 0;                   // wave 0 solves
    double x[7];
    x[6] = 0.0;
    int fail = 0;
    if (est_scale) {                                       // Sim(3): the 7x7 system, on one lane (wave-uniform branch)
        if (t == 0) fail = (sums[28] < 6.0) ? 1 : solve7_serial(sums, damping, eig_rel, x);
    } else {
        fail = (sums[28] < 6.0) ? 1 : solve6_wave(sums, sums + 21, damping, eig_rel, x);
    }
    if (t != 0) return 0;
    if (fail) {
        st_agent(&state->done, 1);
        st_agent(&state->status, 2);
        return 2;
    }
    se3_apply(x, state->T, T_f32);
    if (est_scale) {
        const double sn = ld_agent(&state->scale) * exp(x[6]);
        st_agent(&state->scale, sn);
        if (T_f32) T_f32[12] = (float)sn;
    }
    st_agent(&state->iters_run, (updates_so_far >= 0 ? updates_so_far : ld_agent(&state->iters_run)) + 1);    // (the load is a round trip)
    double mx = 0.0;
    for (int i = 0; i < (est_scale ? 7 : 6); ++i) mx = fmax(mx, fabs(x[i]));
    if (mx < eps) {
        st_agent(&state->done, 1);
        st_agent(&state->status, 1);
        return 1;
    }
    return 0;
}

// One ICP iteration in one launch.  Hand-off between workgroups inside the launch (MI355X guide, Guideline 16 / the
// split-K "arrival ticket, last arriver combines" form): partial = 8-byte agent-scope (write-through) stores, the storing
// wave drains them, the workgroup's barrier, ONE lane takes an agent-scope ticket; the workgroup whose ticket is the last
// one acquires (one lane, then wait + barrier) and reads every partial with agent-scope loads.  Nothing depends on
// dispatch order or placement; every workgroup takes exactly one ticket per launch, so the grid always drains.
__global__ __launch_bounds__(256) void icp_iter_kernel(Cam cam, const IcpRun *__restrict__ run, IcpState *state, int final_pass,
                                                       double *slab, unsigned *ticket) {
    if (!final_pass && state->done) return;                // set by an EARLIER launch only: uniform over the grid
    __shared__ double sm[8][ICP_SLAB];
    __shared__ double tot[ICP_SLAB];
    __shared__ int s_last;
    icp_accumulate(cam, run, state, sm, tot);
    if (threadIdx.x < ICP_SLAB) {
        __hip_atomic_store(slab + (size_t)blockIdx.x * ICP_SLAB + threadIdx.x, tot[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the storing wave drains before anyone signals for it
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (tk == gridDim.x - 1u);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    (void)icp_finish(slab, (int)gridDim.x, state, run->damping, run->eps, run->eig_rel, final_pass, sm, tot, final_pass ? 0 : run->est_scale);
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // re-arm for the next launch
}

// A batch of registrations, each through all its levels and iterations, in ONE launch.  `members` workgroups share a
// pair; after every pass they meet at the pair's barrier in device memory: partial sums as agent-scope stores (drained),
// one arrival ticket per workgroup; the last arriver acquires, sums the partials in member order, solves, updates the
// pose (write-through stores, drained) and publishes the pair's 64-B generation line: words 1..12 = the new pose as the
// twelve floats the next pass uses, then word 0 = pass count + the done / over / failed flags.  The others poll that line with ONE
// wave instruction (13 lanes, one 64-B request) that returns the flags and the pose together: no fence and no load on
// the waiting side.  Publishing and polling are read-modify-write atomics, which execute at the memory side: polls by
// agent-scope (sc1) LOADS were seen to return a word their XCD had cached before the store for seconds (88 of 113
// members of a pair stuck, the 25 on the publisher's XCD gone ahead), whatever the allocation flags.  Short sleeps between
// polls: polls of one line from a hundred CUs at full rate saturate its channel and starve the arrivals.
// Arrival counter and generation line of a pair are different lines; consecutive pairs' lines are > 4 KB apart.
// Waiting needs the pair's other workgroups to be running.  The launch is therefore PERSISTENT: at most as many workgroups as
// the chip holds at once, each taking (pair, member) TICKETS in a loop -- one when it starts, the next when its pair is through
// all its passes.  The tickets handed out at any moment form a window of consecutive (pair, member) slots held by running
// workgroups: every pair that lies wholly inside the window completes, its workgroups come back for tickets, and the pair at
// the window's upper end gets its missing members from them (members <= 32 against >= 256 running workgroups: the grid is
// what the occupancy query says the chip holds, never less than one workgroup per CU).  Nothing
// depends on WHEN the hardware starts a workgroup.  (Until round 3 the grid was one workgroup per slot, tickets taken at
// the start: the last pair of a 128-pair batch of 720p frames then waited for the grid's last two or three workgroups, which
// the dispatcher now and then -- one batch in eight -- started seconds late: the in-kernel time-out of config 4.)
// Every wait is bounded in time; a time-out raises the error word and ends the launch.
constexpr unsigned long long ICP_WAIT_LIMIT_TICKS = 200000000ull;          // 2 s of the 100 MHz wall clock
__device__ __forceinline__ size_t icp_sync_line(int pair, int rows) {        // 16-word line of `pair`: neighbours are rows*64 B (> 4 KB) apart
    return ((size_t)(pair & 63) * (size_t)rows + (size_t)(pair >> 6)) * 16;
}
// SCALE_OK: the launch may hold levels that estimate the source depth's scale (Sim(3)).  The common instantiation (false) carries
// neither the scale column's sums nor the 7-unknown solver: 256 registers instead of 512, i.e. TWO workgroups per CU instead of one
// -- twice the pairs in flight (a waiting member holds its slot).
// SEVERAL SLOTS PER WORKGROUP (round 4; ICP_SLOTS).  The trace of a 512-pair launch (tools/bench_icp.py, TL3D_ICP_TRACE) showed a pass
// of a pair at ~21 us of which a member accumulated for 9 and then sat out 10-12: the stragglers' arrivals, the last arriver's sum +
// solve + pose update (5-7 us on one wave) and the poll.  A workgroup therefore holds several (pair, member) slots and runs whichever
// has its pose, the oldest first: while slot A's pair is being solved, slot B accumulates.  With two slots a pair's pass stretches to
// 33 us (a member's workgroup may be busy with its other slot for a pass when the pose arrives) and the workgroups still idle a
// third of the time; with four they were busy and the launch no faster: what remained was the cost per member and pass, and the
// answer to that fewer members per pair (tl3d_internal.h: ICP_BATCH_SAMPLES_PER_MEMBER).  Two slots it is.
// Nothing blocks on ONE slot: a workgroup with a ready slot runs it, a workgroup with none polls the generation lines of all its
// waiting slots in turn -- so every pair whose tickets are all handed out still completes whatever the other slots of its workgroups
// hold (the argument above, per slot), and the slots it frees take the next tickets.  Slot s only takes a ticket once every workgroup
// of the grid has had the chance of s earlier ones (tickets handed out >= s * gridDim.x): a launch with fewer slots than the chip
// holds workgroups spreads over all CUs as before.
// TAB: the pixel-ray factors of the W columns and H rows sit in (dynamic) LDS, filled once per workgroup (icp_accumulate_core);
// frames too large for that (W + H > ICP_RAY_TAB_MAX) run the instantiation that divides.
constexpr int ICP_RAY_TAB_MAX = 12288;                     // floats: 48 KB
#ifndef TL3D_ICP_SLOTS
#define TL3D_ICP_SLOTS 2
#endif
constexpr int ICP_SLOTS = TL3D_ICP_SLOTS;                  // (pair, member) slots a workgroup works on in turn
enum { ICP_PH_NEED = 0, ICP_PH_INIT = 1, ICP_PH_READY = 2, ICP_PH_WAITING = 3, ICP_PH_EMPTY = 4 };
struct IcpSlot {                                           // LDS; written by thread 0 only, read by all after a barrier
    int phase, ticket, pair, member;
    int lv, it, done, over, failed_run, final_pass;
    unsigned gen, polls;
    unsigned long long wait_t0;
};
template <bool SCALE_OK, bool TAB>
__global__ __launch_bounds__(256, SCALE_OK ? 1 : 2) void icp_batch_kernel(Cam cam, IcpBatchArgs a) {
    __shared__ double sm[8][ICP_SLAB];
    __shared__ double tot[ICP_SLAB];
    __shared__ float sT[ICP_SLOTS][16];                    // per slot: the pose as 12 floats + the source depth's scale
    __shared__ IcpSlot sl[ICP_SLOTS];
    __shared__ int s_flag[4];                              // [1] last arriver, [3] leave the launch (a wait timed out)
    extern __shared__ float ray_tab_lds[];                 // TAB: [W] x factors, then [H] y factors
    const float *ray_tab = ray_tab_lds;
    const int tid = threadIdx.x;
    if (TAB) {
        for (int i = tid; i < cam.W; i += 256) ray_tab_lds[i] = ((float)i - cam.cx) / cam.fx;
        for (int i = tid; i < cam.H; i += 256) ray_tab_lds[cam.W + i] = ((float)i - cam.cy) / cam.fy;
    }
    if (tid == 0) {
        for (int s = 0; s < ICP_SLOTS; ++s) sl[s].phase = ICP_PH_NEED;
        s_flag[3] = 0;
    }
    __syncthreads();
    const size_t gen_base = (size_t)64 * a.sync_rows * 16;
    // what the pair of a pass just completed goes on with, from the generation word (thread 0)
    auto advance = [&](int s, unsigned word) {
        IcpSlot &S = sl[s];
        S.gen += 1u;
        S.done = (int)(word & 1u);
        S.over = (int)((word >> 1) & 1u);
        S.failed_run = (int)((word >> 2) & 1u);
        if (S.final_pass) {
            if (S.over || S.lv + 1 >= a.n_levels) {
                S.phase = ICP_PH_NEED;                     // the pair is through: the slot takes the next ticket
            } else {
                S.lv += 1; S.it = 0; S.done = 0; S.over = 0;
                S.phase = ICP_PH_READY;
            }
        } else {
            S.it += 1;
            S.phase = ICP_PH_READY;
        }
    };
    for (;;) {
        // ---- tickets and initial poses ---------------------------------------------------------------------------------------
        if (tid == 0) {
            for (int s = 0; s < ICP_SLOTS; ++s) {
                if (sl[s].phase != ICP_PH_NEED) continue;
                if (s > 0 && __hip_atomic_load(a.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)s * gridDim.x) continue;
                const int ticket = (int)__hip_atomic_fetch_add(a.ctl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int pair = ticket / a.members;
                if (pair >= a.n_pairs) { sl[s].phase = ICP_PH_EMPTY; continue; }     // every slot has been handed out
                IcpSlot &S = sl[s];
                S.phase = ICP_PH_INIT; S.ticket = ticket; S.pair = pair; S.member = ticket - pair * a.members;
                S.lv = 0; S.it = 0; S.done = 0; S.over = 0; S.failed_run = 0; S.final_pass = 0; S.gen = 0u; S.polls = 0u; S.wait_t0 = 0ull;
                if (a.stage) { unsigned *stage = a.stage + (size_t)ticket * 4; stage[0] = 1u; stage[1] = (unsigned)blockIdx.x; stage[3] = __builtin_amdgcn_s_getreg((4 << 11) | (0 << 6) | 20); }
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < ICP_SLOTS; ++s)
            if (sl[s].phase == ICP_PH_INIT) {              // the initial pose and scale: uploaded before the launch
                const IcpState *st0 = a.states + sl[s].pair;
                if (tid < 12) sT[s][tid] = (float)st0->T[tid];
                if (tid == 12) sT[s][12] = (float)st0->scale;
            }
        __syncthreads();
        if (tid == 0)
            for (int s = 0; s < ICP_SLOTS; ++s)
                if (sl[s].phase == ICP_PH_INIT) sl[s].phase = ICP_PH_READY;
        __syncthreads();
        int run = -1, n_wait = 0;
#pragma unroll
        for (int s = 0; s < ICP_SLOTS; ++s) {
            const int ph = sl[s].phase;
            if (ph == ICP_PH_READY && (run < 0 || sl[s].ticket < sl[run].ticket)) run = s;      // the oldest pair first
            n_wait += (ph == ICP_PH_WAITING);
        }
        // Every wave has taken its decision from the same slot states before anybody changes them: wave 0's poll below may move a
        // slot to READY, and a wave that read the states only then would run a pass while the others poll (barriers out of step).
        __syncthreads();
        // Nothing in hand: slot 0, which takes a ticket whenever it needs one, is neither ready nor waiting, so it has found every
        // ticket handed out -- and so would the later slots that have not tried yet.
        if (run < 0 && n_wait == 0) return;
        if (run < 0) {
            // ---- no slot has its pose: wave 0 polls the generation lines of the waiting ones ----------------------------------
            // One wave instruction per line (14 lanes, one 64-B request) returns the flags and the pose together.  Polling is a
            // read-modify-write atomic, which executes at the memory side: polls by agent-scope (sc1) LOADS were seen to return a
            // word their XCD had cached before the store for seconds, whatever the allocation flags.
            if (tid < 64) {
                bool got = false;
#pragma unroll
                for (int s = 0; s < ICP_SLOTS; ++s) {
                    if (sl[s].phase != ICP_PH_WAITING) continue;
                    unsigned *genl = a.sync + gen_base + icp_sync_line(sl[s].pair, a.sync_rows);
                    unsigned w = 0;
                    if (tid < 14) w = __hip_atomic_fetch_add(genl + tid, (unsigned)a.zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned word = __builtin_amdgcn_readfirstlane(w);
                    if ((word >> 3) != sl[s].gen) {
                        if (tid >= 1 && tid <= 13) sT[s][tid - 1] = __uint_as_float(w);
                        if (tid == 0) {
                            if (a.dbg && sl[s].pair == 0 && sl[s].gen < 16u) a.dbg[((size_t)sl[s].member * 16 + sl[s].gen) * 8 + 6] = wall_clock64();
                            advance(s, word);
                        }
                        got = true;
                    } else if (tid == 0) {
                        const unsigned polls = ++sl[s].polls;
                        if ((polls & 63u) == 0u &&
                            (wall_clock64() - sl[s].wait_t0 > ICP_WAIT_LIMIT_TICKS || __hip_atomic_load(a.ctl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
                            if (__hip_atomic_exchange(a.ctl + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
                                unsigned *arrive = a.sync + icp_sync_line(sl[s].pair, a.sync_rows);
                                a.ctl[4] = (unsigned)sl[s].pair; a.ctl[5] = (unsigned)sl[s].member; a.ctl[6] = sl[s].gen; a.ctl[7] = polls;      // the first time-out, for the host's message
                                a.ctl[8] = __hip_atomic_fetch_add(arrive, (unsigned)a.zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                a.ctl[9] = word;
                                a.ctl[10] = (unsigned)sl[s].lv; a.ctl[11] = (unsigned)sl[s].it;
                            }
                            s_flag[3] = 1;
                        }
                    }
                }
                if (!got) __builtin_amdgcn_s_sleep(16);    // polls of one line from a hundred CUs at full rate saturate its channel and starve the arrivals
            }
            __syncthreads();
            if (s_flag[3]) return;                         // a wait timed out: the error word is set, the host reports it
            continue;
        }
        // ---- one pass of slot `run` ----------------------------------------------------------------------------------------------
        const int pair = sl[run].pair, member = sl[run].member, lv = sl[run].lv, it = sl[run].it;
        const unsigned gen = sl[run].gen;
        const int failed_run = sl[run].failed_run;
        const IcpBatchPair pr = a.pairs[pair];
        IcpState *st = a.states + pair;
        const IcpLevel L = a.lv[lv];
        const int done = sl[run].done;
        const int final_pass = (done || it >= L.iters);
        unsigned *stage = a.stage ? a.stage + (size_t)sl[run].ticket * 4 : nullptr;      // experiments: how far this slot got
        unsigned *arrive = a.sync + icp_sync_line(pair, a.sync_rows);
        unsigned *genl = a.sync + gen_base + icp_sync_line(pair, a.sync_rows);
        double *slab = a.slab + (size_t)pair * a.members * ICP_SLAB;
        unsigned long long *dbg = (a.dbg && pair == 0 && tid == 0) ? a.dbg + (size_t)member * 16 * 8 : nullptr;
#define ICP_STAMP(k_) do { if (dbg && gen < 16u) dbg[gen * 8 + (k_)] = wall_clock64(); } while (0)
        ICP_STAMP(0);
        {
            // the pose is the same in every lane: scalar registers (an LDS read lands in vector registers, twelve of them, live
            // through the whole accumulation)
            auto uni = [](float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); };
            const float *P = sT[run];
            float r[9], t[3];
            r[0] = uni(P[0]); r[1] = uni(P[1]); r[2] = uni(P[2]);  t[0] = uni(P[3]);
            r[3] = uni(P[4]); r[4] = uni(P[5]); r[5] = uni(P[6]);  t[1] = uni(P[7]);
            r[6] = uni(P[8]); r[7] = uni(P[9]); r[8] = uni(P[10]); t[2] = uni(P[11]);
            const float sc_u = uni(P[12]);
            ICP_STAMP(1);
            const int est = SCALE_OK ? (final_pass ? 0 : L.est_scale) : 0;
            if (est)
                icp_accumulate_core<true, TAB>(cam, pr.depth_src, pr.nmap_tgt, sc_u, a.mind, a.maxd, L.md2, L.stride, L.Ws, L.Hs, r, t, member, a.members, pr.src_pm, sm, tot,
                                               (dbg && gen < 16u) ? dbg + gen * 8 + 3 : nullptr, ray_tab);
            else
                icp_accumulate_core<false, TAB>(cam, pr.depth_src, pr.nmap_tgt, sc_u, a.mind, a.maxd, L.md2, L.stride, L.Ws, L.Hs, r, t, member, a.members, pr.src_pm, sm, tot,
                                                (dbg && gen < 16u) ? dbg + gen * 8 + 3 : nullptr, ray_tab);
            ICP_STAMP(2);
            if (stage && tid == 0) stage[0] = 2u + 16u * gen;
            if (tid < ICP_SLAB) {
                __hip_atomic_store(slab + (size_t)member * ICP_SLAB + tid, tot[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __syncthreads();
            if (tid == 0) {
                const unsigned arrived = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int last = (arrived == (unsigned)a.members - 1u);
                if (stage) { stage[0] = 3u + 16u * gen; stage[2] = arrived; }
                if (last) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                s_flag[1] = last;
                sl[run].final_pass = final_pass;
                if (!last) { sl[run].phase = ICP_PH_WAITING; sl[run].polls = 0u; sl[run].wait_t0 = wall_clock64(); }
                if (dbg && gen < 16u) dbg[gen * 8 + 7] = (unsigned long long)last;
            }
            ICP_STAMP(5);
            __syncthreads();
            if (s_flag[1]) {                               // the last arriver: sum, solve, new pose, publish
                const int fin = icp_finish(slab, a.members, st, L.damping, L.eps, L.eig_rel, final_pass, sm, tot, est, sT[run], it);
                if (tid < 64) {                            // wave 0 publishes
                    // thread 0 may just have written the new pose to sT: make that visible to lanes 1..12 of this wave
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    // pose words and the arrival counter of the next pass: one instruction, issued before the state stores have drained
                    // (returning forms: their data comes back only after the memory side has performed them)
                    unsigned old = 0;
                    if (tid >= 1 && tid <= 13) old = __hip_atomic_exchange(genl + tid, __float_as_uint(sT[run][tid - 1]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (tid == 14) old = __hip_atomic_exchange(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    asm volatile("" ::"v"(old));
                    unsigned word = 0;
                    if (tid == 0) {
                        int fl_done = (done || fin != 0), fl_fail = (failed_run || fin == 2), fl_over = 0;
                        if (final_pass) {                  // what the host did between levels: stop on failure or < 8 correspondences
                            if (lv == a.n_levels - 1 || fl_fail || tot[28] < 8.0) {
                                st_agent(&st->over, 1);
                                fl_over = 1;
                            } else {
                                st_agent(&st->done, 0);
                                st_agent(&st->status, 0);
                                st_agent(&st->iters_run, 0);
                                fl_done = 0;
                            }
                        }
                        word = ((gen + 1u) << 3) | (fl_fail ? 4u : 0u) | (fl_over ? 2u : 0u) | (fl_done ? 1u : 0u);
                    }
                    // state stores written through, pose words and arrival counter in place: only then the flags word says so
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (tid == 0) {
                        (void)__hip_atomic_exchange(genl, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (dbg && gen < 16u) dbg[gen * 8 + 6] = wall_clock64();
                        advance(run, word);
                    }
                }
            }
        }
#undef ICP_STAMP
        __syncthreads();                                   // slot state and the shared scratch are rewritten by the next trip
    }
}

int launch_icp_batch(hipStream_t s, const Cam &cam, const IcpBatchArgs &a) {
    bool scale = false;
    for (int l = 0; l < a.n_levels; ++l) scale = scale || a.lv[l].est_scale != 0;
    const bool tab = cam.W + cam.H <= ICP_RAY_TAB_MAX;
    const size_t lds = tab ? (size_t)(cam.W + cam.H) * sizeof(float) : 0;
    using Kern = void (*)(Cam, IcpBatchArgs);
    const Kern kern = scale ? (tab ? (Kern)icp_batch_kernel<true, true> : (Kern)icp_batch_kernel<true, false>)
                            : (tab ? (Kern)icp_batch_kernel<false, true> : (Kern)icp_batch_kernel<false, false>);
    static int resident[2][2] = {{0, 0}, {0, 0}};          // workgroups the chip holds at once, per instantiation
    static size_t resident_lds[2][2] = {{0, 0}, {0, 0}};   // ... for this much dynamic LDS
    if (!resident[scale][tab] || resident_lds[scale][tab] != lds) {
        int dev = 0, cus = 0, per_cu = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds);
        if (e != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 1; }
        resident[scale][tab] = per_cu * cus;
        resident_lds[scale][tab] = lds;
    }
    const unsigned slots = (unsigned)a.n_pairs * (unsigned)a.members;
    const unsigned grid = slots < (unsigned)resident[scale][tab] ? slots : (unsigned)resident[scale][tab];
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, cam, a);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// a normal map (phase-major rows) as the row-major [H][W] image the caller of tl3d_download_normals gets
__global__ __launch_bounds__(256) void nmap_rowmajor_kernel(int W, int H, const float4 *__restrict__ nmap, float4 *__restrict__ out) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u < W && v < H) out[(size_t)v * W + u] = nmap[pm_index(u, v, pm_w4(W))];
}

int launch_nmap_rowmajor(hipStream_t s, const Cam &cam, const float4 *nmap, float4 *out) {
    hipLaunchKernelGGL(nmap_rowmajor_kernel, dim3((cam.W + 63) / 64, (cam.H + 3) / 4), dim3(256), 0, s, cam.W, cam.H, nmap, out);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// radius 0: central differences of the depth image itself; radius >= 1: the window-averaged depth goes to `sdepth` first and the
// normals come from it with a `radius`-pixel step
int launch_normals(hipStream_t s, const Cam &cam, const float *depth, float scale, float mind, float maxd, float jump, int radius, float *sdepth,
                   float4 *nmap) {
    dim3 grid((cam.W + 63) / 64, (cam.H + 3) / 4);
    if (radius >= 1) {
        hipLaunchKernelGGL(smooth_depth_kernel, grid, dim3(256), 0, s, cam, depth, scale, mind, maxd, jump, radius, sdepth);
        TL3D_HIP(hipGetLastError());
        hipLaunchKernelGGL(normals_kernel<true>, grid, dim3(256), 0, s, cam, sdepth, scale, mind, maxd, jump, radius, nmap);
    } else {
        hipLaunchKernelGGL(normals_kernel<false>, grid, dim3(256), 0, s, cam, depth, scale, mind, maxd, jump, 1, nmap);
    }
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

int launch_icp_iteration(hipStream_t s, const Cam &cam, const IcpRun *run, int final_pass, double *slab, IcpState *state, int nblocks,
                         unsigned *ticket) {
    hipLaunchKernelGGL(icp_iter_kernel, dim3(nblocks), dim3(256), 0, s, cam, run, state, final_pass, slab, ticket);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

}  // namespace tl3d
