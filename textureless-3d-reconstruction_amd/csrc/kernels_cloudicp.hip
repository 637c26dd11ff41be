// kernels_cloudicp.hip -- registration of two unorganised point clouds (tl3d_cloud_evaluate, tl3d_cloud_register; DESIGN.md section
// 14): ICP over the uniform cell index of cellgrid.h, point-to-plane or point-to-point, optionally with scale as a 7th unknown.  No
// reference code: the reference never registers a cloud; the method is the unorganised-cloud ICP of any point-cloud library.
//
// One pass at the pose (T, sigma) in device memory (IcpState), every operation fp64 and rounded once (-ffp-contract=off), in the
// order include/tl3d.h states and tests/cloud_register_reference.py restates:
//   m = R p, w = sigma m, q = w + t;  y = argmin (d2, index) over the target;  kept iff sqrt(d2) <= max_dist;  e = q - y
//   row(n): r = n . e, J = [q x n, n, n . w];  point-to-plane: one row with y's normal; point-to-point: rows n = e_x, e_y, e_z
// A pass is TWO kernels with 4 bytes per source point between them:
//   cloud_search_kernel   one thread per sampled point: q, the shell walk and the stop bound of nn_search_kernel (q may lie far outside
//                         the target's box), the winner's index (or -1) to index[i].  Threads may serve the samples in ANY order: the
//                         order only decides which lanes share a wave, a thread's result depends on its own point alone.
//   cloud_reduce_kernel   in input order with a shape that depends on n_src alone: thread t of the launch takes samples t, t + G, ...
//                         (G = 256 cloud_members(n_src)), recomputes q and the rows from the stored index, adds them in that order;
//                         then wave shuffle, LDS in wave order, one partial per workgroup.  cloud_step_kernel (kernels_regstep.hip) adds
//                         the partials in member order.
// So the sums, and the pose, are the same bytes in every run, for every cell size and for every query order: nothing that varies
// (fill order inside a cell, the cells' size, which lanes walk together) reaches a sum other than through an index that is itself
// the unique minimum of (d2, index).
// The target's index is built once per call.  Per level the sampled points are bucketed by the target grid's cell (unless the context
// runs its queries in input order): cloud_order_kernel writes f32-rounded copies of q at the level's first pose, and a second
// cell_index_build over the target's cnt gives the order.  The copies are used for ordering only.
// Everything is enqueued on the context's stream; launches behind a converged or failed level return at once.
#include <math.h>

#include <algorithm>
#include <vector>

#include "api_host.h"
#include "cellgrid.h"

namespace tl3d {

constexpr int CLOUD_MEMBERS_CAP = 512;     // workgroups of the reduce pass at most: two per CU; the step adds that many partials

struct CloudPose { double R[9], t[3], s; };
__device__ __forceinline__ CloudPose cloud_pose(const IcpState *__restrict__ st) {
    CloudPose P;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) P.R[3 * i + j] = st->T[4 * i + j];
        P.t[i] = st->T[4 * i + 3];
    }
    P.s = st->scale;
    return P;
}
// w = sigma (R p), q = w + t
__device__ __forceinline__ void cloud_transform(const CloudPose &P, const float *__restrict__ p, double w[3], double q[3]) {
    const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double m = (P.R[3 * a] * px + P.R[3 * a + 1] * py) + P.R[3 * a + 2] * pz;
        w[a] = P.s * m;
        q[a] = w[a] + P.t[a];
    }
}

// f32 copies of the sampled points at the state's pose: what the level's query order is built from, and nothing else
__global__ __launch_bounds__(256) void cloud_order_kernel(const float *__restrict__ src, long long n_samp, int stride, const IcpState *__restrict__ state,
                                                          float *__restrict__ qf) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_samp) return;
    const CloudPose P = cloud_pose(state);
    double w[3], q[3];
    cloud_transform(P, src + 3 * (k * stride), w, q);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float f = (float)q[a];
        qf[3 * k + a] = isfinite(f) ? f : 0.0f;            // (a pose that left the floats' range: any cell will do)
    }
}

// order == nullptr: thread k serves sample k; else sample order[k]
__global__ __launch_bounds__(256) void cloud_search_kernel(CellGrid g, const float *__restrict__ src, long long n_samp, int stride,
                                                           const unsigned *__restrict__ order, const unsigned *__restrict__ start, NnPointEval eval,
                                                           double max_dist, const IcpState *__restrict__ state, StepKind kind,
                                                           int *__restrict__ index) {
    if (state->over || (kind == STEP_ITERATE && state->done)) return;      // set by EARLIER launches only: uniform over the grid
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_samp) return;
    const long long i = (order ? (long long)order[t] : t) * stride;
    const CloudPose P = cloud_pose(state);
    double w[3], p[3];
    cloud_transform(P, src + 3 * i, w, p);
    const int n[3] = {g.nx, g.ny, g.nz};
    const double u[3] = {cell_u(p[0], g.ox, g.inv_cell), cell_u(p[1], g.oy, g.inv_cell), cell_u(p[2], g.oz, g.inv_cell)};
    int c[3];
    double box2[3];
    const double nmax = (double)max(g.nx, max(g.ny, g.nz)) + 1.0;
    for (int a = 0; a < 3; ++a) {
        c[a] = cell_clampi(u[a], n[a]);
        const double b = cell_lower(fmax(0.0, fmax(-u[a], u[a] - (double)n[a])), nmax + fabs(u[a]), g.cell);
        box2[a] = b * b;
    }
    const double md2 = max_dist > 0.0 ? max_dist * max_dist : INFINITY;
    NnBest best = {INFINITY, 0x7fffffff};
    for (int r = 0;; ++r) {
        cell_shell_walk(g, start, c[0], c[1], c[2], r, [&](unsigned s, unsigned e) { eval(s, e, p[0], p[1], p[2], best); });
        double bound2 = INFINITY;
        bool open = false;
        cell_face_bound(u[0], c[0], r, g.nx, nmax, g.cell, box2[1] + box2[2], bound2, open);
        cell_face_bound(u[1], c[1], r, g.ny, nmax, g.cell, box2[2] + box2[0], bound2, open);
        cell_face_bound(u[2], c[2], r, g.nz, nmax, g.cell, box2[0] + box2[1], bound2, open);
        if (!open || best.d2 < bound2 || bound2 > md2) break;
    }
    int idx = best.idx;
    if (!(sqrt(best.d2) <= (max_dist > 0.0 ? max_dist : INFINITY)) || idx == 0x7fffffff) idx = -1;
    index[i] = idx;
}

// one row of the system: r = n . e, J = [q x n, n, n . w]; acc: the upper triangle of the 7 x 7 matrix row-major (28), b (7), e
template <bool SCALE>
__device__ __forceinline__ void cloud_row(const double n[3], const double e[3], const double q[3], const double w[3], double (&acc)[36]) {
    const double r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2];
    double J[7];
    J[0] = q[1] * n[2] - q[2] * n[1];
    J[1] = q[2] * n[0] - q[0] * n[2];
    J[2] = q[0] * n[1] - q[1] * n[0];
    J[3] = n[0];
    J[4] = n[1];
    J[5] = n[2];
    J[6] = SCALE ? (n[0] * w[0] + n[1] * w[1]) + n[2] * w[2] : 0.0;
    int m = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = i; j < 7; ++j) {
            if (SCALE || j < 6) acc[m] += J[i] * J[j];
            ++m;
        }
        if (SCALE || i < 6) acc[28 + i] += J[i] * r;
    }
    acc[35] += r * r;
}

// where entry k of acc (the 7 x 7 triangle, b, e) lies in IcpState::sums
__device__ __forceinline__ constexpr int cloud_sum_slot(int k) {
    if (k == 35) return 27;
    if (k >= 28) return k - 28 < 6 ? 21 + (k - 28) : 39;
    int m = 0, m6 = 0;
    for (int i = 0; i < 7; ++i)
        for (int j = i; j < 7; ++j) {
            if (m == k) return j < 6 ? m6 : (i < 6 ? 32 + i : 38);
            ++m;
            if (j < 6) ++m6;
        }
    return 31;
}

template <bool PLANE, bool SCALE>
__global__ __launch_bounds__(256) void cloud_reduce_kernel(const float *__restrict__ src, long long n_samp, int stride, const float *__restrict__ tgt,
                                                           const float *__restrict__ nrm, const int *__restrict__ index,
                                                           const IcpState *__restrict__ state, StepKind kind, double *__restrict__ slab) {
    if (state->over || (kind == STEP_ITERATE && state->done)) return;
    __shared__ double sm[4][CLOUD_SUMS];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const CloudPose P = cloud_pose(state);
    double acc[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] = 0.0;
    double n_corr = 0.0, n_samples = 0.0, n_zero = 0.0;
#pragma unroll 1
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n_samp; k += (long long)gridDim.x * 256) {
        const long long i = k * stride;
        n_samples += 1.0;
        const int idx = index[i];
        if (idx < 0) continue;
        double w[3], q[3];
        cloud_transform(P, src + 3 * i, w, q);
        const float *y = tgt + 3 * (size_t)idx;
        const double e[3] = {q[0] - (double)y[0], q[1] - (double)y[1], q[2] - (double)y[2]};
        if (PLANE) {
            const float *nf = nrm + 3 * (size_t)idx;
            const double n[3] = {(double)nf[0], (double)nf[1], (double)nf[2]};
            if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) { n_zero += 1.0; continue; }
            n_corr += 1.0;
            cloud_row<SCALE>(n, e, q, w, acc);
        } else {
            n_corr += 1.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double n[3] = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
                cloud_row<SCALE>(n, e, q, w, acc);
            }
        }
    }
    // every lane is back here: the shuffles run with EXEC full
#pragma unroll
    for (int k = 0; k < 36; ++k) {
        double v = acc[k];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
        if (lane == 0) sm[wid][cloud_sum_slot(k)] = v;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        n_corr += __shfl_down(n_corr, d);
        n_samples += __shfl_down(n_samples, d);
        n_zero += __shfl_down(n_zero, d);
    }
    if (lane == 0) {
        sm[wid][ICP_SUM_CORR] = n_corr;
        sm[wid][ICP_SUM_SRC] = n_samples;
        sm[wid][CLOUD_SUM_NO_NORMAL] = n_zero;
        sm[wid][31] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < CLOUD_SUMS)
        slab[(size_t)blockIdx.x * CLOUD_SUMS + threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
#define CI_HIP(x)                                                                                   \
    do {                                                                                            \
        hipError_t e__ = (x);                                                                       \
        if (e__ != hipSuccess) return set_err(TL3D_E_HIP, "%s failed: %s", #x, hipGetErrorString(e__)); \
    } while (0)

// workgroups of the reduce pass: a function of the source's size alone (256 points per workgroup until the cap)
int cloud_members(long long n_src) { return (int)std::max(1ll, std::min((long long)CLOUD_MEMBERS_CAP, (n_src + 255) / 256)); }

static long long cloud_samples(long long n_src, int stride) { return (n_src + stride - 1) / stride; }

// Every pointer is device memory but `levels`; n_src, n_tgt >= 1.  The run starts at the pose already in *state.  evaluate: one
// search, one reduce and a final step at levels[0]'s stride and gate (its max_dist <= 0: unlimited).  index_out: [n_src] or null.
int cloud_icp_run(tl3d_ctx *ctx, const float *src, long long n_src, const float *tgt, long long n_tgt, const float *nrm,
                  const tl3d_icp_params *levels, int n_levels, bool evaluate, double cell, IcpState *state, int *index_out) {
    hipStream_t s = ctx->stream;
    int rc = cell_slab(ctx);
    if (rc) return rc;
    float *bslab = (float *)ctx->cg_slab;
    std::vector<float> h((size_t)NN_RED * 16);
    nn_bounds_launch(s, src, n_src, bslab);
    nn_bounds_launch(s, tgt, n_tgt, bslab + (size_t)NN_RED * 8);
    CI_HIP(hipGetLastError());
    CI_HIP(hipMemcpyAsync(h.data(), bslab, h.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    CI_HIP(hipStreamSynchronize(s));
    double mn[3], mx[3];
    unsigned long long bad = nn_bounds_fold(h.data(), n_src, mn, mx);
    if (bad) return set_err(TL3D_E_INVALID, "%llu source points have a non-finite coordinate", bad);
    bad = nn_bounds_fold(h.data() + (size_t)NN_RED * 8, n_tgt, mn, mx);
    if (bad) return set_err(TL3D_E_INVALID, "%llu target points have a non-finite coordinate", bad);
    if (!(cell > 0.0)) cell = nn_default_cell_points(mn, mx, n_tgt);
    CellGrid g;
    cell_grid_fit(mn, mx, cell, &g);
    const long long ncell = cell_grid_cells(g);
    long long max_samp = 0;
    for (int l = 0; l < n_levels; ++l) max_samp = std::max(max_samp, cloud_samples(n_src, levels[l].stride));
    const int members = cloud_members(n_src);
    const bool ordered = !ctx->nn_input_order;
    // the target's tables, the queries' start table over the same cnt, the sorted target, the query order and the f32 copies it is
    // built from, the indices between the two kernels of a pass, the block partials
    size_t bytes[10];
    cell_table_bytes(ncell, bytes);
    bytes[4] = (size_t)(ncell + 1) * sizeof(unsigned);
    bytes[5] = (size_t)n_tgt * sizeof(float4);
    bytes[6] = ordered ? (size_t)max_samp * sizeof(unsigned) : 0;
    bytes[7] = ordered ? (size_t)max_samp * 3 * sizeof(float) : 0;
    bytes[8] = index_out ? 0 : (size_t)n_src * sizeof(int);
    bytes[9] = (size_t)members * CLOUD_SUMS * sizeof(double);
    void *p[10];
    rc = scratch_carve(ctx, 0, bytes, 10, p, "cloud registration scratch");
    if (rc) return rc;
    const CellTables tt = CellTables::at(p);
    CellTables qt = tt;
    qt.start = (unsigned *)p[4];
    float4 *sorted = (float4 *)p[5];
    unsigned *order = (unsigned *)p[6];
    float *qf = (float *)p[7];
    int *index = index_out ? index_out : (int *)p[8];
    double *slab = (double *)p[9];
    rc = cell_index_build(s, g, tgt, n_tgt, tt, true, EmitPointIndex{sorted});
    if (rc) return rc;
    CI_HIP(hipMemsetAsync(index, 0xff, (size_t)n_src * sizeof(int), s));        // -1: not sampled (a level writes its samples only)
    const NnPointEval pe = {sorted};
    for (int l = 0; l < n_levels; ++l) {
        const tl3d_icp_params &lv = levels[l];
        const long long n_samp = cloud_samples(n_src, lv.stride);
        const unsigned nb = (unsigned)((n_samp + 255) / 256);
        const int est = lv.estimate_scale ? 1 : 0;
        if (ordered) {
            hipLaunchKernelGGL(cloud_order_kernel, dim3(nb), dim3(256), 0, s, src, n_samp, lv.stride, (const IcpState *)state, qf);
            CI_HIP(hipGetLastError());
            rc = cell_index_build(s, g, qf, n_samp, qt, false, EmitIndex{order});
            if (rc) return rc;
        }
        const int passes = evaluate ? 1 : lv.iters + 1;
        for (int it = 0; it < passes; ++it) {
            const StepKind kind = step_kind(it, lv.iters, l == n_levels - 1, evaluate);
            hipLaunchKernelGGL(cloud_search_kernel, dim3(nb), dim3(256), 0, s, g, src, n_samp, lv.stride, ordered ? (const unsigned *)order : nullptr,
                               (const unsigned *)tt.start, pe, lv.max_dist, (const IcpState *)state, kind, index);
            const dim3 rg(members), rb(256);
#define CLOUD_REDUCE(PL, SC) \
    hipLaunchKernelGGL((cloud_reduce_kernel<PL, SC>), rg, rb, 0, s, src, n_samp, lv.stride, tgt, nrm, (const int *)index, (const IcpState *)state, kind, slab)
            if (nrm) { if (est) CLOUD_REDUCE(true, true); else CLOUD_REDUCE(true, false); }
            else     { if (est) CLOUD_REDUCE(false, true); else CLOUD_REDUCE(false, false); }
#undef CLOUD_REDUCE
            CI_HIP(hipGetLastError());
            rc = launch_cloud_step(s, slab, members, state, est, lv.damping, lv.eps, lv.eig_rel, kind);
            if (rc) return rc;
        }
    }
    return TL3D_OK;
}

}  // namespace tl3d
