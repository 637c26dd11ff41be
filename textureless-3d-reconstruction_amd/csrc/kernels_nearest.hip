// kernels_nearest.hip -- exact nearest-neighbour search from one set to ANOTHER: for every query point the
// nearest target point (tl3d_nearest_points) or the nearest point of an indexed triangle list (tl3d_nearest_triangles), distance in
// fp64 and the index of what was hit; and the fixed-shape summary of a distance array (tl3d_distance_summary).  No reference code:
// the reference never scores a cloud; the definitions are those of Open3D's compute_point_cloud_distance and of the Chamfer / F-score
// literature.
//
// The target is counting-sorted into the uniform cell index of cellgrid.h over its own box (cell_index_build; the original index rides
// beside each sorted point; a triangle goes into every cell its box overlaps: nn_tri_bin_kernel counts and fills in place of the
// build's count and fill, over the same tables and scan).  A query walks the shells of growing Chebyshev radius around its CLAMPED
// cell (cell_shell_walk).  Two things differ from the filter's k-NN:
//   * the winner is the minimum over the PAIR (d2, index), so neither the fill order inside a cell (atomics) nor the order in which
//     cells are met shows in the result, and an exact tie goes to the smaller index;
//   * the stop rule.  A query may lie outside the grid, so the search ends on the bound of cellgrid.h (cell_face_bound, derived
//     there): when no face is open, when best2 < bound2 (strictly: a tie further out may have the smaller index), or when
//     bound2 > max_dist^2.
#include <math.h>

#include <vector>

#include "api_host.h"
#include "cellgrid.h"

namespace tl3d {

constexpr int NN_LEVELS = 16;           // candidate cell sizes one triangle-pair count pass looks at (cell * 2^j)

// ---- validation -----------------------------------------------------------------------------------------------------------------
// per block: [0] the sum of the triangles' largest box extents (what the default cell is taken from; only the cell depends on it),
// [1] the number of triangles with an index >= n_vert.  An index is compared before it is used.
__global__ __launch_bounds__(256) void nn_tri_stats_kernel(const float *__restrict__ xyz, long long n_vert, const unsigned *__restrict__ tri,
                                                           long long n_tri, double *__restrict__ slab) {
    __shared__ double sm[4][2];
    double ext = 0.0, bad = 0.0;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n_tri; t += (long long)gridDim.x * 256) {
        const unsigned i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
        if ((long long)i0 >= n_vert || (long long)i1 >= n_vert || (long long)i2 >= n_vert) {
            bad += 1.0;
            continue;
        }
        float e = 0.0f;
        for (int a = 0; a < 3; ++a) {
            const float p = xyz[3 * (size_t)i0 + a], q = xyz[3 * (size_t)i1 + a], r = xyz[3 * (size_t)i2 + a];
            e = fmaxf(e, fmaxf(p, fmaxf(q, r)) - fminf(p, fminf(q, r)));
        }
        if (isfinite(e)) ext += (double)e;
    }
    for (int d = 32; d > 0; d >>= 1) { ext += __shfl_down(ext, d); bad += __shfl_down(bad, d); }
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = ext; sm[threadIdx.x >> 6][1] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        slab[2 * blockIdx.x] = ((sm[0][0] + sm[1][0]) + sm[2][0]) + sm[3][0];
        slab[2 * blockIdx.x + 1] = ((sm[0][1] + sm[1][1]) + sm[2][1]) + sm[3][1];
    }
}

// ---- triangles into cells ------------------------------------------------------------------------------------------------------
struct NnBox { int lo[3], hi[3]; };
__device__ __forceinline__ NnBox nn_tri_box(const CellGrid &g, const float *__restrict__ xyz, const unsigned *__restrict__ tri, long long t) {
    const float *a = xyz + 3 * (size_t)tri[3 * t], *b = xyz + 3 * (size_t)tri[3 * t + 1], *c = xyz + 3 * (size_t)tri[3 * t + 2];
    const double o[3] = {g.ox, g.oy, g.oz};
    const int n[3] = {g.nx, g.ny, g.nz};
    NnBox bx;
    for (int k = 0; k < 3; ++k) {
        bx.lo[k] = cell_clampi(cell_u((double)fminf(a[k], fminf(b[k], c[k])), o[k], g.inv_cell), n[k]);
        bx.hi[k] = cell_clampi(cell_u((double)fmaxf(a[k], fmaxf(b[k], c[k])), o[k], g.inv_cell), n[k]);
    }
    return bx;
}

struct NnLevels { CellGrid g[NN_LEVELS]; };
// total[j] = (triangle, cell) pairs of the grid g[j] (integer adds: the same in every run)
__global__ __launch_bounds__(256) void nn_tri_pairs_kernel(NnLevels lv, const float *__restrict__ xyz, const unsigned *__restrict__ tri,
                                                           long long n_tri, unsigned long long *__restrict__ total) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    for (int j = 0; j < NN_LEVELS; ++j) {
        unsigned long long c = 0;
        if (t < n_tri) {
            const NnBox b = nn_tri_box(lv.g[j], xyz, tri, t);
            c = (unsigned long long)(b.hi[0] - b.lo[0] + 1) * (unsigned long long)(b.hi[1] - b.lo[1] + 1) * (unsigned long long)(b.hi[2] - b.lo[2] + 1);
        }
        for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
        if ((threadIdx.x & 63) == 0 && c) atomicAdd(total + j, c);
    }
}

// fill == nullptr: count the triangle into every cell of its box; else write its index there (cnt counted down, as cell_fill_kernel does)
__global__ __launch_bounds__(256) void nn_tri_bin_kernel(CellGrid g, const float *__restrict__ xyz, const unsigned *__restrict__ tri, long long n_tri,
                                                         const unsigned *__restrict__ start, unsigned *__restrict__ cnt, unsigned *__restrict__ fill) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tri) return;
    const NnBox b = nn_tri_box(g, xyz, tri, t);
    for (int z = b.lo[2]; z <= b.hi[2]; ++z)
        for (int y = b.lo[1]; y <= b.hi[1]; ++y)
            for (int x = b.lo[0]; x <= b.hi[0]; ++x) {
                const long long c = ((long long)z * g.ny + y) * g.nx + x;
                if (!fill) atomicAdd(cnt + c, 1u);
                else fill[start[c] + atomicSub(cnt + c, 1u) - 1u] = (unsigned)t;
            }
}

// ---- the search ----------------------------------------------------------------------------------------------------------------
// (NnBest and NnPointEval: cellgrid.h, shared with kernels_cloudicp.hip)
// squared distance from the origin to the segment [p, q]
__device__ __forceinline__ double nn_seg_d2(const double p[3], const double q[3]) {
    const double e[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
    const double ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
    double t = 0.0;
    if (ee > 0.0) t = fmin(fmax(-(p[0] * e[0] + p[1] * e[1] + p[2] * e[2]) / ee, 0.0), 1.0);
    const double c[3] = {p[0] + t * e[0], p[1] + t * e[1], p[2] + t * e[2]};
    return c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
}
__device__ __forceinline__ void nn_cross(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double nn_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// Squared distance from the origin to the closed triangle (a, b, c), the corners given relative to the query.  The foot of the
// perpendicular lies in the triangle when the three edge functions n . (edge x (foot - corner)) are >= 0: then the distance is the
// plane's, (n . a)^2 / (n . n); otherwise the nearest point is on the boundary: the minimum over the three closed edges.  A
// triangle without a normal (collinear or repeated corners: n . n == 0) IS its boundary, so segments and points need no case.
__device__ __forceinline__ double nn_tri_d2(const double a[3], const double b[3], const double c[3]) {
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, bc[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
    const double ca[3] = {a[0] - c[0], a[1] - c[1], a[2] - c[2]};
    double n[3], w[3];
    nn_cross(ab, bc, n);
    const double nn = nn_dot(n, n);
    if (nn > 0.0) {
        // edge x (0 - corner) = corner x edge
        nn_cross(a, ab, w);
        const double wc = nn_dot(n, w);
        nn_cross(b, bc, w);
        const double wa = nn_dot(n, w);
        nn_cross(c, ca, w);
        const double wb = nn_dot(n, w);
        if (wa >= 0.0 && wb >= 0.0 && wc >= 0.0) {
            const double h = nn_dot(n, a);
            return h * h / nn;
        }
    }
    return fmin(nn_seg_d2(a, b), fmin(nn_seg_d2(b, c), nn_seg_d2(c, a)));
}

struct NnTriEval {
    const unsigned *__restrict__ pairs;
    const float *__restrict__ xyz;
    const unsigned *__restrict__ tri;
    __device__ __forceinline__ void operator()(unsigned s, unsigned e, double px, double py, double pz, NnBest &best) const {
        for (unsigned q = s; q < e; ++q) {
            const unsigned t = pairs[q];
            const float *pa = xyz + 3 * (size_t)tri[3 * (size_t)t], *pb = xyz + 3 * (size_t)tri[3 * (size_t)t + 1];
            const float *pc = xyz + 3 * (size_t)tri[3 * (size_t)t + 2];
            const double a[3] = {(double)pa[0] - px, (double)pa[1] - py, (double)pa[2] - pz};
            const double b[3] = {(double)pb[0] - px, (double)pb[1] - py, (double)pb[2] - pz};
            const double c[3] = {(double)pc[0] - px, (double)pc[1] - py, (double)pc[2] - pz};
            best.take(nn_tri_d2(a, b, c), (int)t);
        }
    }
};

// order == nullptr: thread i serves query i; else query order[i] (queries bucketed by cell: a wave's lanes walk the same cells)
template <class Eval>
__global__ __launch_bounds__(256) void nn_search_kernel(CellGrid g, const float *__restrict__ query, long long nq, const unsigned *__restrict__ order,
                                                        const unsigned *__restrict__ start, Eval eval, double max_dist,
                                                        double *__restrict__ dist_out, int *__restrict__ index_out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nq) return;
    const long long qi = order ? (long long)order[t] : t;
    const double p[3] = {(double)query[3 * qi], (double)query[3 * qi + 1], (double)query[3 * qi + 2]};
    const int n[3] = {g.nx, g.ny, g.nz};
    const double u[3] = {cell_u(p[0], g.ox, g.inv_cell), cell_u(p[1], g.oy, g.inv_cell), cell_u(p[2], g.oz, g.inv_cell)};
    int c[3];
    double box2[3];                                        // squared distance to the grid's extent, per axis (a lower bound)
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
    double d = sqrt(best.d2);
    int idx = best.idx;
    if (!(d <= (max_dist > 0.0 ? max_dist : INFINITY)) || idx == 0x7fffffff) { d = INFINITY; idx = -1; }
    if (dist_out) dist_out[qi] = d;
    if (index_out) index_out[qi] = idx;
}

__global__ __launch_bounds__(256) void nn_none_kernel(long long nq, double *__restrict__ dist_out, int *__restrict__ index_out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nq) return;
    if (dist_out) dist_out[t] = INFINITY;
    if (index_out) index_out[t] = -1;
}

// ---- summary -------------------------------------------------------------------------------------------------------------------
struct NnThr { double t[8]; };
// per block 16 words: [0] finite entries, [1 .. 8] entries <= threshold j (u64), [9] sum, [10] sum of squares, [11] max (fp64)
__global__ __launch_bounds__(256) void nn_summary_kernel(const double *__restrict__ d, long long n, int nthr, NnThr thr_in,
                                                         unsigned long long *__restrict__ slab) {
    __shared__ unsigned long long smc[4][9];
    __shared__ double smd[4][3];
    double thr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) thr[j] = thr_in.t[j];
    unsigned long long cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double sum = 0.0, sq = 0.0, mx = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double v = d[i];
        if (isfinite(v)) { cnt[0]++; sum += v; sq += v * v; mx = fmax(mx, v); }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < nthr && v <= thr[j]) cnt[1 + j]++;
    }
    for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
        for (int j = 0; j < 9; ++j) cnt[j] += __shfl_down(cnt[j], s);
        sum += __shfl_down(sum, s);
        sq += __shfl_down(sq, s);
        mx = fmax(mx, __shfl_down(mx, s));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 9; ++j) smc[w][j] = cnt[j];
        smd[w][0] = sum; smd[w][1] = sq; smd[w][2] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long *o = slab + 16 * (size_t)blockIdx.x;
        for (int j = 0; j < 9; ++j) o[j] = smc[0][j] + smc[1][j] + smc[2][j] + smc[3][j];
        o[9] = (unsigned long long)__double_as_longlong(((smd[0][0] + smd[1][0]) + smd[2][0]) + smd[3][0]);
        o[10] = (unsigned long long)__double_as_longlong(((smd[0][1] + smd[1][1]) + smd[2][1]) + smd[3][1]);
        o[11] = (unsigned long long)__double_as_longlong(fmax(fmax(smd[0][2], smd[1][2]), fmax(smd[2][2], smd[3][2])));
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
#define NN_HIP(x)                                                                                   \
    do {                                                                                            \
        hipError_t e__ = (x);                                                                       \
        if (e__ != hipSuccess) return set_err(TL3D_E_HIP, "%s failed: %s", #x, hipGetErrorString(e__)); \
    } while (0)

// Default cell of a point target: the box has V = the product of its non-zero extents (k of them) and n points; cell = (V / (4 n))^(1/k),
// i.e. four cells per point if the points filled the box -- surface clouds fill a thin sheet of it, and end near ten points per
// occupied cell.  A box without extent is one cell.
double nn_default_cell_points(const double mn[3], const double mx[3], long long n) {
    double v = 1.0;
    int k = 0;
    for (int a = 0; a < 3; ++a)
        if (mx[a] > mn[a]) { v *= mx[a] - mn[a]; ++k; }
    if (!k) return 1.0;
    const double c = pow(v / (4.0 * (double)n), 1.0 / k);
    return (c > 0.0 && isfinite(c)) ? c : 1.0;
}

// A search's scratch, carved from the context's buffer: the target's cell tables, the queries' start table over the same cnt, the
// target's payload behind the cells (P: float4 points, or triangle indices) and the query order.
template <class P> struct NnScratch {
    CellTables t;
    unsigned *q_start;
    P *payload;
    unsigned *order;
};
template <class P> static int nn_scratch(tl3d_ctx *ctx, long long ncell, size_t n_payload, long long nq, NnScratch<P> *sc) {
    size_t bytes[7];
    cell_table_bytes(ncell, bytes);
    bytes[4] = (size_t)(ncell + 1) * sizeof(unsigned);
    bytes[5] = n_payload * sizeof(P);
    bytes[6] = (size_t)nq * sizeof(unsigned);
    void *p[7];
    const int rc = scratch_carve(ctx, 0, bytes, 7, p, "nearest-neighbour scratch");
    if (rc) return rc;
    *sc = {CellTables::at(p), (unsigned *)p[4], (P *)p[5], (unsigned *)p[6]};
    return TL3D_OK;
}

// the queries bucketed into the target's grid (unless the context runs them in input order), then the search
template <class P, class Eval>
static int nn_search(tl3d_ctx *ctx, const CellGrid &g, const float *query, long long nq, const NnScratch<P> &sc, const Eval &eval, double max_dist,
                     double *dist, int *index) {
    hipStream_t s = ctx->stream;
    const unsigned nb = (unsigned)((nq + 255) / 256);
    const unsigned *ord = nullptr;
    if (!ctx->nn_input_order) {            // a second build over the target's cnt, which its fill counted down to zero again
        CellTables q = sc.t;
        q.start = sc.q_start;
        const int rc = cell_index_build(s, g, query, nq, q, false, EmitIndex{sc.order});
        if (rc) return rc;
        ord = sc.order;
    }
    hipLaunchKernelGGL(nn_search_kernel<Eval>, dim3(nb), dim3(256), 0, s, g, query, nq, ord, sc.t.start, eval, max_dist, dist, index);
    NN_HIP(hipGetLastError());
    return TL3D_OK;
}

static int nn_fill_none(tl3d_ctx *ctx, long long nq, double *dist, int *index) {
    hipLaunchKernelGGL(nn_none_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, nq, dist, index);
    NN_HIP(hipGetLastError());
    return TL3D_OK;
}

// every pointer is device memory; dist / index may be null
int nearest_points_run(tl3d_ctx *ctx, const float *query, long long nq, const float *target, long long nt, double cell, double max_dist,
                       double *dist, int *index) {
    hipStream_t s = ctx->stream;
    int rc = cell_slab(ctx);
    if (rc) return rc;
    float *slab = (float *)ctx->cg_slab;
    std::vector<float> h((size_t)NN_RED * 16);
    nn_bounds_launch(s, query, nq, slab);
    if (nt) nn_bounds_launch(s, target, nt, slab + (size_t)NN_RED * 8);
    NN_HIP(hipGetLastError());
    NN_HIP(hipMemcpyAsync(h.data(), slab, h.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    NN_HIP(hipStreamSynchronize(s));
    double mn[3], mx[3];
    unsigned long long bad = nn_bounds_fold(h.data(), nq, mn, mx);
    if (bad) return set_err(TL3D_E_INVALID, "%llu query points have a non-finite coordinate", bad);
    if (nt == 0) return nn_fill_none(ctx, nq, dist, index);
    bad = nn_bounds_fold(h.data() + (size_t)NN_RED * 8, nt, mn, mx);
    if (bad) return set_err(TL3D_E_INVALID, "%llu target points have a non-finite coordinate", bad);
    if (!(cell > 0.0)) cell = nn_default_cell_points(mn, mx, nt);
    CellGrid g;
    cell_grid_fit(mn, mx, cell, &g);
    NnScratch<float4> sc;
    rc = nn_scratch(ctx, cell_grid_cells(g), (size_t)nt, nq, &sc);
    if (rc) return rc;
    rc = cell_index_build(s, g, target, nt, sc.t, true, EmitPointIndex{sc.payload});
    if (rc) return rc;
    const NnPointEval pe = {sc.payload};
    return nn_search(ctx, g, query, nq, sc, pe, max_dist, dist, index);
}

// The (triangle, cell) pair list is bounded: the cell doubles until the list has at most NN_PAIR_CAP(n_tri) = min(16 n_tri + 2^20, 2^31)
// entries (4 B each).  A mesh of even triangles needs ~4 per triangle at the default cell; the 2^20 lets a small mesh keep a fine grid
// under one large triangle; one cell needs n_tri < 2^31 entries, so the doubling ends.
static unsigned long long nn_pair_cap(long long n_tri) { return std::min(16ull * (unsigned long long)n_tri + (1ull << 20), 1ull << 31); }

int nearest_triangles_run(tl3d_ctx *ctx, const float *query, long long nq, const float *xyz, long long nv, const unsigned *tri, long long n_tri,
                          double cell, double max_dist, double *dist, int *index) {
    hipStream_t s = ctx->stream;
    int rc = cell_slab(ctx);
    if (rc) return rc;
    float *slab = (float *)ctx->cg_slab;
    double *tslab = (double *)(slab + (size_t)NN_RED * 16);
    unsigned long long *totals = (unsigned long long *)(tslab + (size_t)NN_RED * 2);       // [NN_LEVELS]
    std::vector<float> h((size_t)NN_RED * 16);
    std::vector<double> ht((size_t)NN_RED * 2);
    nn_bounds_launch(s, query, nq, slab);
    if (nv) nn_bounds_launch(s, xyz, nv, slab + (size_t)NN_RED * 8);
    if (n_tri) hipLaunchKernelGGL(nn_tri_stats_kernel, dim3(nn_red_blocks(n_tri)), dim3(256), 0, s, xyz, nv, tri, n_tri, tslab);
    NN_HIP(hipGetLastError());
    NN_HIP(hipMemcpyAsync(h.data(), slab, h.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    NN_HIP(hipMemcpyAsync(ht.data(), tslab, ht.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    NN_HIP(hipStreamSynchronize(s));
    double mn[3], mx[3];
    unsigned long long bad = nn_bounds_fold(h.data(), nq, mn, mx);
    if (bad) return set_err(TL3D_E_INVALID, "%llu query points have a non-finite coordinate", bad);
    if (nv) {
        bad = nn_bounds_fold(h.data() + (size_t)NN_RED * 8, nv, mn, mx);
        if (bad) return set_err(TL3D_E_INVALID, "%llu vertices have a non-finite coordinate", bad);
    }
    double ext = 0.0, oob = 0.0;
    if (n_tri)
        for (unsigned b = 0; b < nn_red_blocks(n_tri); ++b) { ext += ht[2 * b]; oob += ht[2 * b + 1]; }
    if (oob > 0.0) return set_err(TL3D_E_INVALID, "%.0f triangles have an index out of range [0, %lld)", oob, nv);
    if (n_tri == 0) return nn_fill_none(ctx, nq, dist, index);
    // default cell: the mean over the triangles of their box's largest extent
    if (!(cell > 0.0)) {
        cell = ext / (double)n_tri;
        if (!(cell > 0.0) || !isfinite(cell)) cell = 1.0;
    }
    CellGrid g;
    const unsigned long long cap = nn_pair_cap(n_tri);
    const unsigned ntb = (unsigned)((n_tri + 255) / 256);
    unsigned long long npairs = 0;
    for (bool found = false; !found;) {
        NnLevels lv;
        bool ok[NN_LEVELS];
        for (int j = 0; j < NN_LEVELS; ++j) {
            ok[j] = cell_grid_make(mn, mx, ldexp(cell, j), &lv.g[j]);
            if (!ok[j]) lv.g[j].nx = lv.g[j].ny = lv.g[j].nz = 1;       // not a candidate: counted as one cell, never chosen
        }
        unsigned long long got[NN_LEVELS];
        NN_HIP(hipMemsetAsync(totals, 0, sizeof(got), s));
        hipLaunchKernelGGL(nn_tri_pairs_kernel, dim3(ntb), dim3(256), 0, s, lv, xyz, tri, n_tri, totals);
        NN_HIP(hipGetLastError());
        NN_HIP(hipMemcpyAsync(got, totals, sizeof(got), hipMemcpyDeviceToHost, s));
        NN_HIP(hipStreamSynchronize(s));
        for (int j = 0; j < NN_LEVELS && !found; ++j)
            if (ok[j] && got[j] <= cap) { g = lv.g[j]; npairs = got[j]; found = true; }
        cell = ldexp(cell, NN_LEVELS);
    }
    const long long ncell = cell_grid_cells(g);
    NnScratch<unsigned> sc;
    rc = nn_scratch(ctx, ncell, (size_t)npairs, nq, &sc);
    if (rc) return rc;
    // cell_index_build's sequence with nn_tri_bin_kernel as count and fill: a triangle goes into every cell of its box
    NN_HIP(hipMemsetAsync(sc.t.cnt, 0, ncell * sizeof(unsigned), s));
    hipLaunchKernelGGL(nn_tri_bin_kernel, dim3(ntb), dim3(256), 0, s, g, xyz, tri, n_tri, (const unsigned *)nullptr, sc.t.cnt, (unsigned *)nullptr);
    rc = launch_cell_scan(s, sc.t.cnt, ncell, sc.t.chunk_sums, sc.t.chunk_off, sc.t.start);
    if (rc) return rc;
    hipLaunchKernelGGL(nn_tri_bin_kernel, dim3(ntb), dim3(256), 0, s, g, xyz, tri, n_tri, (const unsigned *)sc.t.start, sc.t.cnt, sc.payload);
    const NnTriEval te = {sc.payload, xyz, tri};
    return nn_search(ctx, g, query, nq, sc, te, max_dist, dist, index);
}

// dist: device memory.  The block partials are added in block order on the host: the same input gives the same bytes.
int distance_summary_run(tl3d_ctx *ctx, const double *dist, long long n, const double *thresholds, int nthr, tl3d_distance_stats *out) {
    hipStream_t s = ctx->stream;
    int rc = cell_slab(ctx);
    if (rc) return rc;
    unsigned long long *slab = (unsigned long long *)ctx->cg_slab;          // [NN_RED][16]
    NnThr thr;
    for (int j = 0; j < 8; ++j) thr.t[j] = j < nthr ? thresholds[j] : 0.0;
    const unsigned nb = nn_red_blocks(n);
    hipLaunchKernelGGL(nn_summary_kernel, dim3(nb), dim3(256), 0, s, dist, n, nthr, thr, slab);
    NN_HIP(hipGetLastError());
    std::vector<unsigned long long> h((size_t)nb * 16);
    NN_HIP(hipMemcpyAsync(h.data(), slab, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    NN_HIP(hipStreamSynchronize(s));
    for (unsigned b = 0; b < nb; ++b) {
        const unsigned long long *r = h.data() + 16 * (size_t)b;
        double v[3];
        memcpy(v, r + 9, sizeof(v));
        out->n_finite += (int64_t)r[0];
        for (int j = 0; j < nthr; ++j) out->below[j] += (int64_t)r[1 + j];
        out->sum += v[0];
        out->sum_sq += v[1];
        out->max = fmax(out->max, v[2]);
    }
    return TL3D_OK;
}

}  // namespace tl3d
