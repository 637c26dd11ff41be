// cellgrid.h -- the device half of the uniform cell index under the outlier filter (kernels_sor.hip), the
// nearest searches (kernels_nearest.hip), cloud normals (kernels_normals.hip) and plane segmentation (kernels_planes.hip): points
// are counting-sorted into the cells of a grid over their box.  A caller asks for the index in ONE call and walks it with ONE routine:
//   cell_index_build   memset (a call's first build), count, scan, fill over the caller's CellTables:
//     count   cnt[c] += 1 per point of cell c; cnt is all zero in front of it
//     scan    start[c] = points in cells < c; start has ncell + 1 entries and start[ncell] is the total, so the run of cell c is
//             [start[c], start[c + 1]) for the last cell too, and a row of cells is one run
//     fill    cell_fill_kernel: a point takes slot start[c] + --cnt[c]; cnt is counted DOWN and is all zero again behind the fill,
//             ready for a second build of the same call over the same cnt (the searches bucket their queries with it); the order
//             inside a cell is whatever the atomics give, and no caller's result depends on it
//   cell_shell_walk    the runs [s, e) of the sorted list in the cells of Chebyshev shell r around a cell
//   cell_face_bound    the stop rule of a walk: how near anything in the shells not yet walked can be (derived at cell_lower)
// The host half (grid sizing, the finite bounds pass in front of every build, the count and scan launches, the context's scratch) is
// kernels_cellgrid.hip, declared in tl3d_internal.h.
#pragma once
#include "tl3d_internal.h"

namespace tl3d {

struct CellGrid {
    double ox, oy, oz, cell, inv_cell;
    int nx, ny, nz;
};
inline long long cell_grid_cells(const CellGrid &g) { return (long long)g.nx * g.ny * g.nz; }

// ONE binning expression.  Everything that is binned -- the filter's points, the searches' targets, triangle corners and queries --
// goes through cell_u and cell_clampi.  cell_u is monotone in x (a rounded subtraction, then a rounded multiplication by a positive
// number), so "binned beyond a face" implies u beyond that face exactly: the stop rule of the nearest search rests on this.  The
// clamp is done in fp64 and then converted, so a coordinate far outside the box (or one whose u does not fit an int) lands in a
// border cell by defined arithmetic.  For a point inside the grid's box -- all the outlier filter ever bins -- floor(u) lies in
// [0, n - 1] already or is clamped to it from n (the box's upper face), which is what converting first and clamping the integer gave.
__device__ __forceinline__ double cell_u(double x, double o, double inv_cell) { return (x - o) * inv_cell; }
__device__ __forceinline__ int cell_clampi(double u, int n) { return (int)fmin(fmax(floor(u), 0.0), (double)(n - 1)); }
// linear index of p's cell, and its three coordinates
__device__ __forceinline__ long long cell_of(const CellGrid &g, const float *__restrict__ p, int &cx, int &cy, int &cz) {
    cx = cell_clampi(cell_u((double)p[0], g.ox, g.inv_cell), g.nx);
    cy = cell_clampi(cell_u((double)p[1], g.oy, g.inv_cell), g.ny);
    cz = cell_clampi(cell_u((double)p[2], g.oz, g.inv_cell), g.nz);
    return ((long long)cz * g.ny + cy) * g.nx + cx;
}
__device__ __forceinline__ long long cell_of(const CellGrid &g, const float *__restrict__ p) {
    int cx, cy, cz;
    return cell_of(g, p, cx, cy, cz);
}

// what a fill leaves at slot pos for point i (p: its three floats)
struct EmitPointIndex {                 // the point and its index beside it (the searches' point target, the normals' points)
    float4 *__restrict__ sorted;
    __device__ __forceinline__ void operator()(unsigned pos, long long i, const float *__restrict__ p) const {
        sorted[pos] = make_float4(p[0], p[1], p[2], __int_as_float((int)i));
    }
};
struct EmitIndex {                      // the index alone (the searches' query order)
    unsigned *__restrict__ order;
    __device__ __forceinline__ void operator()(unsigned pos, long long i, const float *__restrict__) const { order[pos] = (unsigned)i; }
};
struct EmitXyz {                        // three packed floats (the filter's sorted points)
    float *__restrict__ sorted;
    __device__ __forceinline__ void operator()(unsigned pos, long long, const float *__restrict__ p) const {
        sorted[3 * (size_t)pos + 0] = p[0];
        sorted[3 * (size_t)pos + 1] = p[1];
        sorted[3 * (size_t)pos + 2] = p[2];
    }
};

template <class Emit>
__global__ __launch_bounds__(256) void cell_fill_kernel(CellGrid g, const float *__restrict__ xyz, long long n, const unsigned *__restrict__ start,
                                                        unsigned *__restrict__ cnt, Emit emit) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long c = cell_of(g, xyz + 3 * i);
    emit(start[c] + atomicSub(cnt + c, 1u) - 1u, i, xyz + 3 * i);
}

// The index of xyz[n] over g into the tables t, emit's payload in slot order behind it.  zero_cnt: a call's first build; a second one
// over the same cnt (another start table) finds cnt zero behind the first one's fill.  Returns the scan's code.
template <class Emit>
inline int cell_index_build(hipStream_t s, const CellGrid &g, const float *xyz, long long n, const CellTables &t, bool zero_cnt, const Emit &emit) {
    const long long ncell = cell_grid_cells(g);
    if (zero_cnt) TL3D_HIP(hipMemsetAsync(t.cnt, 0, (size_t)ncell * sizeof(unsigned), s));
    launch_cell_count(s, g, xyz, n, t.cnt);
    const int rc = launch_cell_scan(s, t.cnt, ncell, t.chunk_sums, t.chunk_off, t.start);
    if (rc) return rc;
    hipLaunchKernelGGL(cell_fill_kernel<Emit>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, xyz, n, t.start, t.cnt, emit);
    return TL3D_OK;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------
// visit(s, e) for the runs [s, e) of the sorted list in the cells of Chebyshev shell r around cell (c0, c1, c2) of the grid, rows in
// ascending z, then y: a face row (z or y at distance r) is ONE run, start[row + lo] .. start[row + hi + 1] with its ends clamped to
// the grid; an interior row gives its two end cells, c0 - r then c0 + r, where they exist.  visit has ONE call site: a k-best insert
// of 64 entries is inlined once.  The loops run over OFFSETS from the cell: r and the grid are the same in every lane, so counters,
// face test and step are scalar and a lane's own registers hold only its cell (loops from a per-lane z0 to a per-lane z1 put every
// counter into vector registers: the filter's k-NN left its 96-register block with them).  Rows outside the grid are skipped; no
// offset beyond the grid's size is tried, so a shell costs at most four times the rows it has inside the grid.
template <class Visit>
__device__ __forceinline__ void cell_shell_walk(const CellGrid &g, const unsigned *__restrict__ start, int c0, int c1, int c2, int r, Visit &&visit) {
    const int rz = min(r, g.nz - 1), ry = min(r, g.ny - 1);            // beyond them a row lies outside the grid whatever the cell
    for (int dz = -rz; dz <= rz; ++dz)
        for (int dy = -ry; dy <= ry; ++dy) {
            const int z = c2 + dz, y = c1 + dy;
            if (z < 0 || z >= g.nz || y < 0 || y >= g.ny) continue;
            const unsigned row = ((unsigned)z * g.ny + y) * g.nx;
            const bool face = dz == -r || dz == r || dy == -r || dy == r;
            const int step = face ? 2 * r + 1 : 2 * r;                  // a face row: one run; an interior row: its two end cells
            for (int dx = -r; dx <= r; dx += step) {
                const int lo = max(c0 + dx, 0), hi = min(face ? c0 + r : c0 + dx, g.nx - 1);
                if (lo > hi) continue;
                visit(start[row + lo], start[row + hi + 1]);
            }
        }
}

// ---- the stop bound ------------------------------------------------------------------------------------------------------------
// After shell r the cells not yet walked lie beyond the OPEN faces of the walked cube [c - r, c + r]^3 (faces with grid cells behind
// them).  The walker's point may lie outside the grid (a search's query: a millimetre or a hundred diagonals), so "r shells walked
// = r * cell cleared" is false in general.  Whatever lies beyond the open face of axis a is at least gap_a away along a (the point's
// own coordinate to the face plane) and, being in the grid, at least box_b and box_c away along the other two (the point's distance
// to the grid's extent on that axis; 0 inside).  bound2 = min over the open faces of gap_a^2 + box_b^2 + box_c^2, and a walk may end
// when no face is open or when what it holds lies strictly under bound2 (a tie further out may have the smaller index).
// All of it in cell units u = (x - origin) * inv_cell, evaluated by ONE expression (cell_u) for what is binned and for who walks: it
// is monotone in x, so "binned beyond the face" implies u beyond the face exactly.  Turning cell units back into metres costs at
// most 4 roundings (2^-53 each, relative to the larger |u|), which CELL_SLACK = 1e-15 (4.5 of them) pays for: every bound is
// shrunk by it, which can only make a walk go one shell further.
constexpr double CELL_SLACK = 1e-15;
// metres that v cell units are worth at least; um: the largest |u| involved
__device__ __forceinline__ double cell_lower(double v, double um, double cell) {
    return fmax(0.0, v * cell * (1.0 - CELL_SLACK) - CELL_SLACK * cell * um);
}
// One axis of the bound behind shell r (u: the point's coordinate in cell units, c: its clamped cell, n: cells on the axis, nmax: the
// largest n + 1, other: box_b^2 + box_c^2 of the other two axes, 0.0 for a point inside the grid).  Scalars per axis, not arrays
// indexed by axis: those went to scratch in normals_kernel.
__device__ __forceinline__ void cell_face_bound(double u, int c, int r, int n, double nmax, double cell, double other, double &bound2, bool &open) {
    if (c - r > 0) {                                       // cells below c - r: u < c - r
        const double gap = cell_lower(u - (double)(c - r), nmax + fabs(u), cell);
        bound2 = fmin(bound2, gap * gap + other);
        open = true;
    }
    if (c + r < n - 1) {                                   // cells above c + r: u >= c + r + 1
        const double gap = cell_lower((double)(c + r + 1) - u, nmax + fabs(u), cell);
        bound2 = fmin(bound2, gap * gap + other);
        open = true;
    }
}

// ---- the k nearest of a point of the indexed list itself ------------------------------------------------------------------------------
// What cloud normals (kernels_normals.hip) and the FPFH descriptors (kernels_cloudglobal.hip) search with: the k <= KMAX best
// (d2, index) pairs around the point p of the sorted list (EmitPointIndex), in registers (ordered insert over static indices, as
// sor_knn_kernel's list); the order is the PAIR's, so neither the fill order inside a cell (atomics) nor the cell size shows in which
// points are kept or in the order they are listed.  The walk ends when no face of the walked cube has cells behind it, when the
// k-th pair's d2 lies strictly under the bound of everything not yet walked (a tie further out may have the smaller index), or when
// that bound exceeds md2 (the squared radius, INFINITY for none).  The bound is cell_face_bound's for a point inside the grid: the
// other axes add nothing.  bd / bi must come in as INFINITY / 0x7fffffff; entries the list does not reach stay so.
__device__ __forceinline__ bool knn_less(double a, int ai, double b, int bi) { return a < b || (a == b && ai < bi); }   // (a, ai) < (b, bi)

template <int KMAX>
__device__ __forceinline__ void cell_knn_search(const CellGrid &g, const unsigned *__restrict__ start, const float4 *__restrict__ sorted, double px,
                                                double py, double pz, int k, double md2, double (&bd)[KMAX], int (&bi)[KMAX]) {
    const double u0 = cell_u(px, g.ox, g.inv_cell), u1 = cell_u(py, g.oy, g.inv_cell), u2 = cell_u(pz, g.oz, g.inv_cell);
    const int c0 = cell_clampi(u0, g.nx), c1 = cell_clampi(u1, g.ny), c2 = cell_clampi(u2, g.nz);
    const double nmax = (double)max(g.nx, max(g.ny, g.nz)) + 1.0;
    for (int r = 0;; ++r) {
        cell_shell_walk(g, start, c0, c1, c2, r, [&](unsigned s, unsigned e) {
            for (unsigned q = s; q < e; ++q) {
                const float4 p = sorted[q];
                const double dx = (double)p.x - px, dy = (double)p.y - py, dz = (double)p.z - pz;
                double v = dx * dx + dy * dy + dz * dz;
                int vi = __float_as_int(p.w);
                if (knn_less(v, vi, bd[KMAX - 1], bi[KMAX - 1])) {
#pragma unroll
                    for (int j = 0; j < KMAX; ++j) {               // ordered insert, static indices -> registers
                        const double b = bd[j];
                        const int ib = bi[j];
                        const bool sw = knn_less(v, vi, b, ib);
                        bd[j] = sw ? v : b;
                        bi[j] = sw ? vi : ib;
                        v = sw ? b : v;
                        vi = sw ? ib : vi;
                    }
                }
            }
        });
        double bound2 = INFINITY;
        bool open = false;
        cell_face_bound(u0, c0, r, g.nx, nmax, g.cell, 0.0, bound2, open);
        cell_face_bound(u1, c1, r, g.ny, nmax, g.cell, 0.0, bound2, open);
        cell_face_bound(u2, c2, r, g.nz, nmax, g.cell, 0.0, bound2, open);
        double kth = INFINITY;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j == k - 1) kth = bd[j];
        if (!open || kth < bound2 || bound2 > md2) break;
    }
}

// ---- the nearest-point candidate ---------------------------------------------------------------------------------------------------
// what a nearest search keeps (kernels_nearest.hip, kernels_cloudicp.hip): the minimum over the pair (d2, index), and the evaluation
// of a run of a point target's sorted list against a query in fp64
struct NnBest {
    double d2;
    int idx;
    __device__ __forceinline__ void take(double v, int i) {
        if (v < d2 || (v == d2 && i < idx)) { d2 = v; idx = i; }
    }
};

struct NnPointEval {
    const float4 *__restrict__ sorted;
    __device__ __forceinline__ void operator()(unsigned s, unsigned e, double px, double py, double pz, NnBest &best) const {
        for (unsigned q = s; q < e; ++q) {
            const float4 t = sorted[q];
            const double dx = (double)t.x - px, dy = (double)t.y - py, dz = (double)t.z - pz;
            best.take(dx * dx + dy * dy + dz * dz, __float_as_int(t.w));
        }
    }
};

}  // namespace tl3d
