// cellgrid.h -- the device half of the uniform cell index that the outlier filter's k-NN (kernels_sor.hip) and the nearest searches
// (kernels_nearest.hip) share: points are counting-sorted into the cells of a grid over their box.
//   count   cnt[c] += 1 per point of cell c (kernels_cellgrid.hip); cnt is zeroed by the CALLER in front of a call's first count
//   scan    start[c] = points in cells < c; start has ncell + 1 entries and start[ncell] is the total, so the run of cell c is
//           [start[c], start[c + 1]) for the last cell too, and a row of cells is one run (kernels_cellgrid.hip)
//   fill    cell_fill_kernel: a point takes slot start[c] + --cnt[c]; cnt is counted DOWN and is all zero again behind the fill,
//           ready for the next count of the same call (the searches bucket their queries with it); the order inside a cell is
//           whatever the atomics give, and no caller's result depends on it
// The host half (grid sizing, the launches, the context's scratch) is declared in tl3d_internal.h.
#pragma once
#include "tl3d_internal.h"

namespace tl3d {

struct CellGrid {
    double ox, oy, oz, cell, inv_cell;
    int nx, ny, nz;
};

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
struct EmitPointIndex {                 // the point and its index beside it (the searches' point target)
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

template <class Emit>
inline void launch_cell_fill(hipStream_t s, const CellGrid &g, const float *xyz, long long n, const unsigned *start, unsigned *cnt, const Emit &emit) {
    hipLaunchKernelGGL(cell_fill_kernel<Emit>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, xyz, n, start, cnt, emit);
}

}  // namespace tl3d
