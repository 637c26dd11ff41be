// kernels_cellgrid.hip -- the host half of the uniform cell index (cellgrid.h): the grid of a cell size over a box, the count and
// the two-level scan of the cell counts, and the scratch of the calls that use the index (the outlier filter, the nearest searches).
#include <math.h>

#include "cellgrid.h"

namespace tl3d {

__global__ __launch_bounds__(256) void cell_count_kernel(CellGrid g, const float *__restrict__ xyz, long long n, unsigned *__restrict__ cnt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    atomicAdd(cnt + cell_of(g, xyz + 3 * i), 1u);
}

// block sums of 1024-element chunks
__global__ __launch_bounds__(256) void cell_chunk_sum_kernel(const unsigned *__restrict__ v, long long n, unsigned *__restrict__ sums) {
    __shared__ unsigned sm[4];
    const long long base = (long long)blockIdx.x * 1024;
    unsigned s = 0;
    for (int k = 0; k < 4; ++k) {
        const long long i = base + k * 256 + threadIdx.x;
        if (i < n) s += v[i];
    }
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

// exclusive scan inside each 1024-element chunk, offset by the scanned chunk sums; start[n] = the total
__global__ __launch_bounds__(256) void cell_chunk_scan_kernel(const unsigned *__restrict__ v, long long n,
                                                              const unsigned long long *__restrict__ chunk_off, int nchunks,
                                                              unsigned *__restrict__ start) {
    __shared__ unsigned sm[4];
    const long long i0 = (long long)blockIdx.x * 1024 + (long long)threadIdx.x * 4;
    unsigned a[4], s = 0;
    for (int k = 0; k < 4; ++k) { a[k] = (i0 + k < n) ? v[i0 + k] : 0u; s += a[k]; }
    unsigned inc = s;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) sm[wid] = inc;
    __syncthreads();
    unsigned run = (unsigned)chunk_off[blockIdx.x] + inc - s;
    for (int w = 0; w < wid; ++w) run += sm[w];
    for (int k = 0; k < 4; ++k) {
        if (i0 + k < n) start[i0 + k] = run;
        run += a[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) start[n] = (unsigned)chunk_off[nchunks];
}

// the grid of `cell` over [mn, mx]; false when it has more than 2^27 cells
bool cell_grid_make(const double mn[3], const double mx[3], double cell, CellGrid *g) {
    g->cell = cell;
    g->inv_cell = 1.0 / cell;
    g->ox = mn[0]; g->oy = mn[1]; g->oz = mn[2];
    const double ex = floor((mx[0] - mn[0]) / cell) + 1, ey = floor((mx[1] - mn[1]) / cell) + 1, ez = floor((mx[2] - mn[2]) / cell) + 1;
    if (!(ex * ey * ez <= 134217728.0)) return false;
    g->nx = (int)ex; g->ny = (int)ey; g->nz = (int)ez;
    return true;
}

// the first of cell, 2 cell, 4 cell, .. whose grid has at most 2^27 cells
void cell_grid_fit(const double mn[3], const double mx[3], double cell, CellGrid *g) {
    while (!cell_grid_make(mn, mx, cell, g)) cell *= 2.0;
}

void launch_cell_count(hipStream_t s, const CellGrid &g, const float *xyz, long long n, unsigned *cnt) {
    hipLaunchKernelGGL(cell_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, xyz, n, cnt);
}

// cnt[ncell] -> start[ncell + 1]; chunk_sums: cell_chunks(ncell) words, chunk_off: one more
int launch_cell_scan(hipStream_t s, const unsigned *cnt, long long ncell, unsigned *chunk_sums, unsigned long long *chunk_off, unsigned *start) {
    const int nchunks = (int)cell_chunks(ncell);
    hipLaunchKernelGGL(cell_chunk_sum_kernel, dim3(nchunks), dim3(256), 0, s, cnt, ncell, chunk_sums);
    const int rc = launch_scan(s, chunk_sums, chunk_off, nchunks, chunk_off + nchunks);
    if (rc) return rc;
    hipLaunchKernelGGL(cell_chunk_scan_kernel, dim3(nchunks), dim3(256), 0, s, cnt, ncell, chunk_off, nchunks, start);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// the fixed slab the callers' reductions leave their block partials in
int cell_slab(tl3d_ctx *ctx) {
    if (ctx->cg_slab) return TL3D_OK;
    if (hipMalloc(&ctx->cg_slab, CELL_SLAB_BYTES) != hipSuccess) {
        (void)hipGetLastError();
        ctx->cg_slab = nullptr;
        return set_err(TL3D_E_NOMEM, "nearest-neighbour slab alloc failed");
    }
    return TL3D_OK;
}

}  // namespace tl3d
