// kernels_cellgrid.hip -- the host half of the uniform cell index (cellgrid.h): the finite bounds pass in front of every build, the
// grid of a cell size over a box, the count and the two-level scan of the cell counts that cell_index_build launches, and the slab
// of the calls that use the index (the outlier filter, the nearest searches, cloud normals, plane segmentation).
#include <math.h>

#include <algorithm>
#include <vector>

#include "cellgrid.h"

namespace tl3d {

static_assert((size_t)NN_RED * 128 <= CELL_SLAB_BYTES, "the block partials of every reduction of the index's callers fit the slab");

// ---- validation and bounds -----------------------------------------------------------------------------------------------------
// per block: min[3], max[3] over the finite points (f32), and the number of points with a non-finite coordinate (its bits in [6])
__global__ __launch_bounds__(256) void nn_bounds_kernel(const float *__restrict__ xyz, long long n, float *__restrict__ slab) {
    __shared__ float sm[4][7];
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    unsigned bad = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if (isfinite(x) && isfinite(y) && isfinite(z)) {
            mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
            mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
        } else {
            ++bad;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        for (int a = 0; a < 3; ++a) {
            mn[a] = fminf(mn[a], __shfl_down(mn[a], d));
            mx[a] = fmaxf(mx[a], __shfl_down(mx[a], d));
        }
        bad += __shfl_down(bad, d);
    }
    if ((threadIdx.x & 63) == 0) {
        float *w = sm[threadIdx.x >> 6];
        for (int a = 0; a < 3; ++a) { w[a] = mn[a]; w[3 + a] = mx[a]; }
        w[6] = __uint_as_float(bad);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float *o = slab + 8 * (size_t)blockIdx.x;
        unsigned b = 0;
        for (int a = 0; a < 3; ++a) {
            o[a] = fminf(fminf(sm[0][a], sm[1][a]), fminf(sm[2][a], sm[3][a]));
            o[3 + a] = fmaxf(fmaxf(sm[0][3 + a], sm[1][3 + a]), fmaxf(sm[2][3 + a], sm[3][3 + a]));
        }
        for (int w = 0; w < 4; ++w) b += __float_as_uint(sm[w][6]);
        o[6] = __uint_as_float(b);
        o[7] = 0.0f;
    }
}

unsigned nn_red_blocks(long long n) { return (unsigned)std::max(1ll, std::min((long long)NN_RED, (n + 255) / 256)); }

void nn_bounds_launch(hipStream_t s, const float *xyz, long long n, float *slab) {
    hipLaunchKernelGGL(nn_bounds_kernel, dim3(nn_red_blocks(n)), dim3(256), 0, s, xyz, n, slab);
}
unsigned long long nn_bounds_fold(const float *h, long long n, double mn[3], double mx[3]) {
    unsigned long long bad = 0;
    for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; }
    for (unsigned b = 0; b < nn_red_blocks(n); ++b) {
        for (int a = 0; a < 3; ++a) {
            mn[a] = fmin(mn[a], (double)h[8 * b + a]);
            mx[a] = fmax(mx[a], (double)h[8 * b + 3 + a]);
        }
        unsigned w;
        memcpy(&w, h + 8 * b + 6, 4);
        bad += w;
    }
    return bad;
}

int points_bounds_finite(tl3d_ctx *ctx, const float *xyz, long long n, double mn[3], double mx[3], unsigned long long *bad) {
    hipStream_t s = ctx->stream;
    const int rc = cell_slab(ctx);
    if (rc) return rc;
    float *slab = (float *)ctx->cg_slab;
    std::vector<float> h((size_t)NN_RED * 8);
    nn_bounds_launch(s, xyz, n, slab);
    TL3D_HIP(hipGetLastError());
    TL3D_HIP(hipMemcpyAsync(h.data(), slab, h.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipStreamSynchronize(s));
    *bad = nn_bounds_fold(h.data(), n, mn, mx);
    return TL3D_OK;
}

// ---- count and scan ------------------------------------------------------------------------------------------------------------
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
