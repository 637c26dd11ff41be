// kernels_sor.hip -- row f1: statistical outlier removal with the semantics of Open3D
// remove_statistical_outlier as the reference calls it (depth_to_reconstruction.py:412-415, nb_neighbors=20,
// std_ratio=2.0): per point the mean distance to its k nearest neighbours (the point itself included, as the
// KNN search returns it), mu / sigma (Bessel-corrected) of those means, keep  0 < mean < mu + ratio*sigma.
// Restated in oracle/ref_numpy.py: statistical_outlier_open3d (Open3D itself: parity unpinned).
//
// Exact k-NN without a tree: points are counting-sorted into the uniform cell index of cellgrid.h (cell_index_build; cell ~ 2
// voxels); each point walks the shells around its cell (cell_shell_walk) and stops once its k-th best distance is inside the
// walked radius.  That rule is simpler than the bound of cellgrid.h (cell_face_bound) and valid here because every point lies
// inside the box it was binned over: it is IN its cell, so whatever lies outside the walked cube [c - r, c + r]^3 is at least r
// whole cells away along some axis.  (A search's query may lie outside the grid, where its clamped cell says nothing of the kind.)
// The list holds the k smallest squared distances, kept sorted by a strict <: its content does not depend on the order in which
// the walk meets the points.  Distances in fp64 (Open3D works on double points); the list lives in registers (static indexing).
#include <math.h>

#include <vector>

#include "api_host.h"
#include "cellgrid.h"

namespace tl3d {

template <int KMAX>
__global__ __launch_bounds__(256) void sor_knn_kernel(CellGrid cg, const float *__restrict__ xyz, long long n, int k,
                                                      const unsigned *__restrict__ cell_start,
                                                      const float *__restrict__ sorted_xyz, double *__restrict__ mean_d) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    int cx, cy, cz;
    cell_of(cg, xyz + 3 * i, cx, cy, cz);
    double best[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) best[j] = 1e300;
    const int rmax = max(cg.nx, max(cg.ny, cg.nz));
    for (int r = 0; r <= rmax; ++r) {
        cell_shell_walk(cg, cell_start, cx, cy, cz, r, [&](unsigned s, unsigned e) {
            for (unsigned q = s; q < e; ++q) {
                const double ddx = (double)sorted_xyz[3 * (size_t)q] - px, ddy = (double)sorted_xyz[3 * (size_t)q + 1] - py;
                const double ddz = (double)sorted_xyz[3 * (size_t)q + 2] - pz;
                double v = ddx * ddx + ddy * ddy + ddz * ddz;
                if (v < best[KMAX - 1]) {
#pragma unroll
                    for (int j = 0; j < KMAX; ++j) {                   // ordered insert, static indices -> registers
                        const double b = best[j];
                        const bool sw = v < b;
                        best[j] = sw ? v : b;
                        v = sw ? b : v;
                    }
                }
            }
        });
        // everything outside the walked cube is at least r*cell away (the head of the file)
        const double reach = (double)r * cg.cell;
        double kth = 1e300;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j == k - 1) kth = best[j];
        if (kth <= reach * reach) break;
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < k) s += sqrt(best[j]);
    mean_d[i] = s / (double)k;
}

// pass 0: count and sum of the positive means; pass 1: sum of squared deviations; pass 2: write the mask
__global__ __launch_bounds__(256) void sor_stat_kernel(const double *__restrict__ mean_d, long long n, int pass, double mu,
                                                       double thr, double *__restrict__ slab, uint8_t *__restrict__ keep) {
    __shared__ double sm[4][2];
    double a = 0.0, b = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double m = mean_d[i];
        if (pass == 0) {
            if (m > 0.0) { a += 1.0; b += m; }
        } else if (pass == 1) {
            if (m > 0.0) { const double d = m - mu; a += d * d; }
        } else {
            const bool kp = (m > 0.0) && (m < thr);
            keep[i] = kp ? 1 : 0;
            if (kp) a += 1.0;
        }
    }
    for (int d = 32; d > 0; d >>= 1) { a += __shfl_down(a, d); b += __shfl_down(b, d); }
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = a; sm[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        slab[2 * blockIdx.x] = ((sm[0][0] + sm[1][0]) + sm[2][0]) + sm[3][0];
        slab[2 * blockIdx.x + 1] = ((sm[0][1] + sm[1][1]) + sm[2][1]) + sm[3][1];
    }
}

// the mean-distance stage alone: (*mean_d)[i] (device, n doubles) = mean fp64 distance of point i to its min(k, n) nearest
// neighbours, itself included.  tl3d_knn_mean_distance returns it as it is; sor_run thresholds it.  *mean_d == nullptr: the n
// doubles come out of the call's carve too, and *mean_d is set to them.
int sor_mean_distance(tl3d_ctx *ctx, const float *xyz, long long n, int k, double cell, double **mean_d) {
    hipStream_t s = ctx->stream;
    if (k > n) k = (int)n;
    double mn[3], mx[3];
    int rc = tl3d_points_bounds(ctx, xyz, n, mn, mx);
    if (rc) return rc;
    CellGrid cg;
    cell_grid_fit(mn, mx, cell, &cg);
    size_t bytes[6];
    cell_table_bytes(cell_grid_cells(cg), bytes);
    bytes[4] = (size_t)n * 3 * sizeof(float);
    bytes[5] = *mean_d ? 0 : (size_t)n * sizeof(double);
    void *p[6];
    rc = scratch_carve(ctx, 0, bytes, 6, p, "nearest-neighbour scratch");
    if (rc) return rc;
    const CellTables t = CellTables::at(p);
    const unsigned *start = t.start;
    float *sorted = (float *)p[4];
    if (!*mean_d) *mean_d = (double *)p[5];
    rc = cell_index_build(s, cg, xyz, n, t, true, EmitXyz{sorted});
    if (rc) return rc;
    const unsigned nb = (unsigned)((n + 255) / 256);
    if (k <= 32)
        hipLaunchKernelGGL(sor_knn_kernel<32>, dim3(nb), dim3(256), 0, s, cg, xyz, n, k, start, sorted, *mean_d);
    else
        hipLaunchKernelGGL(sor_knn_kernel<64>, dim3(nb), dim3(256), 0, s, cg, xyz, n, k, start, sorted, *mean_d);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

int sor_run(tl3d_ctx *ctx, const float *xyz, long long n, int k, double std_ratio, double cell, uint8_t *keep, long long *kept) {
    hipStream_t s = ctx->stream;
    const int nred = 1024;
    static_assert(2 * nred * sizeof(double) <= CELL_SLAB_BYTES, "the block partials fit the slab");
    std::vector<double> h(2 * nred);
    double m = 0, sum = 0, mu = 0, sq = 0, sigma = 0, thr = 0, cnt = 0;
    double *mean_d = nullptr;
    int rc = cell_slab(ctx);
    if (!rc) rc = sor_mean_distance(ctx, xyz, n, k, cell, &mean_d);
    if (rc) return rc;
    double *slab = (double *)ctx->cg_slab;
    // mu, sigma over the positive means (fixed-order sums of the block partials)
    hipLaunchKernelGGL(sor_stat_kernel, dim3(nred), dim3(256), 0, s, mean_d, n, 0, 0.0, 0.0, slab, keep);
    TL3D_HIP(hipMemcpyAsync(h.data(), slab, 2 * nred * sizeof(double), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < nred; ++i) { m += h[2 * i]; sum += h[2 * i + 1]; }
    if (m > 1.0) {
        mu = sum / m;
        hipLaunchKernelGGL(sor_stat_kernel, dim3(nred), dim3(256), 0, s, mean_d, n, 1, mu, 0.0, slab, keep);
        TL3D_HIP(hipMemcpyAsync(h.data(), slab, 2 * nred * sizeof(double), hipMemcpyDeviceToHost, s));
        TL3D_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < nred; ++i) sq += h[2 * i];
        sigma = sqrt(sq / (m - 1.0));
        thr = mu + std_ratio * sigma;
    } else {
        thr = INFINITY;                         // <= 1 valid point: keep every point with a positive mean
    }
    hipLaunchKernelGGL(sor_stat_kernel, dim3(nred), dim3(256), 0, s, mean_d, n, 2, mu, thr, slab, keep);
    TL3D_HIP(hipMemcpyAsync(h.data(), slab, 2 * nred * sizeof(double), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < nred; ++i) cnt += h[2 * i];
    *kept = (long long)cnt;
    return TL3D_OK;
}

}  // namespace tl3d
