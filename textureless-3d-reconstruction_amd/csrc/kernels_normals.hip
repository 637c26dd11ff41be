// kernels_normals.hip -- normals and surface variation of a point list by PCA over each point's k nearest neighbours (DESIGN.md
// section 4.5; tl3d_estimate_normals in tl3d.h has the definition).  No reference code: the reference writes positions and colours
// only; the definition is the one of Open3D's estimate_normals + orient_normals_towards_camera_location and of PCL's surface variation.
//
// The points are counting-sorted into the uniform cell index of cellgrid.h over their own box (cell_index_build), as float4 with the
// original index beside the point.  Thread t serves the point in slot t of that sorted list, so the lanes of a wave are neighbours in
// space and walk the same few cells; the result is scattered back by the original index.  (The sorted list IS the cell order of the
// queries: the second build that the searches of kernels_nearest.hip need for a foreign query set has nothing to add here.)
//   search   cell_knn_search (cellgrid.h, shared with the FPFH descriptors): the shells of growing Chebyshev radius around the
//            point's cell, the k best (d2, index) pairs in registers; the order is the PAIR's, so neither the fill order inside a
//            cell nor the cell size shows in which points are kept or in the order they are summed in.
//   PCA      e_j = p_j - p_i fetched again by index (twice: mean, then centred products; the list cannot hold 64 points beside the
//            pairs), all in fp64 in list order; sym3_eigen.h solves the 3x3.
//   sign     the viewpoints pass through LDS in chunks of 256; nearest by (d2, index); n . (c - p) < 0 negates.
#include <math.h>

#include "api_host.h"
#include "cellgrid.h"
#include "sym3_eigen.h"

namespace tl3d {

constexpr int NRM_VP_CHUNK = 256;       // viewpoints per LDS chunk (one per thread of the block: 6 KB)

template <int KMAX>
__global__ __launch_bounds__(256) void normals_kernel(CellGrid g, const float *__restrict__ xyz, long long n, int k, double md2,
                                                      const unsigned *__restrict__ start, const float4 *__restrict__ sorted,
                                                      const double *__restrict__ vp, int n_vp, float *__restrict__ normal_out,
                                                      float *__restrict__ curv_out, unsigned long long *__restrict__ n_degenerate) {
    __shared__ double sm_vp[NRM_VP_CHUNK * 3];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < n;                               // every thread of the block stays for the barriers of the viewpoint chunks
    const float4 me = sorted[live ? t : 0];
    const int qi = __float_as_int(me.w);
    const double px = (double)me.x, py = (double)me.y, pz = (double)me.z;

    double bd[KMAX];
    int bi[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { bd[j] = INFINITY; bi[j] = 0x7fffffff; }

    if (live) cell_knn_search<KMAX>(g, start, sorted, px, py, pz, k, md2, bd, bi);

    // the neighbourhood: the first k entries that exist and lie within the radius (the list is ordered: they are a prefix)
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < k && bi[j] != 0x7fffffff && bd[j] <= md2) ++cnt;
    double sx = 0.0, sy = 0.0, sz = 0.0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < cnt) {
            const float *q = xyz + 3 * (size_t)bi[j];
            sx += (double)q[0] - px; sy += (double)q[1] - py; sz += (double)q[2] - pz;
        }
    const double kk = (double)cnt;
    const double mx = sx / kk, my = sy / kk, mz = sz / kk;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < cnt) {
            const float *q = xyz + 3 * (size_t)bi[j];
            const double dx = ((double)q[0] - px) - mx, dy = ((double)q[1] - py) - my, dz = ((double)q[2] - pz) - mz;
            a[0] += dx * dx; a[1] += dy * dy; a[2] += dz * dz;
            a[3] += dx * dy; a[4] += dx * dz; a[5] += dy * dz;
        }
    double lam[3] = {0.0, 0.0, 0.0}, nv[3] = {0.0, 0.0, 0.0};
    bool degenerate = cnt < 3;
    if (!degenerate) {
        sym3_smallest(a, lam, nv);
        degenerate = !(lam[2] > 0.0);
    }
    double curv = 0.0;
    if (degenerate) {
        nv[0] = nv[1] = nv[2] = 0.0;
    } else {
        const double sum = (lam[0] + lam[1]) + lam[2];
        if (sum != 0.0) curv = lam[0] / sum;
    }

    // the nearest viewpoint by (d2, index): chunks are met in index order, so a strict < keeps the smaller index
    if (n_vp > 0) {
        double best = INFINITY, cx = 0.0, cy = 0.0, cz = 0.0;
        for (int base = 0; base < n_vp; base += NRM_VP_CHUNK) {
            const int m = min(NRM_VP_CHUNK, n_vp - base);
            __syncthreads();
            if ((int)threadIdx.x < m) {
                sm_vp[3 * threadIdx.x + 0] = vp[3 * (size_t)(base + threadIdx.x) + 0];
                sm_vp[3 * threadIdx.x + 1] = vp[3 * (size_t)(base + threadIdx.x) + 1];
                sm_vp[3 * threadIdx.x + 2] = vp[3 * (size_t)(base + threadIdx.x) + 2];
            }
            __syncthreads();
            for (int j = 0; j < m; ++j) {
                const double dx = sm_vp[3 * j] - px, dy = sm_vp[3 * j + 1] - py, dz = sm_vp[3 * j + 2] - pz;
                const double d2 = dx * dx + dy * dy + dz * dz;
                if (d2 < best) { best = d2; cx = dx; cy = dy; cz = dz; }
            }
        }
        if (nv[0] * cx + nv[1] * cy + nv[2] * cz < 0.0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
    }

    if (live) {
        normal_out[3 * (size_t)qi + 0] = (float)nv[0];
        normal_out[3 * (size_t)qi + 1] = (float)nv[1];
        normal_out[3 * (size_t)qi + 2] = (float)nv[2];
        if (curv_out) curv_out[qi] = (float)curv;
    }
    const unsigned long long deg = __popcll(__ballot(live && degenerate));
    if ((threadIdx.x & 63) == 0 && deg) atomicAdd(n_degenerate, deg);      // integer adds: the same total in every run
}

// every pointer is device memory but vp_host; curvature may be null.  *degenerate: the count, read back behind the kernel.
int normals_run(tl3d_ctx *ctx, const float *xyz, long long n, int k, double max_radius, double cell, const double *vp_host, long long n_vp,
                float *normal, float *curvature, long long *degenerate) {
    hipStream_t s = ctx->stream;
    if (k > n) k = (int)n;
    double mn[3], mx[3];
    unsigned long long bad = 0;
    int rc = points_bounds_finite(ctx, xyz, n, mn, mx, &bad);
    if (rc) return rc;
    if (bad) return set_err(TL3D_E_INVALID, "%llu points have a non-finite coordinate", bad);
    CellGrid g;
    cell_grid_fit(mn, mx, cell, &g);
    size_t bytes[7];
    cell_table_bytes(cell_grid_cells(g), bytes);
    bytes[4] = (size_t)n * sizeof(float4);
    bytes[5] = (size_t)n_vp * 3 * sizeof(double);
    bytes[6] = sizeof(unsigned long long);
    void *p[7];
    rc = scratch_carve(ctx, 0, bytes, 7, p, "normal estimation scratch");
    if (rc) return rc;
    const CellTables t = CellTables::at(p);
    const unsigned *start = t.start;
    float4 *sorted = (float4 *)p[4];
    double *vp = (double *)p[5];
    unsigned long long *n_deg = (unsigned long long *)p[6];
    TL3D_HIP(hipMemsetAsync(n_deg, 0, sizeof(unsigned long long), s));
    if (n_vp) TL3D_HIP(hipMemcpyAsync(vp, vp_host, (size_t)n_vp * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    rc = cell_index_build(s, g, xyz, n, t, true, EmitPointIndex{sorted});
    if (rc) return rc;
    const unsigned nb = (unsigned)((n + 255) / 256);
    const double md2 = max_radius > 0.0 ? max_radius * max_radius : INFINITY;
    if (k <= 32)
        hipLaunchKernelGGL(normals_kernel<32>, dim3(nb), dim3(256), 0, s, g, xyz, n, k, md2, start, sorted, vp, (int)n_vp, normal, curvature, n_deg);
    else
        hipLaunchKernelGGL(normals_kernel<64>, dim3(nb), dim3(256), 0, s, g, xyz, n, k, md2, start, sorted, vp, (int)n_vp, normal, curvature, n_deg);
    TL3D_HIP(hipGetLastError());
    unsigned long long h = 0;
    TL3D_HIP(hipMemcpyAsync(&h, n_deg, sizeof(h), hipMemcpyDeviceToHost, s));
    TL3D_HIP(hipStreamSynchronize(s));          // (also: the viewpoints' upload has left the caller's host array)
    *degenerate = (long long)h;
    return TL3D_OK;
}

}  // namespace tl3d
