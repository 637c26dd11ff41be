// kernels_raycast.hip -- ray-casting the TSDF channel from one camera (tl3d_raycast).
//   One ray per pixel of the context's camera; a wave takes an 8 x 8 pixel tile (neighbouring rays gather neighbouring records).
//   Everything is f32 with -ffp-contract=off, in the order written here: tests/raycast_reference.py restates it bit for bit.
//   Grid coordinates: voxel (i, j, k) has its centre at x = (i, j, k); x(z) = cg + z * dg, z the camera depth.
//   t(v) = (float)sum / ((float)w * 32767) through tsdf_record (free-space counts included); v is usable when w >= mw.
//   F(x): trilinear over the 8 voxel centres around x, DEFINED only when all 8 are inside the grid and usable.
//   March: z from max(z_near, entry) while z <= min(z_far, exit) (the ray against the box [0, n - 1]^3 of voxel centres), at
//   most RAY_MAX_STEPS samples.  Step: max(vs / 2, 0.8 * trunc * F) where F is defined, vs where it is not.  The first defined
//   sample with F <= 0 ends the ray: a hit when the sample before it was defined (then F > 0 there), z* = z_k + (dz_k * F_k) /
//   (F_k - F_k+1); no hit otherwise (the ray started behind or inside a surface, or came out of unobserved space behind one).
#include "tl3d_internal.h"
#include "tsdf_cell.h"

namespace tl3d {

constexpr int RAY_MAX_STEPS = 4096;

struct RayArgs {
    float r[9];                  // world->camera rotation (row-major), rotates the normals
    float c[3];                  // camera centre in the world, -R^T t (computed in fp64, rounded)
    float ivs;                   // (float)(1 / voxel size), fp64 quotient rounded
    float half_vs, step_k;       // 0.5f * vs, 0.8f * trunc
    float z_near, z_far;
    int mw;                      // max(1, min_weight)
    float *depth, *depth2;       // [H][W] (either may be null; depth2: a frame slot)
    float *nrm;                  // [H][W][3]
    uint8_t *bgr, *bgr2;         // [H][W][3]
};

// BrickCache, corner_record, load_cell, lerpf, trilinear and trilinear_dx / dy / dz -- the cell gather and the field -- live in
// tsdf_cell.h (shared with kernels_track.hip)

__global__ __launch_bounds__(256) void raycast_kernel(Cam cam, Grid g, RayArgs a, const int2 *__restrict__ pool,
                                                      const unsigned long long *__restrict__ cen) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int u = blockIdx.x * 16 + (wid & 1) * 8 + (lane & 7);
    const int v = blockIdx.y * 16 + (wid >> 1) * 8 + (lane >> 3);
    if (u >= cam.W || v >= cam.H) return;
    const float xf = ((float)u - cam.cx) / cam.fx, yf = ((float)v - cam.cy) / cam.fy;
    float cg[3], dg[3];
    const float org[3] = {g.ox, g.oy, g.oz};
    const int n[3] = {g.nx, g.ny, g.nz};
    float z0 = a.z_near, z1 = a.z_far;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const float d = (a.r[ax] * xf + a.r[3 + ax] * yf) + a.r[6 + ax];      // (R^T (xf, yf, 1))_ax
        cg[ax] = (a.c[ax] - org[ax]) * a.ivs - 0.5f;
        dg[ax] = d * a.ivs;
        const float hi = (float)(n[ax] - 1);
        if (dg[ax] != 0.0f) {
            const float ta = (0.0f - cg[ax]) / dg[ax], tb = (hi - cg[ax]) / dg[ax];
            z0 = fmaxf(z0, fminf(ta, tb));
            z1 = fminf(z1, fmaxf(ta, tb));
        } else if (!(cg[ax] >= 0.0f && cg[ax] <= hi)) {
            z1 = -1.0f;
        }
    }
    BrickCache bc{0xffffffffu, SLOT_EMPTY, 0u};
    float z = z0, zp = 0.0f, dzp = 0.0f, fp = 0.0f, hit = 0.0f;
    bool prev = false;
#pragma unroll 1
    for (int s = 0; s < RAY_MAX_STEPS && z <= z1; ++s) {
        const float x[3] = {cg[0] + z * dg[0], cg[1] + z * dg[1], cg[2] + z * dg[2]};
        float tc[8], f[3];
        const bool def = load_cell(g, pool, a.mw, x, tc, f, bc);
        float dz = g.vs;
        float F = 0.0f;
        if (def) {
            F = trilinear(tc, f);
            if (F <= 0.0f) {
                if (prev) hit = zp + (dzp * fp) / (fp - F);
                break;
            }
            dz = fmaxf(a.half_vs, F * a.step_k);
        }
        prev = def;
        fp = F;
        zp = z;
        dzp = dz;
        z = z + dz;
    }
    float nc[3] = {0.0f, 0.0f, 0.0f};
    uint8_t col[3] = {128, 128, 128};
    if (hit > 0.0f) {
        const float x[3] = {cg[0] + hit * dg[0], cg[1] + hit * dg[1], cg[2] + hit * dg[2]};
        float tc[8], f[3];
        if (load_cell(g, pool, a.mw, x, tc, f, bc)) {
            const float gx = trilinear_dx(tc, f), gy = trilinear_dy(tc, f), gz = trilinear_dz(tc, f);
            const float len2 = (gx * gx + gy * gy) + gz * gz;
            if (len2 > 1e-30f) {
                const float inv = 1.0f / sqrtf(len2);
                const float nw[3] = {gx * inv, gy * inv, gz * inv};
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) nc[ax] = (a.r[3 * ax] * nw[0] + a.r[3 * ax + 1] * nw[1]) + a.r[3 * ax + 2] * nw[2];
                if ((nc[0] * xf + nc[1] * yf) + nc[2] > 0.0f) { nc[0] = -nc[0]; nc[1] = -nc[1]; nc[2] = -nc[2]; }
            }
        }
        if (cen) {
            const float xv[3] = {x[0] + 0.5f, x[1] + 0.5f, x[2] + 0.5f};
            if (xv[0] >= 0.0f && xv[0] < (float)g.nx && xv[1] >= 0.0f && xv[1] < (float)g.ny && xv[2] >= 0.0f && xv[2] < (float)g.nz) {
                const unsigned long long *rec = cen_record(g, cen, vox_index((int)xv[0], (int)xv[1], (int)xv[2], g.nbx, g.nby));
                const unsigned long long cnt = rec ? rec[1] >> 32 : 0ull;
                if (cnt > 0) {
                    uint8_t rgb[3];
                    mean_colour(rec, cnt, rgb);
                    col[0] = rgb[2]; col[1] = rgb[1]; col[2] = rgb[0];
                }
            }
        }
    }
    const size_t p = (size_t)v * cam.W + u;
    if (a.depth) a.depth[p] = hit;
    if (a.depth2) a.depth2[p] = hit;
    if (a.nrm) { a.nrm[3 * p] = nc[0]; a.nrm[3 * p + 1] = nc[1]; a.nrm[3 * p + 2] = nc[2]; }
    if (a.bgr) { a.bgr[3 * p] = col[0]; a.bgr[3 * p + 1] = col[1]; a.bgr[3 * p + 2] = col[2]; }
    if (a.bgr2) { a.bgr2[3 * p] = col[0]; a.bgr2[3 * p + 1] = col[1]; a.bgr2[3 * p + 2] = col[2]; }
}

int launch_raycast(hipStream_t s, const Cam &cam, const Grid &g, const double R[9], const double t[3], int min_weight, float z_near,
                   float z_far, const int2 *tsdf, const unsigned long long *cen, float *depth, float *depth2, float *nrm, uint8_t *bgr,
                   uint8_t *bgr2) {
    RayArgs a;
    for (int i = 0; i < 9; ++i) a.r[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) a.c[i] = (float)(-((R[0 + i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]));
    a.ivs = (float)(1.0 / g.vsd);
    a.half_vs = 0.5f * g.vs;
    a.step_k = 0.8f * g.trunc;
    a.z_near = z_near;
    a.z_far = z_far;
    a.mw = min_weight < 1 ? 1 : min_weight;
    a.depth = depth; a.depth2 = depth2; a.nrm = nrm; a.bgr = bgr; a.bgr2 = bgr2;
    const dim3 grid((unsigned)((cam.W + 15) / 16), (unsigned)((cam.H + 15) / 16));
    hipLaunchKernelGGL(raycast_kernel, grid, dim3(256), 0, s, cam, g, a, tsdf, cen);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

}  // namespace tl3d
