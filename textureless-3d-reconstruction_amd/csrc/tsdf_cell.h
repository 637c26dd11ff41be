// tsdf_cell.h -- the trilinear cell of the TSDF channel around a point in grid coordinates: the 8-record gather, the field and its
// analytic gradient.  Shared by the ray caster (kernels_raycast.hip: samples along a ray) and the point-to-SDF tracker
// (kernels_track.hip: the residual and the normal of a back-projected pixel), so that both read the same records under the same
// rule -- tsdf_record's free-space counts included -- and evaluate the same f32 expressions in the same order
// (-ffp-contract=off; tests/raycast_reference.py and tests/track_reference.py restate them bit for bit).
//   Grid coordinates: voxel (i, j, k) has its centre at x = (i, j, k).
//   t(v) = (float)sum / ((float)w * 32767); v is usable when w >= mw.
//   F(x): trilinear over the 8 voxel centres around x, DEFINED only when all 8 are inside the grid and usable.
#pragma once
#include "tl3d_internal.h"

namespace tl3d {

// one-entry cache of a brick's pool slot and pending free-space count: about two in three corner cubes lie in one brick
struct BrickCache {
    unsigned brick, slot, fc;
};

__device__ __forceinline__ int2 corner_record(const Grid &g, const int2 *__restrict__ pool, int i, int j, int k, BrickCache &bc) {
    const unsigned brick = (unsigned)((((size_t)(k >> 3) * (size_t)g.nby + (size_t)(j >> 3)) * (size_t)g.nbx) + (size_t)(i >> 3));
    if (brick != bc.brick) {
        bc.brick = brick;
        bc.slot = brick_slot(g.tsdf_tab, brick);
        bc.fc = g.free_cnt ? g.free_cnt[brick] : 0u;
    }
    int2 r = make_int2(0, 0);
    if (bc.slot < SLOT_FULL) r = pool[((size_t)bc.slot << 9) | (size_t)in_brick_index(i, j, k)];
    r.x += (int)(bc.fc * 32767u);
    r.y += (int)bc.fc;
    return r;
}

// the 8 corner values of the cell whose lowest corner is floor(x); false when the cell is not inside the grid or a corner
// is not usable.  f: the fractions x - floor(x).
__device__ __forceinline__ bool load_cell(const Grid &g, const int2 *__restrict__ pool, int mw, const float x[3], float tc[8],
                                          float f[3], BrickCache &bc) {
    if (!(x[0] >= 0.0f && x[0] < (float)(g.nx - 1) && x[1] >= 0.0f && x[1] < (float)(g.ny - 1) && x[2] >= 0.0f &&
          x[2] < (float)(g.nz - 1)))
        return false;
    const int i = (int)x[0], j = (int)x[1], k = (int)x[2];
    f[0] = x[0] - (float)i;
    f[1] = x[1] - (float)j;
    f[2] = x[2] - (float)k;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int2 r = corner_record(g, pool, i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1), bc);
        ok = ok && r.y >= mw;
        tc[c] = (float)r.x / ((float)r.y * 32767.0f);
    }
    return ok;
}

__device__ __forceinline__ float lerpf(float a, float b, float t) { return a + t * (b - a); }

__device__ __forceinline__ float trilinear(const float tc[8], const float f[3]) {
    const float c00 = lerpf(tc[0], tc[1], f[0]), c10 = lerpf(tc[2], tc[3], f[0]);
    const float c01 = lerpf(tc[4], tc[5], f[0]), c11 = lerpf(tc[6], tc[7], f[0]);
    return lerpf(lerpf(c00, c10, f[1]), lerpf(c01, c11, f[1]), f[2]);
}

// the analytic gradient of the trilinear field at the fractions f, per voxel (not normalised), component by component
__device__ __forceinline__ float trilinear_dx(const float tc[8], const float f[3]) {
    return lerpf(lerpf(tc[1] - tc[0], tc[3] - tc[2], f[1]), lerpf(tc[5] - tc[4], tc[7] - tc[6], f[1]), f[2]);
}
__device__ __forceinline__ float trilinear_dy(const float tc[8], const float f[3]) {
    return lerpf(lerpf(tc[2] - tc[0], tc[3] - tc[1], f[0]), lerpf(tc[6] - tc[4], tc[7] - tc[5], f[0]), f[2]);
}
__device__ __forceinline__ float trilinear_dz(const float tc[8], const float f[3]) {
    return lerpf(lerpf(tc[4] - tc[0], tc[5] - tc[1], f[0]), lerpf(tc[6] - tc[2], tc[7] - tc[3], f[0]), f[1]);
}

}  // namespace tl3d
