// kernels_track.hip -- point-to-SDF registration of a depth frame against the TSDF channel (tl3d_track_evaluate, tl3d_track_frame;
// DESIGN.md section 12): one pass of the normal equations at the pose in device memory, with no intermediate view of the model.
//
// For every sampled pixel (u, v) = (us * stride, vs * stride), us < Ws = ceil(W / stride), vs < Hs = ceil(H / stride), in f32 with
// plain operators in the order written here (-ffp-contract=off; tests/track_reference.py restates it bit for bit, so the gate
// decisions and hence the counts are exact):
//   d   = depth[v][u] * scale                       the slot's f32 depth; valid when d > min_depth && d < max_depth (counts in n_src)
//   p_c = (xf * d, yf * d, d)                       xf = ((float)u - cx) / fx, yf = ((float)v - cy) / fy: the ray caster's quotients
//   x   = cg + (R^T p_c) * ivs                      grid coordinates; cg = (C - origin) * ivs - 0.5f, C = -R^T t from fp64, rounded
//                                                   as kernels_raycast.hip's RayArgs has them (track_pose_f32 below)
//   cell, F, g                                      tsdf_cell.h: load_cell / trilinear / trilinear_dx / dy / dz, usable weight >= max(1, min_weight)
//   correspondence                                  the cell is defined and |F| <= gate, gate = min((float)max_dist / trunc, 0.98f)
//   r   = F * trunc                                 metres
//   n_c = R (g * (trunc * ivs))                     the field's gradient in metres per metre, in the camera frame
//   J   = [p_c x n_c, n_c]
// SIGN.  r(p_c) = trunc * F(M^-1 p_c) with M = (R, t) world -> camera.  J is the Jacobian of r for p_c -> exp(x) p_c = p_c + w x p_c +
// v: dr = n_c . (w x p_c + v) = w . (p_c x n_c) + v . n_c.  Moving the point by exp(x) in the camera frame is moving the camera
// by exp(-x): M <- se3_apply(y) M with y = -x, so dr / dy = -J.  The Gauss-Newton step solves (A + lam I) x = -b (what solve6_*
// return) and the pose update applies y = -x (track_step_kernel, kernels_regstep.hip).  tests/test_track_reference_cpu.py checks
// d(e / 2) / dy = -b against central differences.
// Sums: A = sum J J^T (21), b = sum J r (6), e = sum r^2, n_corr, n_src -- the head of IcpState::sums; per-sample values f32, the
// sums fp64 sums of exact fp64 products (as icp_accumulate_core).
//
// Work layout.  A wave takes 8 x 8-sample tiles (neighbouring samples gather neighbouring cells, as the ray caster's pixels do);
// wave w of the members * 4 waves of the launch takes tiles w, w + members * 4, ... of the row-major tile grid; lanes past the right
// and bottom edges of a partial tile idle.  `members` depends on the sample count only; every workgroup writes its 32 partials
// to slab[member][0..31] and the step kernel adds them in member order: a pass's sums are bit for bit the same in every run.
//
// Iteration: TWO kernels per iteration on the context's stream -- this pass, then track_step_kernel (one wave: sum in member
// order, damped 6 x 6 solve, pose update in device memory).  The kernel boundary is the hand-off: nothing is exchanged between
// workgroups inside a launch, so nothing depends on dispatch order, residency or cache state (the arrival-ticket form of
// icp_iter_kernel saves one launch boundary per iteration and needs write-through partials, a drained ticket and an acquiring last
// arriver to be right; tracking is serial per frame and ends in a host read, and the fixed member-order sum comes for free here).
// No host round trip between iterations: the host enqueues every launch of every level and reads the state once.  A run that has
// converged or failed (state->done), or whose levels are over (state->over), makes its remaining launches return at once.
#include "tl3d_internal.h"
#include "tsdf_cell.h"
#include "icp_sample.h"

namespace tl3d {

constexpr int TRACK_TILES_PER_WAVE = 8;      // 512 samples per wave and pass before another member is added
constexpr int TRACK_MEMBERS_CAP = 256;

// the pose a pass uses, from the fp64 pose T (row-major 4 x 4, world -> camera): R rounded, C = -R^T t in fp64 then rounded --
// the expressions of launch_raycast, so that a pose handed over by the host and a pose updated on the device round alike
__host__ __device__ __forceinline__ void track_pose_f32(const double *T, float r[9], float c[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r[3 * i + j] = (float)T[4 * i + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = (float)(-((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]));
}

__global__ __launch_bounds__(256) void track_pass_kernel(Cam cam, Grid g, TrackArgs a, const int2 *__restrict__ pool,
                                                         const IcpState *__restrict__ state, StepKind kind, double *__restrict__ slab) {
    if (state->over || (kind == STEP_ITERATE && state->done)) return;      // set by EARLIER launches only: uniform over the grid
    __shared__ double sm[4][32];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float r[9], c[3], cg[3];
    track_pose_f32(state->T, r, c);
    const float org[3] = {g.ox, g.oy, g.oz};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) cg[ax] = (c[ax] - org[ax]) * a.ivs - 0.5f;
    double acc[30];
#pragma unroll
    for (int i = 0; i < 30; ++i) acc[i] = 0.0;
    BrickCache bc{0xffffffffu, SLOT_EMPTY, 0u};
    const int ntiles = a.tx * a.ty, nwaves = (int)gridDim.x * 4;
#pragma unroll 1
    for (int tile = (int)blockIdx.x * 4 + wid; tile < ntiles; tile += nwaves) {
        const int tyi = tile / a.tx, txi = tile - tyi * a.tx;
        const int us = txi * 8 + (lane & 7), vs = tyi * 8 + (lane >> 3);
        if (us >= a.Ws || vs >= a.Hs) continue;                   // a partial tile; us * stride <= W - 1 and vs * stride <= H - 1 otherwise
        const int u = us * a.stride, v = vs * a.stride;
        const float d = a.depth[(size_t)v * cam.W + u] * a.scale;
        if (!(d > a.mind && d < a.maxd)) continue;
        acc[29] += 1.0;
        const float xf = ((float)u - cam.cx) / cam.fx, yf = ((float)v - cam.cy) / cam.fy;
        const float p[3] = {xf * d, yf * d, d};
        float x[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const float w = (r[ax] * p[0] + r[3 + ax] * p[1]) + r[6 + ax] * p[2];      // (R^T p_c)_ax
            x[ax] = cg[ax] + w * a.ivs;
        }
        float tc[8], f[3];
        if (!load_cell(g, pool, a.mw, x, tc, f, bc)) continue;
        const float F = trilinear(tc, f);
        if (!(fabsf(F) <= a.gate)) continue;
        const float gx = trilinear_dx(tc, f), gy = trilinear_dy(tc, f), gz = trilinear_dz(tc, f);
        const float res = F * g.trunc;
        const float gw[3] = {gx * a.nk, gy * a.nk, gz * a.nk};
        float n[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) n[ax] = (r[3 * ax] * gw[0] + r[3 * ax + 1] * gw[1]) + r[3 * ax + 2] * gw[2];
        const double J[6] = {(double)(p[1] * n[2] - p[2] * n[1]), (double)(p[2] * n[0] - p[0] * n[2]), (double)(p[0] * n[1] - p[1] * n[0]),
                             (double)n[0], (double)n[1], (double)n[2]};
        const double rr = (double)res;
        // every factor is an f32 value: every product is exact in fp64 and fma(a, b, s) rounds the very sum s + a * b
        int m = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) { acc[m] = fma(J[i], J[j], acc[m]); ++m; }
            acc[21 + i] = fma(J[i], rr, acc[21 + i]);
        }
        acc[27] = fma(rr, rr, acc[27]);
        acc[28] += 1.0;
    }
    // every lane is back here: the shuffles of the reduction run with EXEC full
    double v[32];
#pragma unroll
    for (int i = 0; i < 30; ++i) v[i] = acc[i];
    v[30] = 0.0;
    v[31] = 0.0;
    wave_reduce32(v, lane);
    if (!(lane & 1)) sm[wid][lane >> 1] = v[0];
    __syncthreads();
    if (threadIdx.x < 32) slab[(size_t)blockIdx.x * 32 + threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

int track_members(int Ws, int Hs) {
    const long long tiles = (long long)((Ws + 7) / 8) * ((Hs + 7) / 8);
    long long m = (tiles + 4 * TRACK_TILES_PER_WAVE - 1) / (4 * TRACK_TILES_PER_WAVE);
    if (m < 1) m = 1;
    if (m > TRACK_MEMBERS_CAP) m = TRACK_MEMBERS_CAP;
    return (int)m;
}

// one pass at the pose in state->T; slab: [track_members(Ws, Hs)][32] doubles
int launch_track_pass(hipStream_t s, const Cam &cam, const Grid &g, const float *depth, float scale, float mind, float maxd, int min_weight,
                      int stride, double max_dist, const int2 *tsdf, const IcpState *state, StepKind kind, double *slab) {
    TrackArgs a;
    a.depth = depth;
    a.scale = scale;
    a.mind = mind;
    a.maxd = maxd;
    a.ivs = (float)(1.0 / g.vsd);
    a.gate = fminf((float)max_dist / g.trunc, 0.98f);
    a.nk = g.trunc * a.ivs;
    a.mw = min_weight < 1 ? 1 : min_weight;
    a.stride = stride;
    a.Ws = (cam.W + stride - 1) / stride;
    a.Hs = (cam.H + stride - 1) / stride;
    a.tx = (a.Ws + 7) / 8;
    a.ty = (a.Hs + 7) / 8;
    const int members = track_members(a.Ws, a.Hs);
    hipLaunchKernelGGL(track_pass_kernel, dim3(members), dim3(256), 0, s, cam, g, a, tsdf, state, kind, slab);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

}  // namespace tl3d
