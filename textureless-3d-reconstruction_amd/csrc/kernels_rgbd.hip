// kernels_rgbd.hip -- joint point-to-plane + photometric registration of frame pairs (tl3d_build_intensity_many, tl3d_rgbd_evaluate_pairs,
// tl3d_rgbd_register_pairs): the intensity maps of the slots and one pass of both systems of normal equations
// at the poses in device memory.  tests/rgbd_reference.py restates every sequence below in numpy; it is the normative one.
//
// INTENSITY MAP of a slot: one float4 (S, Sx, Sy, flag) per pixel, kept in PHASE-MAJOR ROWS like the normal map (tl3d_internal.h:
// pm_index): a level samples every stride-th pixel, and there samples 4 px apart are neighbours in memory.
//   y      = 29 B + 150 G + 77 R                     an integer (the weights sum to 256)
//   valid  the slot's f32 depth is finite and > 0;  two valid pixels are LINKED when fabsf(a - b) <= jump * fminf(a, b) (f32: the depth
//          filter's rule, scale-free)
//   S      = (float)sum y / (float)(n * 65280)       over the n pixels of the (2 r + 1)^2 window that are in the image, valid and linked
//                                                    to the centre (the centre is one of them): two integers below 2^24 (r <= 7), one
//                                                    correctly rounded division -- the order of the window does not matter
//   flag   0 invalid centre (the whole record is zero); 2 all four axis neighbours are in the image, valid and linked to the centre;
//          else 1
//   Sx, Sy = 0.5f * (S(u + 1, v) - S(u - 1, v)), 0.5f * (S(u, v + 1) - S(u, v - 1)) where flag is 2, else 0
// Smoothing and gradients stay on one side of a depth edge: an occlusion boundary, whose intensity edge moves with the viewpoint,
// gives no target record (flag 2) and is averaged with its own side only.
//
// THE PASS.  Per sampled pixel the geometric half is the arithmetic of icp_accumulate_core (icp_sample.h), restated: the same
// source vertex (the window-averaged depth when normal smoothing is on), fmaf chains, pixel-ray quotients, rcp + Newton reciprocal,
// nearest-pixel (ut, vt), gate, residual and J = [q x n, n].  The photometric half, f32 with plain operators and FMAs only where
// written (-ffp-contract=off):
//   M_t = imap_tgt[vt][ut], M_s = imap_src[v][u]
//   a geometric correspondence QUALIFIES when M_t.flag == 2 and M_s.flag >= 1; it is a photometric one when also |r_I| <= photo_gate
//   r_I = fmaf(M_t.Sx, uf - (float)ut, fmaf(M_t.Sy, vf - (float)vt, M_t.S)) - M_s.S      the target image to first order about (ut, vt)
//   gx = (M_t.Sx * fx) * inv,  gy = (M_t.Sy * fy) * inv,  gz = -fmaf(gx, qx, gy * qy) * inv      d r_I / d q, inv = 1 / qz
//   J_I = [q x g, g]                                  the form and the fmaf pattern of the geometric J
// SIGN.  r_I(q) = I_t(pi(q)) - I_s with pi(q) = (fx qx / qz + cx, fy qy / qz + cy): d r_I / d q = (Sx fx / qz, Sy fy / qz,
// -(Sx fx qx + Sy fy qy) / qz^2) = g.  The update T <- exp(x) T moves q by w x q + v: d r_I = g . (w x q + v) = w . (q x g) + v . g,
// the geometric J with g for n, so both systems are solved by one x = -(A + lam I)^+ b (tests/test_rgbd_reference_cpu.py checks J_I
// against central differences).
// Sums: fp64 sums of exact fp64 products of f32 values, the two systems apart (tl3d_internal.h: RGBD_SUMS).
//
// Work layout, as kernels_icp_eval.hip and kernels_track.hip: grid = (members, pairs); workgroup (m, p) takes samples m * 256 + tid,
// + members * 256, ... of pair p and writes its 64 partial sums to slab[p][m]; rgbd_step_kernel (kernels_regstep.hip)
// adds them in member order, one wave per pair.  `members` is a function of the level geometry only and nothing is exchanged
// between workgroups inside a launch: a pair's sums and pose are bit for bit the same in every run, whatever batch it is in and
// wherever in it.  Two launches per iteration on the context's stream; the host enqueues every launch of every level and reads the
// states once; a pair that is done or over returns at once.
// Bytes per sampled pixel: 4 (source depth) + 16 (source record) + 16 (target normal record) + 16 (target record) = 52 B.
#include "tl3d_internal.h"
#include "icp_sample.h"

namespace tl3d {

// ---- intensity maps ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool im_valid(float d) { return d > 0.0f && d < __builtin_inff(); }                 // NaN fails both
__device__ __forceinline__ bool im_linked(float a, float b, float jump) { return fabsf(a - b) <= jump * fminf(a, b); }

// first half: S of every pixel, the rest of the record zero (the flag too: the second half sets it)
__global__ __launch_bounds__(256) void intensity_smooth_kernel(int W, int H, const float *__restrict__ depth, const uint8_t *__restrict__ bgr,
                                                               int radius, float jump, float4 *__restrict__ imap) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u >= W || v >= H) return;
    const float d0 = depth[(size_t)v * W + u];
    float S = 0.0f;
    if (im_valid(d0)) {
        unsigned sum = 0, n = 0;
        const int v0 = max(v - radius, 0), v1 = min(v + radius, H - 1), u0 = max(u - radius, 0), u1 = min(u + radius, W - 1);
        for (int vv = v0; vv <= v1; ++vv)
            for (int uu = u0; uu <= u1; ++uu) {
                const float d = depth[(size_t)vv * W + uu];
                if (!im_valid(d) || !im_linked(d, d0, jump)) continue;
                const uint8_t *c = bgr + ((size_t)vv * W + uu) * 3;
                sum += 29u * c[0] + 150u * c[1] + 77u * c[2];
                n += 1u;
            }
        S = (float)sum / (float)(n * 65280u);
    }
    imap[pm_index(u, v, pm_w4(W))] = make_float4(S, 0.0f, 0.0f, 0.0f);
}

// second half: flag and central differences.  It reads the neighbours' S and writes this pixel's other three words only.
__global__ __launch_bounds__(256) void intensity_gradient_kernel(int W, int H, const float *__restrict__ depth, float jump, float4 *imap) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63);
    const int v = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u >= W || v >= H) return;
    const size_t i = (size_t)v * W + u;
    const float d0 = depth[i];
    float sx = 0.0f, sy = 0.0f, flag = 0.0f;
    if (im_valid(d0)) {
        flag = 1.0f;
        if (u >= 1 && v >= 1 && u <= W - 2 && v <= H - 2) {
            const float dl = depth[i - 1], dr = depth[i + 1], du = depth[i - W], dd = depth[i + W];
            if (im_valid(dl) && im_valid(dr) && im_valid(du) && im_valid(dd) && im_linked(dl, d0, jump) && im_linked(dr, d0, jump) &&
                im_linked(du, d0, jump) && im_linked(dd, d0, jump)) {
                const float *S = (const float *)imap;
                const int w4 = pm_w4(W);
                flag = 2.0f;
                sx = 0.5f * (S[4 * pm_index(u + 1, v, w4)] - S[4 * pm_index(u - 1, v, w4)]);
                sy = 0.5f * (S[4 * pm_index(u, v + 1, w4)] - S[4 * pm_index(u, v - 1, w4)]);
            }
        }
    }
    float *o = (float *)(imap + pm_index(u, v, pm_w4(W)));
    o[1] = sx;
    o[2] = sy;
    o[3] = flag;
}

int launch_intensity(hipStream_t s, const Cam &cam, const float *depth, const uint8_t *bgr, int radius, float jump, float4 *imap) {
    const dim3 grid((cam.W + 63) / 64, (cam.H + 3) / 4);
    hipLaunchKernelGGL(intensity_smooth_kernel, grid, dim3(256), 0, s, cam.W, cam.H, depth, bgr, radius, jump, imap);
    TL3D_HIP(hipGetLastError());
    hipLaunchKernelGGL(intensity_gradient_kernel, grid, dim3(256), 0, s, cam.W, cam.H, depth, jump, imap);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// ---- the pass --------------------------------------------------------------------------------------------------------------------
// 56 fp64 sums and 4 counts per lane, four samples per trip: 214 VGPRs, no scratch, two waves per SIMD
__global__ __launch_bounds__(256) void rgbd_pass_kernel(Cam cam, const RgbdPair *__restrict__ pairs, RgbdLevel L, const RgbdState *__restrict__ states,
                                                        StepKind kind, double *__restrict__ slab) {
    const int pair = blockIdx.y, member = blockIdx.x, members = gridDim.x;
    const RgbdState *st = states + pair;
    if (st->icp.over || (kind == STEP_ITERATE && st->icp.done)) return;    // set by EARLIER launches only: uniform over the pair's workgroups
    __shared__ double sm[4][RGBD_SUMS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const RgbdPair pr = pairs[pair];
    // the pose is the same in every lane: scalar registers
    auto uni = [](float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); };
    float r[9], t[3];
    r[0] = uni((float)st->icp.T[0]); r[1] = uni((float)st->icp.T[1]); r[2] = uni((float)st->icp.T[2]);  t[0] = uni((float)st->icp.T[3]);
    r[3] = uni((float)st->icp.T[4]); r[4] = uni((float)st->icp.T[5]); r[5] = uni((float)st->icp.T[6]);  t[1] = uni((float)st->icp.T[7]);
    r[6] = uni((float)st->icp.T[8]); r[7] = uni((float)st->icp.T[9]); r[8] = uni((float)st->icp.T[10]); t[2] = uni((float)st->icp.T[11]);
    const float sc = uni(pr.scale);
    const float wlim = (float)cam.W - 0.5f, hlim = (float)cam.H - 0.5f;
    const int w4 = pm_w4(cam.W);
    auto xray = [&](int u) { return ((float)u - cam.cx) / cam.fx; };
    auto yray = [&](int v) { return ((float)v - cam.cy) / cam.fy; };
    double ag[28], ap[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) { ag[i] = 0.0; ap[i] = 0.0; }
    int n_src = 0, n_corr = 0, n_elig = 0, n_photo = 0;
    const int ns = L.Ws * L.Hs, step = members * 256;
    struct Samp { float px, py, pz, inv, uf, vf; int ut, vt; bool src_ok, ok; };
    // up to the association: the source vertex, its transform, the projection and the nearest target pixel (0, 0 when there is none)
    auto prep = [&](float draw, int u, int v) {
        Samp q;
        const float d = draw * sc;
        q.src_ok = (d > L.mind && d < L.maxd);
        const float p0 = xray(u) * d;
        const float p1 = yray(v) * d;
        q.px = fmaf(r[0], p0, fmaf(r[1], p1, fmaf(r[2], d, t[0])));
        q.py = fmaf(r[3], p0, fmaf(r[4], p1, fmaf(r[5], d, t[1])));
        q.pz = fmaf(r[6], p0, fmaf(r[7], p1, fmaf(r[8], d, t[2])));
        bool ok = q.src_ok && (q.pz > 0.0f);
        // 1 / pz as icp_accumulate_core has it: v_rcp_f32 + one Newton step is the IEEE quotient in [2^-126, 2^126), else the division
        float inv = __builtin_amdgcn_rcpf(q.pz);
        inv = fmaf(fmaf(-q.pz, inv, 1.0f), inv, inv);
        if (__builtin_expect(ok && !(q.pz >= 1.17549435e-38f && q.pz < 8.5e37f), 0)) inv = 1.0f / q.pz;
        q.inv = inv;
        q.uf = fmaf(cam.fx * q.px, inv, cam.cx);
        q.vf = fmaf(cam.fy * q.py, inv, cam.cy);
        ok = ok && (q.uf >= -0.5f && q.uf < wlim && q.vf >= -0.5f && q.vf < hlim);
        int ut = (int)floorf(q.uf + 0.5f), vt = (int)floorf(q.vf + 0.5f);
        ut = min(ut, cam.W - 1);
        vt = min(vt, cam.H - 1);
        q.ut = ok ? ut : 0;
        q.vt = ok ? vt : 0;
        q.ok = ok;
        return q;
    };
    auto accum = [&](const Samp &q, const float4 ms, const float4 nd, const float4 mt) {
        if (q.src_ok) n_src += 1;
        const float dt = nd.w;
        if (!(q.ok && dt > 0.0f)) return;
        const float px = q.px, py = q.py, pz = q.pz;
        const float qx = xray(q.ut) * dt;
        const float qy = yray(q.vt) * dt;
        const float dx = px - qx, dy = py - qy, dz = pz - dt;
        const float dist2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
        if (!(dist2 <= L.md2)) return;
        const float res = fmaf(dx, nd.x, fmaf(dy, nd.y, dz * nd.z));
        {
            const double J[6] = {(double)fmaf(py, nd.z, -(pz * nd.y)), (double)fmaf(pz, nd.x, -(px * nd.z)),
                                 (double)fmaf(px, nd.y, -(py * nd.x)), (double)nd.x, (double)nd.y, (double)nd.z};
            const double rr = (double)res;
            // every factor is an f32 value: every product is exact in fp64 and fma(a, b, s) rounds the very sum s + a * b
            int m = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
#pragma unroll
                for (int b = a; b < 6; ++b) { ag[m] = fma(J[a], J[b], ag[m]); ++m; }
                ag[21 + a] = fma(J[a], rr, ag[21 + a]);
            }
            ag[27] = fma(rr, rr, ag[27]);
            n_corr += 1;
        }
        if (!(mt.w == 2.0f && ms.w >= 1.0f)) return;
        n_elig += 1;
        const float ri = fmaf(mt.y, q.uf - (float)q.ut, fmaf(mt.z, q.vf - (float)q.vt, mt.x)) - ms.x;
        if (!(fabsf(ri) <= L.photo_gate)) return;
        const float gx = (mt.y * cam.fx) * q.inv;
        const float gy = (mt.z * cam.fy) * q.inv;
        const float gz = -fmaf(gx, px, gy * py) * q.inv;
        {
            const double J[6] = {(double)fmaf(py, gz, -(pz * gy)), (double)fmaf(pz, gx, -(px * gz)),
                                 (double)fmaf(px, gy, -(py * gx)), (double)gx, (double)gy, (double)gz};
            const double rr = (double)ri;
            int m = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
#pragma unroll
                for (int b = a; b < 6; ++b) { ap[m] = fma(J[a], J[b], ap[m]); ++m; }
                ap[21 + a] = fma(J[a], rr, ap[21 + a]);
            }
            ap[27] = fma(rr, rr, ap[27]);
            n_photo += 1;
        }
    };
    // NS samples per trip: their source reads, then their projections and pairs of gathers, then the sums -- each of the two
    // memory round trips of a sample is shared by the NS of them (7.2 / 4.9 / 4.4 us per 1080p pair-iteration with 1 / 2 / 4).  A slot past the thread's last sample reads element 0 and counts as
    // depth 0 (rejected as any invalid depth); the per-thread order of the sums is the sample order.
    constexpr int NS = 4;
#pragma unroll 1
    for (int s0 = member * 256 + tid; s0 < ns; s0 += NS * step) {
        float draw[NS];
        float4 ms[NS], nd[NS], mt[NS];
        int uu[NS], vv[NS];
        Samp q[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int s = s0 + k * step;
            const bool in = s < ns;
            const int vs = in ? s / L.Ws : 0, us = in ? s - vs * L.Ws : 0;
            uu[k] = us * L.stride;                           // <= W - 1, H - 1: Ws, Hs are the ceilings
            vv[k] = vs * L.stride;
            const float dv = pr.depth_src[pr.src_pm ? pm_index(uu[k], vv[k], w4) : (size_t)vv[k] * cam.W + uu[k]];
            ms[k] = pr.imap_src[pm_index(uu[k], vv[k], w4)];
            draw[k] = in ? dv : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            q[k] = prep(draw[k], uu[k], vv[k]);
            const size_t it = pm_index(q[k].ut, q[k].vt, w4);
            nd[k] = pr.nmap_tgt[it];
            mt[k] = pr.imap_tgt[it];                         // the one extra gather, at the pixel (and index) of the normal record
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) accum(q[k], ms[k], nd[k], mt[k]);
    }
    // every lane is back here: the shuffles of the reduction run with EXEC full.  Two trees of 32 sums (icp_sample.h)
    double w[32];
#pragma unroll
    for (int i = 0; i < 28; ++i) w[i] = ag[i];
    w[28] = (double)n_corr;
    w[29] = (double)n_src;
    w[30] = (double)n_elig;
    w[31] = 0.0;
    wave_reduce32(w, lane);
    if (!(lane & 1)) sm[wid][lane >> 1] = w[0];
#pragma unroll
    for (int i = 0; i < 28; ++i) w[i] = ap[i];
    w[28] = (double)n_photo;
    w[29] = 0.0;
    w[30] = 0.0;
    w[31] = 0.0;
    wave_reduce32(w, lane);
    if (!(lane & 1)) sm[wid][32 + (lane >> 1)] = w[0];
    __syncthreads();
    if (tid < RGBD_SUMS) slab[((size_t)pair * members + member) * RGBD_SUMS + tid] = ((sm[0][tid] + sm[1][tid]) + sm[2][tid]) + sm[3][tid];
}

int rgbd_members(int Ws, int Hs) {
    long long m = ((long long)Ws * Hs + RGBD_SAMPLES_PER_MEMBER - 1) / RGBD_SAMPLES_PER_MEMBER;
    if (m < 1) m = 1;
    if (m > RGBD_MEMBERS_CAP) m = RGBD_MEMBERS_CAP;
    return (int)m;
}

// one pass of every pair at the pose in its state; slab: [n_pairs][L.members][RGBD_SUMS] doubles; n_pairs <= 65535 (grid.y)
int launch_rgbd_pass(hipStream_t s, const Cam &cam, const RgbdPair *pairs, int n_pairs, const RgbdLevel &L, const RgbdState *states,
                     StepKind kind, double *slab) {
    if (n_pairs <= 0) return TL3D_OK;
    hipLaunchKernelGGL(rgbd_pass_kernel, dim3(L.members, n_pairs), dim3(256), 0, s, cam, pairs, L, states, kind, slab);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

}  // namespace tl3d
