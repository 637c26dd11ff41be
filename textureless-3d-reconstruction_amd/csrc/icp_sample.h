// icp_sample.h -- the per-sample arithmetic of one point-to-plane pass (oracle/tl3d_oracle.c: icp_pass) and a workgroup's
// reduction of its sums: shared by the registration kernels (kernels_icp.hip: they iterate) and the evaluation kernel
// (kernels_icp_eval.hip: one pass at a given pose), so that both take the same source vertex, the same fmaf chains, the same
// nearest-pixel association, gate, residual and J, and add the same fp64 products.
#pragma once
#include "tl3d_internal.h"

namespace tl3d {

// accumulate this workgroup's share of the sums and leave the workgroup total in sm_out[0..31] (valid for threads < 32
// after the function's last barrier)
// `member` of `members` workgroups share one registration: member m takes samples m*256 + tid, + members*256, ...
// ray_tab (batched kernel; null: computed in place): the pixel-ray factors ((float)u - cx) / fx for u < W, then ((float)v - cy) / fy
// for v < H, in LDS -- the very quotients the expression gives (filled with that expression), looked up instead of divided
// out four times per sample and pass (an IEEE f32 division is ~10 vector instructions; they were 40 of the ~115 per sample).
template <bool SCALE, bool TAB>
__device__ __forceinline__ void icp_accumulate_core(const Cam &cam, const float *__restrict__ depth_s, const float4 *__restrict__ nmap_t,
                                                    float sc, float mind, float maxd, float md2, int stride, int Ws, int Hs,
                                                    const float r[9], const float t[3], int member, int members, int src_pm,
                                                    double (*sm)[ICP_SLAB], double *__restrict__ sm_out, unsigned long long *stamp = nullptr,
                                                    const float *ray_tab = nullptr) {
    const float wlim = (float)cam.W - 0.5f, hlim = (float)cam.H - 0.5f;
    // Both maps are device memory: say so.  The batched kernel reads the pointers from a table in memory, where the compiler only
    // knows a generic pointer and issues FLAT loads -- which also count on the LDS counter, so that every wait for an LDS read (the
    // ray tables below) would wait for every gather in flight and undo the software pipeline.
    typedef const __attribute__((address_space(1))) float *gfloat_p;
    typedef float v4f __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) v4f *gfloat4_p;
    const gfloat_p depth_g = (gfloat_p)depth_s;
    const gfloat4_p nmap_g = (gfloat4_p)nmap_t;
    // the target map is kept in phase-major rows, the source depth too when it is a window-averaged one (src_pm); a raw frame is
    // row-major: (mask, shift, phase length, row length) make one index expression of both (wave-uniform values)
    const int w4 = pm_w4(cam.W);
    const int s_mask = src_pm ? 3 : 0, s_shift = src_pm ? 2 : 0, s_row = src_pm ? 4 * w4 : cam.W;
    const float *xtab = ray_tab, *ytab = ray_tab + cam.W;
    auto xray = [&](int u) { return TAB ? xtab[u] : ((float)u - cam.cx) / cam.fx; };
    auto yray = [&](int v) { return TAB ? ytab[v] : ((float)v - cam.cy) / cam.fy; };
    double acc[30];
#pragma unroll
    for (int i = 0; i < 30; ++i) acc[i] = 0.0;
    double accs[8];                                      // scale column (Sim(3) runs): sum J_a J_alpha (6), J_alpha^2, J_alpha r
#pragma unroll
    for (int i = 0; i < 8; ++i) accs[i] = 0.0;
    // Samples are walked with 32-bit pixel coordinates kept per thread (a sample index divided by the level's width cost a 64-bit
    // division per sample): sample s = vs * Ws + us; the next one of this thread is `step` = members * 256 samples on.
    const int step = members * 256;
    const int dvs = step / Ws, dus = step - dvs * Ws;        // wave-uniform
    struct Samp { float px, py, pz; int ut, vt; bool src_ok, ok; };
    auto prep = [&](float draw, int u, int v) {
        Samp q;
        const float d = draw * sc;
        q.src_ok = (d > mind && d < maxd);
        const float p0 = xray(u) * d;
        const float p1 = yray(v) * d;
        q.px = fmaf(r[0], p0, fmaf(r[1], p1, fmaf(r[2], d, t[0])));
        q.py = fmaf(r[3], p0, fmaf(r[4], p1, fmaf(r[5], d, t[1])));
        q.pz = fmaf(r[6], p0, fmaf(r[7], p1, fmaf(r[8], d, t[2])));
        bool ok = q.src_ok && (q.pz > 0.0f);
        // 1 / pz: v_rcp_f32 + one Newton step IS the IEEE quotient for every positive float in [2^-126, 2^126) (exhaustive check:
        // tools/ubench_rcp.hip, profiles/r03_ubench_rcp.txt); lanes outside take the division; pz <= 0 is rejected whatever it gives
        float inv = __builtin_amdgcn_rcpf(q.pz);
        inv = fmaf(fmaf(-q.pz, inv, 1.0f), inv, inv);
        if (__builtin_expect(ok && !(q.pz >= 1.17549435e-38f && q.pz < 8.5e37f), 0)) inv = 1.0f / q.pz;
        const float uf = fmaf(cam.fx * q.px, inv, cam.cx);
        const float vf = fmaf(cam.fy * q.py, inv, cam.cy);
        ok = ok && (uf >= -0.5f && uf < wlim && vf >= -0.5f && vf < hlim);
        int ut = (int)floorf(uf + 0.5f), vt = (int)floorf(vf + 0.5f);
        ut = min(ut, cam.W - 1);
        vt = min(vt, cam.H - 1);
        q.ut = ok ? ut : 0;
        q.vt = ok ? vt : 0;
        q.ok = ok;
        return q;
    };
    auto accum = [&](const Samp &q, const v4f nd) {
        if (q.src_ok) acc[29] += 1.0;
        const float dt = nd.w;
        if (!(q.ok && dt > 0.0f)) return;
        const float px = q.px, py = q.py, pz = q.pz;
        const float qx = xray(q.ut) * dt;
        const float qy = yray(q.vt) * dt;
        const float dx = px - qx, dy = py - qy, dz = pz - dt;
        const float dist2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
        if (!(dist2 <= md2)) return;
        const float res = fmaf(dx, nd.x, fmaf(dy, nd.y, dz * nd.z));
        const double J[6] = {(double)fmaf(py, nd.z, -(pz * nd.y)), (double)fmaf(pz, nd.x, -(px * nd.z)),
                             (double)fmaf(px, nd.y, -(py * nd.x)), (double)nd.x, (double)nd.y, (double)nd.z};
        const double rr = (double)res;
        // every factor is an f32 value, so every product is EXACT in fp64 (48 significant bits) and fma(a, b, s) rounds the very
        // sum s + a * b the oracle's multiply-then-add rounds: one instruction instead of two, the same bits
        int m = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = a; b < 6; ++b) { acc[m] = fma(J[a], J[b], acc[m]); ++m; }
            acc[21 + a] = fma(J[a], rr, acc[21 + a]);
        }
        acc[27] = fma(rr, rr, acc[27]);
        acc[28] += 1.0;
        if (SCALE) {
            // sigma <- sigma exp(alpha) moves q = R sigma p_hat + t by alpha (q - t):  J_alpha = n . (q - t)
            const double ja = (double)fmaf(nd.x, px - t[0], fmaf(nd.y, py - t[1], nd.z * (pz - t[2])));
#pragma unroll
            for (int a = 0; a < 6; ++a) accs[a] = fma(J[a], ja, accs[a]);
            accs[6] = fma(ja, ja, accs[6]);
            accs[7] = fma(ja, rr, accs[7]);
        }
    };
    // Four samples per trip, software-pipelined over the trips: while trip i is added up, the normal-map gathers of trip i + 1 and
    // the source depths of trip i + 2 are in flight (the trace of round 4 showed a trip of the plain loop -- depths, wait, gathers,
    // wait, sums -- at 2.7-4 us, two exposed memory latencies, against ~0.8 us of arithmetic: with two workgroups per CU there is
    // one other wave per SIMD to fill them).  Loads past a thread's last sample go to element 0 and count as depth 0 (rejected
    // as any invalid depth); the per-thread order of the sums is the sample order, as ever.
    constexpr int NS = 4;
    struct Src { float d[NS]; int uu[NS], vv[NS]; };
    int us, vs;                                              // the next sample this thread fetches
    {
        const int s0 = member * 256 + (int)threadIdx.x;
        vs = s0 / Ws;
        us = s0 - vs * Ws;
    }
    auto fetch_src = [&]() {
        Src x;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const bool in = vs < Hs;
            x.uu[k] = in ? us * stride : 0;
            x.vv[k] = in ? vs * stride : 0;
            const float dv = depth_g[(size_t)x.vv[k] * s_row + ((x.uu[k] & s_mask) * w4 + (x.uu[k] >> s_shift))];
            x.d[k] = in ? dv : 0.0f;
            us += dus;
            vs += dvs;
            if (us >= Ws) { us -= Ws; vs += 1; }
        }
        return x;
    };
    const int vs_first = vs;
    Src src = fetch_src();                                  // trip 0's depths
    Samp q[NS];
    v4f nd[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) q[k] = prep(src.d[k], src.uu[k], src.vv[k]);
#pragma unroll
    for (int k = 0; k < NS; ++k) nd[k] = nmap_g[pm_index(q[k].ut, q[k].vt, w4)];      // trip 0's gathers
    int vs_cur = vs_first, vs_next = vs;                    // row of the first sample of the trip in q / of the trip in src
    src = fetch_src();                                      // trip 1's depths
    // Two trips per turn of the loop, the two sets of registers (q, nd) and (qb, ndb) changing roles: a one-trip body ends with
    // "the next trip becomes the current one", 36 register moves per trip (7 % of its vector instructions) that unrolling by hand
    // makes disappear.  The loop is left after whichever half finds no trip of its own in hand.
    Samp qb[NS];
    v4f ndb[NS];
    for (;;) {
        if (!(vs_cur < Hs)) break;                          // the trip in (q, nd) holds no sample of this thread
#pragma unroll
        for (int k = 0; k < NS; ++k) qb[k] = prep(src.d[k], src.uu[k], src.vv[k]);
#pragma unroll
        for (int k = 0; k < NS; ++k) ndb[k] = nmap_g[pm_index(qb[k].ut, qb[k].vt, w4)];      // next trip's gathers
        vs_cur = vs_next;
        vs_next = vs;
        src = fetch_src();                                  // the depths of the trip after the next
#pragma unroll
        for (int k = 0; k < NS; ++k) accum(q[k], nd[k]);    // this trip's gathers were issued a trip ago
        if (!(vs_cur < Hs)) break;                          // ... and the same with the roles of the two register sets exchanged
#pragma unroll
        for (int k = 0; k < NS; ++k) q[k] = prep(src.d[k], src.uu[k], src.vv[k]);
#pragma unroll
        for (int k = 0; k < NS; ++k) nd[k] = nmap_g[pm_index(q[k].ut, q[k].vt, w4)];
        vs_cur = vs_next;
        vs_next = vs;
        src = fetch_src();
#pragma unroll
        for (int k = 0; k < NS; ++k) accum(qb[k], ndb[k]);
    }
    if (stamp) stamp[0] = wall_clock64();
    // Wave reduction of the 30 sums.  A shuffle tree per sum is 30 x 6 dependent 64-bit shuffles (6.6 us measured, a third of
    // an iteration); instead the lanes split the sums between them while they add: at distance 32 the lower half of the wave
    // keeps sums 0..15 and the upper half 16..31, at distance 16 each quarter keeps 8 of those, ... -- 16 + 8 + 4 + 2 + 1 + 1
    // shuffles.  Every sum is still added over the same tree (lane l with l + 32, then with l + 16, ...; IEEE addition commutes),
    // so the totals are bit for bit those of the shuffle tree; the total of sum c ends in lanes 2c and 2c + 1.
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double v[32];
#pragma unroll
    for (int i = 0; i < 30; ++i) v[i] = acc[i];
    v[30] = 0.0;
    v[31] = 0.0;
#pragma unroll
    for (int half = 16, dist = 32; half >= 1; half >>= 1, dist >>= 1) {
        const bool up = (lane & dist) != 0;
#pragma unroll
        for (int k = 0; k < half; ++k) {
            const double send = up ? v[k] : v[k + half];
            const double keep = up ? v[k + half] : v[k];
            v[k] = keep + __shfl_xor(send, dist);
        }
    }
    v[0] += __shfl_xor(v[0], 1);
    if (!(lane & 1)) sm[wid][lane >> 1] = v[0];
    if (SCALE) {                                         // the 8 sums of the scale column: plain shuffle trees
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double w = accs[k];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) w += __shfl_xor(w, d);
            if (lane == 0) sm[wid][32 + k] = w;
        }
    } else if (lane < 8) {
        sm[wid][32 + lane] = 0.0;
    }
    if (stamp) stamp[1] = wall_clock64();
    __syncthreads();
    if (threadIdx.x < ICP_SLAB) {
        const int i = threadIdx.x;
        sm_out[i] = ((sm[0][i] + sm[1][i]) + sm[2][i]) + sm[3][i];            // (sums 30 and 31 are zero; 32..39 too unless the scale is estimated)
    }
}

// The wave reduction above as a function of its own, for kernels that keep 32 fp64 sums per lane (kernels_track.hip): same tree,
// same totals; the total of sum c ends in v[0] of lanes 2c and 2c + 1.  Every lane of the wave must call it.
// (icp_accumulate_core keeps its copy in place: calling this from there changed the instruction schedule of the registration
// kernels, and their code objects are pinned.)
template <int HALF, int DIST>
__device__ __forceinline__ void wave_reduce_step(double (&v)[32], const int lane) {
    const bool up = (lane & DIST) != 0;
#pragma unroll
    for (int k = 0; k < HALF; ++k) {
        const double send = up ? v[k] : v[k + HALF];
        const double keep = up ? v[k + HALF] : v[k];
        v[k] = keep + __shfl_xor(send, DIST);
    }
}
__device__ __forceinline__ void wave_reduce32(double (&v)[32], const int lane) {
    wave_reduce_step<16, 32>(v, lane);
    wave_reduce_step<8, 16>(v, lane);
    wave_reduce_step<4, 8>(v, lane);
    wave_reduce_step<2, 4>(v, lane);
    wave_reduce_step<1, 2>(v, lane);
    v[0] += __shfl_xor(v[0], 1);
}

}  // namespace tl3d
