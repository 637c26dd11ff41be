// kernels_tsdf.hip -- row a11: TSDF integration of depth frames into the brick-major grid, the UPDATE kernel.
// No reference code exists for this row; the convention is the oracle's
// (oracle/tl3d_oracle.c: orc_tsdf_integrate) and both sides evaluate the same f32 sequence, so the integer
// grid {sum of rint(tsdf*32767), weight} is bit-identical.
//
// tl3d_integrate collects frames into BATCHES of up to 32 (TL3D_TSDF_MAXBATCH).  Kernels 1 to 4 -- the prep chain,
// kernels_tsdf_prep.hip -- leave, per batch, the list of bricks that at least one frame lists as MIXED (dearest first), per brick
// the mask of those frames, and per (frame, brick) the masks of its MIXED and FREE 4x4x4 sub-bricks.  Then:
//   5. tsdf_update_pairs_kernel  ONE launch per batch, one 64-lane wave per brick of the batch list: for every frame that lists
//        the brick (frame mask), the voxels of its MIXED sub-bricks are projected; the 8x8-pixel tile under a voxel's pixel
//        decides most of them (free / behind everything), the rest gather their depth value; FREE sub-bricks add (32767, 1);
//        the increments of all frames are summed per voxel and the brick's records are read and written ONCE per batch
//        (integer sums commute: the grid is the one-frame-at-a-time grid bit for bit).  A sub-brick's 64 records are
//        contiguous (tl3d_internal.h: in_brick_index): every record access of a wave is one 512-B run.
// Every classification of the prep chain is conservative with respect to the per-voxel rule, so the result is the oracle's bit
// for bit whatever the view.
// Algorithmic bytes per launch = 8 B x (records read + written), counted by the kernel in counting mode
// ("counted, never estimated"; F = frames of the batch is reported), + 8 B per counted free-space
// brick + the depth images of the batch's frames.
#include <stdlib.h>

#include <type_traits>

#include "tl3d_internal.h"
#include "bp_device.h"
#include "tsdf_batch.h"

namespace tl3d {

// ---- 5. the update: one launch per batch ---------------------------------------------------------------------------------
// A wave takes one brick of the batch list per trip.  What bounds the kernel is the RATE OF SCATTERED DEPTH READS the memory
// system sustains (56 G 64-B requests per second that miss the L2, whatever the occupancy: tools/ubench_gather.hip), so a voxel
// asks for its depth pixel only when the answer is open.  The unit of work is ONE PAIR (frame, MIXED sub-brick of the brick):
// 64 lanes = the 64 voxels of that sub-brick, in three pipelined stages:
//   A  project (the oracle's sequence: pair_project, below) -> pixel, and load the 8-B record of the 8x8-PIXEL TILE that
//      holds the pixel (lowest depth if all 64 pixels are valid, highest valid depth; 260 KB per frame: these loads hit the L2);
//   B  the tile decides most voxels (pair_tile_test): highest - zc < -trunc  => sdf < -trunc whatever the pixel says: no update;
//                                                     lowest - zc >= 1.001 trunc => tsdf == 1 exactly: (+32767, +1);
//      (rounding is monotone: d >= lowest => fl(d - zc) >= fl(lowest - zc), so both decisions are the per-voxel rule's own);
//      only the voxels in between -- a third of the lanes of a MIXED sub-brick -- gather their depth pixel, the others read
//      the frame's valid pixel (one shared line);
//   C  depth value -> quantised tsdf, added to the voxel's running sum.
// After the brick's last pair the records that changed are read, added to and written: once per batch, whatever the number of
// frames.  The shape of the loop:
//   * the brick's pairs are walked in frame-major order (frame f's scalars -- pose, scale, image and tile-record base -- are
//     loaded when its first pair comes up), sub-brick s of the pair is a scalar: the lane's world coordinates are chosen by
//     three selects, everything else is straight-line code (wave-uniform branches cost about five instruction slots each);
//   * the running sums live in LDS: acc[s][lane], wave-private, one ds_add per pair (a register array indexed by a scalar would
//     need eight predicated adds);  FREE sub-bricks are counted per sub-brick over the frames with ballots and enter the sums
//     once per brick;
//   * the stages are software-pipelined over the pairs: step k runs A(k), C(k-1-LAT), B(k-1); a tile record has a full step
//     before anything waits for it, a depth value LAT - 1 steps and a third (and seven other waves of the SIMD have work
//     meanwhile).  ALWAYS one tile load and one depth load per step, so that the number of loads in flight is known wherever a
//     value is awaited (a count that depended on the masks would turn every wait into "all loads", the newest included).
//     LAT = 2 in the kernels without counters: the wait in front of stage C is vmcnt(3), it leaves the two newer steps' loads in
//     flight (at LAT = 1 it was vmcnt(1), and the kernel 3 % slower: DESIGN.md 7.5).  Loads return in order, so stage B's wait
//     for its tile record also waits for every depth value older than two steps: LAT = 3 needs no wait of its own in stage C,
//     buys a fraction of a step, and does not fit the scalar registers.
//   * P pairs take EXACTLY P + 1 + LAT steps.  The steady loop runs whole bodies of full steps and nothing else (6 steps at
//     LAT = 2: the parity of A -> B and the three-entry rings of B -> C both come round), P div 6 of them, with no branch but its
//     back edge and the frame switch.  Behind it, in straight-line code: the P mod 6 full steps that remain, each behind one
//     forward branch, and the drain for the ring phase the last of them leaves (one drain per remainder) -- B of the last pair
//     with C of pair P - 1 - LAT, then C of the LAT pairs still on their way: no projection, no tile record, one depth load.
//     Which stages a step runs is a compile-time argument of the ONE spelling of the stages.  The first 1 + LAT steps of a brick
//     still run their stages B and C on empty slots (zc = +inf, "behind everything": no update, legal addresses).
//     What does NOT work, and why the ends look as they do: the remaining steps and the drains as NESTED if / else (no path
//     rejoining) are linearised by the compiler's control-flow structuriser all the same -- every drain behind every join, the
//     pipeline's state kept alive twice over: 64 vector registers and 15 spilled; the remaining steps IN FRONT of the loop
//     (entering the body's sequence where P mod 6 steps are left of it, one drain) make the first step of every body wait for
//     all loads unless every load of those steps is awaited first, and are no faster; stages skipped by wave-uniform branches
//     INSIDE the loop body: the wait counts at the joins turn conservative and the launch takes a quarter longer (61 k
//     against 76 k frames/s).  Until this shape a brick ran 6 ceil((P + 3) / 6) steps, every one a whole stage A and both
//     loads: 5.5 empty steps per brick, 1.110 steps per pair where it is 1.06 now;
//   * every load of a stage is a scalar base + a 32-bit per-lane offset.
// 61 vector registers at LAT = 2 (56 at LAT = 1, 60 with counters), no scratch: eight waves per SIMD.
// The arithmetic of a voxel is pair_project + stage C below, the oracle's sequence: the grid is the oracle's bit for bit.

// loads from a wave-uniform base + a 32-bit per-lane byte offset (scalar base, vector offset: one address register per load)
template <typename DT> struct PixLoad;
template <> struct PixLoad<float> {
    typedef float raw;
    static __device__ __forceinline__ raw load(const char *base, unsigned off) { return *reinterpret_cast<const float *>(base + off); }
    static __device__ __forceinline__ float value(raw v) { return v; }
};
template <> struct PixLoad<uint16_t> {
    typedef unsigned short raw;
    static __device__ __forceinline__ raw load(const char *base, unsigned off) { return *reinterpret_cast<const unsigned short *>(base + off); }
    static __device__ __forceinline__ float value(raw v) { return mm_to_m(v); }
};
__device__ __forceinline__ float keep_vector(float x) {                   // x, wave-uniform, lives in a VECTOR register from here on
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ unsigned keep_scalar(unsigned x) {             // x, wave-uniform, is computed HERE and lives in one scalar register
    asm volatile("" : "+s"(x));
    return x;
}

// ---- a voxel's projection and its tile test ---------------------------------------------------------------------------------------
// v_mad_u32_u24 spelled out: every operand is below 2^24 (u, v, W < 2^16), the instruction is exact and full rate, and the
// optimiser, left to itself, folds these into 64-bit multiply-adds of the address; as opaque 32-bit values they become the 32-bit
// offset of a load from a wave-uniform base.
__device__ __forceinline__ unsigned mad_u24(unsigned a, unsigned b_uniform, unsigned c) {
    unsigned r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b_uniform), "v"(c));
    return r;
}
__device__ __forceinline__ int clamp_i32(int x, int hi_uniform) {        // min(max(x, 0), hi): one instruction (hi >= 0)
    int r;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(x), "s"(hi_uniform));
    return r;
}
__device__ __forceinline__ int cvt_flr_i32(float x) {                   // (int)floorf(x), one instruction; saturates, NaN -> 0
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// The per-voxel rule is the oracle's (oracle/tl3d_oracle.c: orc_tsdf_integrate), the same f32 sequence operation for operation,
// split so that a wave can issue its loads before it needs any of them:
//   position   xc, yc, zc = the voxel centre through the pose, three nested fmaf per axis;           zc > 0 or no update
//   pixel      uf = fmaf(fx * xc, 1 / zc, cx), vf alike; u = floor(uf + 0.5), v alike;               -0.5 <= uf < W - 0.5 (vf, H) or no update
//   depth      d = depth[v][u] * scale;  mind < d < maxd or no update;  sdf = d - zc;                sdf >= -trunc or no update
//   increment  tsdf = min(1, sdf * inv_trunc);  q = rint(tsdf * 32767);  record += (q, 1)
// pair_project is "position" and "pixel" (no memory access); "depth" and "increment" are stage C of the update kernel,
// which only the voxels that pair_tile_test leaves open reach with a depth value of their own.
//
// Stage A of a pair and rule (4), ONE spelling for the update kernel and for class_refine_kernel: whether the 8x8-pixel tile
// under a voxel's pixel decides it must come out the same in both, bit for bit -- a sub-brick that the refinement takes off a
// frame's MIXED mask is sound for exactly that reason and for no other.
// pair_project: the voxel centre (wxs, wys, wzs) through the pose (r0..r8, t0..t2) -> byte offsets of its pixel (pix) and of the
// 8-B record of the tile that holds it (tix; always legal addresses); returns zc, or +inf for a voxel that is not in front of
// zmin or whose pixel lies outside the image ("behind everything": no update).
__device__ __forceinline__ float pair_project(const Cam &cam, float r0, float r1, float r2, float r3, float r4, float r5, float r6, float r7, float r8,
                                              float t0, float t1, float t2, float wxs, float wys, float wzs, float zmin, unsigned row_bytes,
                                              unsigned pix_bytes, int ntx0, unsigned &pix, unsigned &tix) {
    const float xc = fmaf(r0, wxs, fmaf(r1, wys, fmaf(r2, wzs, t0)));
    const float yc = fmaf(r3, wxs, fmaf(r4, wys, fmaf(r5, wzs, t1)));
    const float zc = fmaf(r6, wxs, fmaf(r7, wys, fmaf(r8, wzs, t2)));
    // 1 / zc.  v_rcp_f32 + one Newton step equals the IEEE quotient for EVERY float with 2^-126 <= zc < 2^126 (exhaustive:
    // tools/ubench_rcp.hip, profiles/r03_ubench_rcp.txt); the division proper (~10 instructions) runs only for lanes outside
    // that range (a voxel centre within 1e-38 m of the camera plane, or absurdly far) -- the value is the oracle's either way.
    float inv = __builtin_amdgcn_rcpf(zc);
    inv = fmaf(fmaf(-zc, inv, 1.0f), inv, inv);
    if (__builtin_expect(!(zc >= 1.17549435e-38f && zc < 8.5e37f), 0)) inv = 1.0f / zc;
    const float uf = fmaf(cam.fx * xc, inv, cam.cx);
    const float vf = fmaf(cam.fy * yc, inv, cam.cy);
    // nearest pixel floor(uf + 0.5) in ONE conversion (v_cvt_flr_i32_f32 == v_floor_f32 + v_cvt_i32_f32 on every bit
    // pattern), and the window  -0.5 <= uf < W - 0.5  as ONE unsigned compare of it  (the same decision for every float
    // and every width: tools/ubench_flr.hip, exhaustive)
    const int ui = cvt_flr_i32(uf + 0.5f), vi = cvt_flr_i32(vf + 0.5f);
    const bool ok = (zc > zmin) & ((unsigned)ui <= (unsigned)(cam.W - 1)) & ((unsigned)vi <= (unsigned)(cam.H - 1));
    const int u = clamp_i32(ui, cam.W - 1), v = clamp_i32(vi, cam.H - 1);     // always a legal address, so the loads need no branch
    // BYTE offsets of the pixel in the image and of the 8-B record of the 8x8-pixel tile that holds it
    pix = mad_u24((unsigned)v, row_bytes, (unsigned)u * pix_bytes);
    tix = mad_u24((unsigned)v >> TILE0_SHIFT, (unsigned)ntx0 << 3, (unsigned)u & ~7u);
    return ok ? zc : INFINITY;
}
// pair_tile_test: tl = the tile's record (lowest depth if all 64 pixels are valid else -inf, highest valid depth), zc as
// pair_project returns it.  fre: tsdf == 1 exactly whatever the pixel says; skp: no update whatever the pixel says.
__device__ __forceinline__ void pair_tile_test(float2 tl, float zc, float trunc_free, float trunc, bool &fre, bool &skp) {
    fre = tl.x - zc >= trunc_free;
    skp = !(tl.y - zc >= -trunc);
}

// A record is read, added to and written ONCE per launch: nothing in the launch asks for it again, so its 2 x 8 B per voxel go
// through the caches as non-temporal traffic.  Measured: the kernel 8 us of 325 shorter, 2 % fewer requests to the
// fabric; that the depth lines neighbours share stay cached longer for it is supposed, the counters do not show it.
typedef int rec_v2i __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int2 rec_load_nt(const int2 *p) {
    const rec_v2i v = __builtin_nontemporal_load(reinterpret_cast<const rec_v2i *>(p));
    return make_int2(v.x, v.y);
}
__device__ __forceinline__ void rec_store_nt(int2 *p, int2 r) {
    rec_v2i v;
    v.x = r.x; v.y = r.y;
    __builtin_nontemporal_store(v, reinterpret_cast<rec_v2i *>(p));
}

#ifdef TL3D_EXPERIMENTS
constexpr unsigned UPD_SPAN_WAVES = 65536;
__device__ unsigned long long g_upd_span[UPD_SPAN_WAVES][2];   // experiments: start / end (100 MHz real-time clock) of every wave of the last stamped launch
#endif
constexpr int UPD_WAVES = 8;             // waves per SIMD the pair kernel is built for (64 vector registers)
// the depth-gather latency (LAT below) the library ships: 2 for both depth formats (f32 +3.0 %, 16-bit +2.4 % frames/s against 1:
// profiles/update_depth_latency_ab.txt); the counting instantiations, not on a timed path, would need 66 vector registers at 2
template <bool COUNT, typename DT> struct PairsLat { static constexpr int value = 1; };
template <typename DT> struct PairsLat<false, DT> { static constexpr int value = 2; };

// EXP (experiments flavour only, results incomplete): bit 0 tile records read at lane * 8 (coalesced), bit 1 every lane reads the frame's
// valid pixel (no scattered depth reads), bit 2 no LDS add, bit 3 no record accesses
// LAT: the steps between stage B of a pair (depth gather issued) and its stage C (depth value used)
template <bool COUNT, typename DT, int EXP = 0, int LAT = PairsLat<COUNT, DT>::value>
__global__ __launch_bounds__(256, UPD_WAVES) void tsdf_update_pairs_kernel(Cam cam, Grid g, BatchBufs B, float mind, float maxd,
                                                                           int2 *__restrict__ grid, unsigned long long *__restrict__ counters) {
    static_assert(LAT >= 1 && LAT <= 3, "the step is unrolled for LAT 1..3");
    constexpr int RING = LAT + 1;                                 // entries of the B -> C rings
    constexpr int UNROLL = (RING % 2) ? 2 * RING : RING;          // steps per loop body: the A -> B parity and the rings both come round
    __shared__ unsigned s_acc[4 * 512];                           // per wave: [8 sub-bricks][64 lanes] packed running sums
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned *const acc = s_acc + wid * 512 + lane;               // + 64 s
    const unsigned nbricks = (unsigned)(g.nbx * g.nby * g.nbz);
    // the trip count comes from device memory: clamp it to what the list can hold, so that no ordering mistake upstream can
    // ever turn into an unbounded loop or an out-of-range list read
    const unsigned ntask = min(B.hdr[0], nbricks);
    unsigned nread = 0, nwritten = 0;
    // Work distribution.  A brick costs one step per (frame, MIXED sub-brick) that lists it (1 .. 256), so a static share of the
    // list leaves waves idle for a third of the launch.  Tasks are handed out by TICKET instead: the workgroups form up to 64
    // groups (blockIdx % groups), group g owns list entries g, g + groups, g + 2 groups, ... (every group sees the same mix of
    // cheap and dear bricks) and a ticket counter of its own (64-B apart; a few hundred returning atomics per counter and
    // launch, handed out two tasks ahead of their use, so nobody waits for one).  A wave's first task needs no ticket: entry
    // bi * 4 + wid of its group, dearest first.  The launch has four times the workgroups the chip holds at once (tl3d_api.hip),
    // so most first tasks wait with a workgroup that has not started: the dispatcher starts it in the very slot a wave retires
    // from, which hands those bricks out one at a time and later than any ticket is committed (a wave holds its tickets two
    // tasks ahead).  At the headline shape the launch has a wave for four of every five list entries; tickets carry the rest,
    // the cheapest bricks, and whatever a longer list leaves.  Measured, not assumed: late workgroups that take their first task by ticket instead
    // make the kernel 7 % slower.  A ticket far beyond the list saturates (entry_of): it must not wrap into it.
    const unsigned ngrp = min((unsigned)TICKET_GROUPS, gridDim.x);
    const unsigned grp = blockIdx.x % ngrp, bi = blockIdx.x / ngrp;
    const unsigned waves_in_group = ((gridDim.x - grp + ngrp - 1u) / ngrp) * 4u;
    unsigned *__restrict__ ticket = B.hdr + HDR_TICKETS + 16u * grp;
    auto entry_of = [&](unsigned k) -> unsigned { return k >= 0x2000000u ? 0xffffffffu : k * ngrp + grp; };
    const DescPtr frames = const_descs(B);
    const int ntx0 = (cam.W + TILE0 - 1) >> TILE0_SHIFT;
    const unsigned row_bytes = (unsigned)cam.W * (unsigned)sizeof(DT);
    // the longer rings take scalar registers (80 a wave at this occupancy, all in use): constants that only the vector arithmetic
    // of stages B and C reads move to vector registers, where there is room
    const float c_mind = LAT > 1 ? keep_vector(mind) : mind, c_maxd = LAT > 1 ? keep_vector(maxd) : maxd;
    const float c_inv_trunc = LAT > 1 ? keep_vector(g.inv_trunc) : g.inv_trunc;
    const float trunc_free = LAT > 1 ? keep_vector(g.trunc * 1.001f) : g.trunc * 1.001f;

    auto fetch = [&](unsigned t, unsigned &brick, unsigned &fm, unsigned &subv, unsigned &slot) {
        brick = min((unsigned)__builtin_amdgcn_readfirstlane((int)B.order[t]), nbricks - 1u);
        fm = (unsigned)__builtin_amdgcn_readfirstlane((int)B.framemask[brick]);
        slot = (unsigned)__builtin_amdgcn_readfirstlane((int)brick_slot(g.tsdf_tab, brick));
        subv = 0u;
        if (lane < B.n_frames && ((fm >> lane) & 1u)) subv = frames[lane].sub[brick];
    };
    auto take_ticket = [&]() -> unsigned {
        unsigned k = 0;
        if (lane == 0) k = atomicAdd(ticket, 1u);
        return (unsigned)__builtin_amdgcn_readfirstlane((int)k) + waves_in_group;
    };
    unsigned t = entry_of(bi * 4u + (unsigned)wid);
    unsigned brick_n = 0, fm_n = 0, subv_n = 0, slot_n = 0;
    if (t < ntask) fetch(t, brick_n, fm_n, subv_n, slot_n);
    unsigned k_next = t < ntask ? take_ticket() : 0u;
    unsigned long long pf_t0 = 0, pf_setup = 0, pf_loop = 0, pf_rmw = 0, pf_bricks = 0, pf_steps = 0, pf_a = 0, pf_b = 0;
    unsigned long long pf_rt0 = 0;
    if (EXP & 16) pf_t0 = pf_a = __builtin_readcyclecounter();
    if (EXP & 32) pf_rt0 = __builtin_amdgcn_s_memrealtime();      // light mode: only the start and the end of every wave (the heavy stamps of bit 4 slow the kernel threefold)
    while (t < ntask) {
        const unsigned brick = brick_n, slot = slot_n;
        unsigned subv = subv_n;
        if (lane == 0) B.framemask[brick] = 0u;                   // re-armed for the next batch that uses this buffer
        const unsigned t_next = entry_of(k_next);
        if (t_next < ntask) {
            fetch(t_next, brick_n, fm_n, subv_n, slot_n);
            k_next = take_ticket();
        }
        t = t_next;
        if (lane >= B.n_frames) subv = 0u;
        const int bx = (int)(brick % (unsigned)g.nbx), by = (int)((brick / (unsigned)g.nbx) % (unsigned)g.nby), bz = (int)(brick / (unsigned)(g.nbx * g.nby));
        // the lane's voxel in sub-brick s is (4 (s & 1) + (lane & 3), 4 (s >> 1 & 1) + (lane >> 2 & 3), 4 (s >> 2) + (lane >> 4)); its
        // centre along an axis: fma(i + 0.5, voxel, origin) with i the LATTICE index (the grid's offset + its own: one scalar add
        // per brick; a multiple of 8, so the in-brick part goes in with an OR: 55 VGPRs, where an add took 58) -- two values per axis
        // (named scalars: an array indexed by a bit of s would be moved to LDS by the compiler)
        const int lx = g.vox + bx * 8, ly = g.voy + by * 8, lz = g.voz + bz * 8;
        const float wx0 = fmaf((float)(lx | (lane & 3)) + 0.5f, g.vs, g.ox), wx1 = fmaf((float)(lx | 4 | (lane & 3)) + 0.5f, g.vs, g.ox);
        const float wy0 = fmaf((float)(ly | ((lane >> 2) & 3)) + 0.5f, g.vs, g.oy), wy1 = fmaf((float)(ly | 4 | ((lane >> 2) & 3)) + 0.5f, g.vs, g.oy);
        const float wz0 = fmaf((float)(lz | (lane >> 4)) + 0.5f, g.vs, g.oz), wz1 = fmaf((float)(lz | 4 | (lane >> 4)) + 0.5f, g.vs, g.oz);
        // the brick's pairs: lane f holds frame f's masks.  Pairs = set MIXED bits; FREE sub-bricks are counted per sub-brick over
        // the frames and start the running sums; touched = sub-bricks anything adds to
        unsigned npairs = 0, touched = 0;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const unsigned long long bm = __ballot((subv >> s) & 1u), bf = __ballot((subv >> (8 + s)) & 1u);
            npairs += (unsigned)__popcll(bm);
            touched |= (bm | bf) ? (1u << s) : 0u;
            acc[64 * s] = (unsigned)__popcll(bf) * (65535u + (1u << 21));
        }
        npairs = keep_scalar(npairs);                                          // (computed now: the sixteen ballots die here)
        touched = keep_scalar(touched);
        unsigned rest = (unsigned)__ballot((subv & 0xffu) != 0u);              // frames with at least one MIXED sub-brick (lanes 0..31)
        if (EXP & 16) { pf_b = __builtin_readcyclecounter(); pf_setup += pf_b - pf_a; pf_bricks += 1; pf_steps += npairs; }
        if (npairs) {
            // ---- scalars of the frame stage A works in, of the pair stage B works on, of the LAT + 1 pairs on their way to stage C
            float r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0, r6 = 0, r7 = 0, r8 = 0, t0 = 0, t1 = 0, t2 = 0, a_sc = 0;
            unsigned a_vp = 0, m = 0;
            const char *a_vt = nullptr, *a_img = nullptr;
            auto switch_frame = [&]() {
                const int f = __builtin_ctz(rest);
                rest &= rest - 1u;
                m = (unsigned)__builtin_amdgcn_readlane((int)subv, f) & 0xffu;
                const DescPtr F = frames + f;
                r0 = F->pose.r[0]; r1 = F->pose.r[1]; r2 = F->pose.r[2]; r3 = F->pose.r[3]; r4 = F->pose.r[4]; r5 = F->pose.r[5];
                r6 = F->pose.r[6]; r7 = F->pose.r[7]; r8 = F->pose.r[8]; t0 = F->pose.t[0]; t1 = F->pose.t[1]; t2 = F->pose.t[2];
                a_sc = F->c.sc;
                a_vp = F->valid_pix * (unsigned)sizeof(DT);
                a_vt = reinterpret_cast<const char *>(F->vtile);
                a_img = static_cast<const char *>(F->depth);
            };
            switch_frame();
            const char *b_img = a_img;
            unsigned b_vp = a_vp;
            // ---- the hand-down from B to C, rings of LAT + 1 entries indexed by the pair number mod (LAT + 1): wave-uniform
            // (sub-brick, the frame's depth scale, "some voxel of the pair is left to its depth pixel") and per lane (zc / +-inf,
            // depth).  All indices are compile-time constants of the unrolled step: named registers, no moves
            float c_sc[RING];
            unsigned c_s[RING];
            bool c_open[RING];
            float zcB[RING];
            typename PixLoad<DT>::raw dvB[RING];
#pragma unroll
            for (int i = 0; i < RING; ++i) { c_sc[i] = a_sc; c_s[i] = 0u; c_open[i] = false; zcB[i] = INFINITY; dvB[i] = 0; }
            // ---- A -> B, by the parity of the pair: zc or +inf, pixel offset, tile record
            float zcA[2] = {INFINITY, INFINITY};
            unsigned pixA[2] = {0u, 0u};
            float2 tlA[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};
            if (EXP & 16) pf_steps += (unsigned long long)(npairs + 1u + (unsigned)LAT) << 32;   // steps run, above the pairs
            // ONE spelling of the stages.  A full step runs A(k), C(k - 1 - LAT), B(k - 1); the drain steps behind the brick's last
            // pair run the stages that still have a pair: `stages` (bit 0 A, bit 1 B; C always) is a compile-time argument
            auto step = [&](const int j, auto stages) {                         // j = the step's number mod UNROLL, a literal at every call
                constexpr bool ST_A = (decltype(stages)::value & 1) != 0, ST_B = (decltype(stages)::value & 2) != 0;
                const int par = j & 1, rc = j % RING, rb = (j + LAT) % RING;   // rings: pair k's and pair k-1-LAT's slot; pair k-1's
                // ---- A(k): the lane's voxel of sub-brick s in the current frame -> pixel, tile record (k < npairs: the mask has a bit)
                const char *n_img = a_img;
                unsigned n_vp = a_vp, n_s = 0u;
                float n_sc = a_sc;
                if constexpr (ST_A) {
                    const unsigned s = (unsigned)__builtin_ctz(m);
                    m &= m - 1u;
                    {
                        const float wxs = (s & 1u) ? wx1 : wx0, wys = (s & 2u) ? wy1 : wy0, wzs = (s & 4u) ? wz1 : wz0;
                        unsigned tix;
                        zcA[par] = pair_project(cam, r0, r1, r2, r3, r4, r5, r6, r7, r8, t0, t1, t2, wxs, wys, wzs, 0.0f, row_bytes, (unsigned)sizeof(DT), ntx0,
                                                pixA[par], tix);
                        tlA[par] = *reinterpret_cast<const float2 *>(a_vt + ((EXP & 1) ? (unsigned)lane * 8u : tix));
                    }
                    // the scalars pair k hands down the pipeline, then -- its frame used up -- the next frame's (the loads have stages C
                    // and B to arrive in)
                    n_s = s;
                    if (m == 0u && rest != 0u) switch_frame();
                }
                // ---- C(k - 1 - LAT): depth value -> increment of the running sum.  A pair whose every voxel the tiles decided (two in five)
                // has only "in front of everything" lanes (zc = -inf: tsdf = 1 exactly, and the pixel they read is valid) and "behind
                // everything" lanes: no arithmetic
                {
                    const float zc = zcB[rc];
                    unsigned inc;
                    if (c_open[rc]) {
                        const float d = PixLoad<DT>::value(dvB[rc]) * c_sc[rc];
                        const float sdf = d - zc;
                        const bool ok = (d > c_mind && d < c_maxd) && (sdf >= -g.trunc);
                        const float tsdf = fminf(1.0f, sdf * c_inv_trunc);
                        const int q = (int)rintf(tsdf * 32767.0f);
                        inc = ok ? (unsigned)(q + 32768) + (1u << 21) : 0u;
                    } else {
                        inc = (zc < 0.0f) ? 65535u + (1u << 21) : 0u;
                    }
                    if (!(EXP & 4) || inc == 0x12345u) (void)__hip_atomic_fetch_add(acc + 64u * c_s[rc], inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                }
                // ---- B(k - 1): what the tile leaves open gathers its pixel; the decided lanes read the frame's valid pixel
                if constexpr (ST_B) {
                    const float zc = zcA[par ^ 1];
                    bool fre, skp;
                    pair_tile_test(tlA[par ^ 1], zc, trunc_free, g.trunc, fre, skp);
                    zcB[rb] = fre ? -INFINITY : (skp ? INFINITY : zc);
                    const unsigned pix = ((EXP & 2) || fre || skp) ? b_vp : pixA[par ^ 1];
                    dvB[rb] = PixLoad<DT>::load(b_img, pix);
                    c_open[rb] = __ballot(!(fre || skp)) != 0ull;
                }
                if constexpr (ST_A) {
                    b_img = n_img; b_vp = n_vp;
                    c_sc[rc] = n_sc; c_s[rc] = n_s;                             // (C of this step has read slot rc)
                }
            };
            constexpr std::integral_constant<int, 7> FULL{};
            constexpr std::integral_constant<int, 6> DRAIN_BC{};
            constexpr std::integral_constant<int, 4> DRAIN_C{};
            // P pairs take P + 1 + LAT steps: whole bodies of full steps in the steady loop and nothing else ...
            const unsigned bodies = UNROLL == 6 ? (npairs * 43691u) >> 18 : npairs / (unsigned)UNROLL;   // (P <= 256; a shift at 2 and 4)
            const unsigned left = npairs - bodies * (unsigned)UNROLL;
            for (unsigned b = bodies; b != 0u; --b) {
                step(0, FULL);
                step(1, FULL);
                if constexpr (UNROLL > 2) { step(2, FULL); step(3, FULL); }
                if constexpr (UNROLL > 4) { step(4, FULL); step(5, FULL); }
            }
            // ... the full steps that are left, fewer than UNROLL, in straight-line code, each behind one forward branch ...
            if (left > 0u) step(0, FULL);
            if constexpr (UNROLL > 2) {
                if (left > 1u) step(1, FULL);
                if (left > 2u) step(2, FULL);
            }
            if constexpr (UNROLL > 4) {
                if (left > 3u) step(3, FULL);
                if (left > 4u) step(4, FULL);
            }
            // ... and the drain for the ring phase the last pair left: B of that pair with C of pair P - 1 - LAT, then C of the LAT
            // pairs still on their way -- no projection, no tile record, one depth load.  The waits are the compiler's
            auto drain = [&](const int j) {
                step(j, DRAIN_BC);
                step((j + 1) % UNROLL, DRAIN_C);
                if constexpr (LAT > 1) step((j + 2) % UNROLL, DRAIN_C);
                if constexpr (LAT > 2) step((j + 3) % UNROLL, DRAIN_C);
            };
            switch (left) {
                case 0: drain(0); break;
                case 1: drain(1); break;
                case 2: if constexpr (UNROLL > 2) drain(2); break;
                case 3: if constexpr (UNROLL > 2) drain(3); break;
                case 4: if constexpr (UNROLL > 4) drain(4); break;
                default: if constexpr (UNROLL > 4) drain(5); break;
            }
        }
        if (EXP & 16) { pf_a = __builtin_readcyclecounter(); pf_loop += pf_a - pf_b; }
        if (touched == 0u || slot >= SLOT_FULL) continue;                       // (a full pool: counted when the slot was refused)
        if ((EXP & 8) && acc[0] != 0x7654321u) continue;
        // the records that change: read, add, write -- once per batch
        int2 *__restrict__ recs = grid + ((size_t)slot << 9);
        unsigned a[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) a[s] = ((touched >> s) & 1u) ? acc[64 * s] : 0u;
        int2 rec[8];
#pragma unroll
        for (int s = 0; s < 8; ++s)
            if (a[s] >> 21) rec[s] = rec_load_nt(recs + s * 64 + lane);
#pragma unroll
        for (int s = 0; s < 8; ++s)
            if (a[s] >> 21) {
                const int w = (int)(a[s] >> 21);
                rec[s].x += (int)(a[s] & 0x1fffffu) - 32768 * w;
                rec[s].y += w;
                rec_store_nt(recs + s * 64 + lane, rec[s]);
                if (COUNT) { nread += 1; nwritten += 1; }
            }
        if (EXP & 16) { const unsigned long long now = __builtin_readcyclecounter(); pf_rmw += now - pf_a; pf_a = now; }
    }
#ifdef TL3D_EXPERIMENTS
    if ((EXP & 32) && lane == 0) {
        const unsigned wv = blockIdx.x * 4u + (unsigned)wid;
        if (wv < UPD_SPAN_WAVES) { g_upd_span[wv][0] = pf_rt0; g_upd_span[wv][1] = __builtin_amdgcn_s_memrealtime(); }
        if (wv == 0) atomicAdd(counters + 14, 1ull);
    }
#endif
    if ((EXP & 16) && lane == 0) {                             // experiments: where a wave's time goes (s_memtime ticks)
        atomicAdd(counters + 8, pf_setup); atomicAdd(counters + 9, pf_loop); atomicAdd(counters + 10, pf_rmw);
        atomicAdd(counters + 11, __builtin_readcyclecounter() - pf_t0); atomicAdd(counters + 12, pf_bricks); atomicAdd(counters + 13, pf_steps);
        atomicAdd(counters + 14, 1ull);
        atomicMax(counters + 15, __builtin_readcyclecounter() - pf_t0);
    }
    if (COUNT) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            nread += __shfl_down(nread, d);
            nwritten += __shfl_down(nwritten, d);
        }
        if (lane == 0) {
            atomicAdd(counters + 2, (unsigned long long)nread);
            atomicAdd(counters + 3, (unsigned long long)nwritten);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            unsigned long long vis = 0, fre = 0;
            for (int f = 0; f < B.n_frames; ++f) {
                const unsigned l = min(frames[f].counts[0], nbricks), fc = min(frames[f].counts[1], nbricks - l);
                vis += l + fc; fre += fc;
            }
            atomicAdd(counters + 4, vis);
            atomicAdd(counters + 5, fre);
            atomicAdd(counters + 6, fre);
            atomicAdd(counters + 7, (unsigned long long)ntask);
        }
    }
}

// ---- the refinement of cached sub-brick masks: a kernel of the prep chain that lives with the update ----------------------------
// It is here, not in kernels_tsdf_prep.hip with the cache's other kernels, for two reasons.  Its decision must be the update
// kernel's, bit for bit, so pair_project and pair_tile_test have these two users and no other, side by side.  And alone in a
// module it would be pair_project's ONLY caller: the compiler then specialises the function for its constant arguments before
// inlining it, and the kernel's code changes (tried: five scalar instructions of its loop head change order and registers).
// The REFINEMENT of a replayed level-2 entry (ClassPlan::refine: the host's choice -- a fusion chain that holds the slot once;
// the header's: the entry fit and is at level 2), behind the replay and in front of everything that reads the masks.  A MIXED
// sub-brick is a PAIR of the update: 64 lanes = its 64 voxels, through the update's own stage A and tile test (pair_project,
// pair_tile_test: the same decision per lane, bit for bit).  A pair whose every lane the tiles decide needs no depth pixel, and
// what the update would add for it is fixed by the key the entry was made under:
//   every lane "behind everything"     the pair adds nothing: its MIXED bit goes;
//   every lane "in front of everything" every voxel gets exactly (32767, 1), what a FREE sub-brick gets: MIXED bit -> FREE bit
//                                       (the update counts it with a ballot: no pipeline step);
//   both kinds, no open lane            counted only (stats[7]): no mask bit can say which lane is which.
// The new mask goes to the frame's sub[] of this batch and to the entry; class_finish_kernel marks the entry level 3.  Brick
// lists, free-space counts and pool slots are not touched: a brick whose pairs all vanish stays listed.
// stats[4..8]: pairs seen, dropped, turned FREE, decided with both kinds of lane, (masks that did not fit: none are kept);
// counted per frame here and folded into the context's words by class_finish_kernel.
__global__ __launch_bounds__(256) void class_refine_kernel(Cam cam, Grid g, BatchBufs B, ClassPlan P) {
    const int f = blockIdx.y;
    if (!((P.refine >> f) & 1u) || !class_replays(P, f)) return;
    unsigned *__restrict__ C = P.cache[f];
    if (C[2] != 2u) return;
    const DescPtr F = const_descs(B) + f;
    __shared__ unsigned s_cnt[4];
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned nbricks = (unsigned)(g.nbx * g.nby * g.nbz), cap = P.cap;
    const unsigned nm = min(C[0], cap);
    unsigned short *__restrict__ cm = reinterpret_cast<unsigned short *>(C + CC_HDR_WORDS + cap);
    unsigned short *__restrict__ sub = F->sub;
    const float r0 = F->pose.r[0], r1 = F->pose.r[1], r2 = F->pose.r[2], r3 = F->pose.r[3], r4 = F->pose.r[4], r5 = F->pose.r[5];
    const float r6 = F->pose.r[6], r7 = F->pose.r[7], r8 = F->pose.r[8], t0 = F->pose.t[0], t1 = F->pose.t[1], t2 = F->pose.t[2];
    const char *vt = reinterpret_cast<const char *>(F->vtile);
    const int ntx0 = (cam.W + TILE0 - 1) >> TILE0_SHIFT;
    const float trunc_free = g.trunc * 1.001f;
    unsigned seen = 0, dropped = 0, freed = 0, both = 0;
    for (unsigned i = blockIdx.x * 4u + (unsigned)wid; i < nm; i += gridDim.x * 4u) {
        const unsigned brick = min((unsigned)__builtin_amdgcn_readfirstlane((int)C[CC_HDR_WORDS + i]), nbricks - 1u);
        const unsigned m0 = (unsigned)__builtin_amdgcn_readfirstlane((int)cm[i]);
        if ((m0 & 0xffu) == 0u) continue;
        const int bx = (int)(brick % (unsigned)g.nbx), by = (int)((brick / (unsigned)g.nbx) % (unsigned)g.nby), bz = (int)(brick / (unsigned)(g.nbx * g.nby));
        // the lane's voxel centres, exactly as the update kernel forms them
        const int lx = g.vox + bx * 8, ly = g.voy + by * 8, lz = g.voz + bz * 8;
        const float wx0 = fmaf((float)(lx | (lane & 3)) + 0.5f, g.vs, g.ox), wx1 = fmaf((float)(lx | 4 | (lane & 3)) + 0.5f, g.vs, g.ox);
        const float wy0 = fmaf((float)(ly | ((lane >> 2) & 3)) + 0.5f, g.vs, g.oy), wy1 = fmaf((float)(ly | 4 | ((lane >> 2) & 3)) + 0.5f, g.vs, g.oy);
        const float wz0 = fmaf((float)(lz | (lane >> 4)) + 0.5f, g.vs, g.oz), wz1 = fmaf((float)(lz | 4 | (lane >> 4)) + 0.5f, g.vs, g.oz);
        // all tile records of the brick's pairs are asked for before the first is looked at
        float zc[8];
        float2 tl[8];
#pragma unroll
        for (unsigned s = 0; s < 8u; ++s) {
            zc[s] = INFINITY;
            tl[s] = make_float2(0.0f, 0.0f);
            if ((m0 >> s) & 1u) {
                const float wxs = (s & 1u) ? wx1 : wx0, wys = (s & 2u) ? wy1 : wy0, wzs = (s & 4u) ? wz1 : wz0;
                unsigned pix, tix;
                zc[s] = pair_project(cam, r0, r1, r2, r3, r4, r5, r6, r7, r8, t0, t1, t2, wxs, wys, wzs, 0.0f, (unsigned)cam.W * 4u, 4u, ntx0, pix, tix);
                tl[s] = *reinterpret_cast<const float2 *>(vt + tix);
            }
        }
        unsigned m = m0;
#pragma unroll
        for (unsigned s = 0; s < 8u; ++s)
            if ((m0 >> s) & 1u) {
                bool fre, skp;
                pair_tile_test(tl[s], zc[s], trunc_free, g.trunc, fre, skp);
                const unsigned long long bfre = __ballot(fre), bskp = __ballot(skp);
                seen += 1u;
                if (bskp == ~0ull) { m &= ~(1u << s); dropped += 1u; }
                else if (bfre == ~0ull) { m = (m & ~(1u << s)) | (1u << (8u + s)); freed += 1u; }
                else if ((bfre | bskp) == ~0ull) both += 1u;
            }
        if (m != m0 && lane == 0) {
            cm[i] = (unsigned short)m;
            sub[brick] = (unsigned short)m;
        }
    }
    // the counts: pooled per workgroup, then into the FRAME's counts block (one address per frame and kind: adds to one address
    // retire one after the other, and 32 k waves adding to the context's four words took longer than the kernel's work);
    // class_finish_kernel folds them into the context's
    if (lane == 0 && seen) {
        atomicAdd(&s_cnt[0], seen);
        if (dropped) atomicAdd(&s_cnt[1], dropped);
        if (freed) atomicAdd(&s_cnt[2], freed);
        if (both) atomicAdd(&s_cnt[3], both);
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(F->counts + REFINE_COUNTS + threadIdx.x, s_cnt[threadIdx.x]);
}

// over the B.n_frames frames of a chain; one wave per cached MIXED brick, a fixed grid strides over each list
int launch_class_refine(hipStream_t s, const Cam &cam, const Grid &g, const BatchBufs &B, const ClassPlan &P) {
    const unsigned quads = (P.cap + 3u) / 4u;
    hipLaunchKernelGGL(class_refine_kernel, dim3(quads < 256u ? quads : 256u, B.n_frames), dim3(256), 0, s, cam, g, B, P);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

// the dominant kernel: ONE read-modify-write pass over the bricks the n prepared frames of the batch list
int launch_tsdf_update(hipStream_t s, const Cam &cam, const Grid &g, int n, int max_frames, bool depth_u16, float mind, float maxd, int2 *grid,
                       void *scratch, unsigned long long *counters, bool count, int max_blocks) {
    const BatchLayout L = batch_layout(g, max_frames);
    BatchBufs B = batch_bufs(L, scratch, n);
    if (n == 1) B.order = B.list;
    const int nbricks = g.nbx * g.nby * g.nbz;
    int nblk = (nbricks + 3) / 4;
    if (nblk > max_blocks) nblk = max_blocks;
#ifdef TL3D_EXPERIMENTS
    static const int no_order = getenv("TL3D_NO_ORDER") ? atoi(getenv("TL3D_NO_ORDER")) : 0;     // walk the list as the classification left it
    if (no_order) B.order = B.list;
    static const int pexp = getenv("TL3D_PAIRS_EXP") ? atoi(getenv("TL3D_PAIRS_EXP")) : 0;
    static const int plat = getenv("TL3D_PAIRS_LAT") ? atoi(getenv("TL3D_PAIRS_LAT")) : 0;       // A/B on one box: 1..3, else what ships
#define TL3D_LAUNCH_PEXP_L(E_, L_) \
    hipLaunchKernelGGL((tsdf_update_pairs_kernel<false, float, E_, L_>), dim3(nblk), dim3(256), 0, s, cam, g, B, mind, maxd, grid, counters)
#define TL3D_LAUNCH_PEXP(E_) TL3D_LAUNCH_PEXP_L(E_, (PairsLat<false, float>::value))
#define TL3D_LAUNCH_PEXP_BY_LAT(E_) /* the modes that are run per LAT: no depth gathers, stamps */ \
    do {                                                                                           \
        if (plat == 1) TL3D_LAUNCH_PEXP_L(E_, 1); else if (plat == 2) TL3D_LAUNCH_PEXP_L(E_, 2);   \
        else if (plat == 3) TL3D_LAUNCH_PEXP_L(E_, 3); else TL3D_LAUNCH_PEXP(E_);                  \
    } while (0)
    if (pexp && !count && !depth_u16) {
        switch (pexp) {
            case 1: TL3D_LAUNCH_PEXP(1); break;
            case 2: TL3D_LAUNCH_PEXP_BY_LAT(2); break;
            case 3: TL3D_LAUNCH_PEXP(3); break;
            case 4: TL3D_LAUNCH_PEXP(4); break;
            case 7: TL3D_LAUNCH_PEXP(7); break;
            case 8: TL3D_LAUNCH_PEXP(8); break;
            case 16: TL3D_LAUNCH_PEXP_BY_LAT(16); break;
            case 32: TL3D_LAUNCH_PEXP(32); break;
            default: TL3D_LAUNCH_PEXP(15); break;
        }
        TL3D_HIP(hipGetLastError());
        return TL3D_OK;
    }
#undef TL3D_LAUNCH_PEXP_BY_LAT
#undef TL3D_LAUNCH_PEXP
#undef TL3D_LAUNCH_PEXP_L
#define TL3D_LAUNCH_PLAT(L_)                                                                                                                       \
    do {                                                                                                                                           \
        if (depth_u16) hipLaunchKernelGGL((tsdf_update_pairs_kernel<false, uint16_t, 0, L_>), dim3(nblk), dim3(256), 0, s, cam, g, B, mind, maxd,  \
                                          grid, counters);                                                                                         \
        else hipLaunchKernelGGL((tsdf_update_pairs_kernel<false, float, 0, L_>), dim3(nblk), dim3(256), 0, s, cam, g, B, mind, maxd, grid,         \
                                counters);                                                                                                         \
    } while (0)
    if (plat >= 1 && plat <= 3 && !count) {
        if (plat == 1) TL3D_LAUNCH_PLAT(1); else if (plat == 2) TL3D_LAUNCH_PLAT(2); else TL3D_LAUNCH_PLAT(3);
        TL3D_HIP(hipGetLastError());
        return TL3D_OK;
    }
#undef TL3D_LAUNCH_PLAT
#endif
#define TL3D_LAUNCH_PAIRS(C_, T_) \
    hipLaunchKernelGGL((tsdf_update_pairs_kernel<C_, T_>), dim3(nblk), dim3(256), 0, s, cam, g, B, mind, maxd, grid, counters)
    if (count) {
        if (depth_u16) TL3D_LAUNCH_PAIRS(true, uint16_t); else TL3D_LAUNCH_PAIRS(true, float);
    } else {
        if (depth_u16) TL3D_LAUNCH_PAIRS(false, uint16_t); else TL3D_LAUNCH_PAIRS(false, float);
    }
#undef TL3D_LAUNCH_PAIRS
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

#ifdef TL3D_EXPERIMENTS
// when the waves of the last stamped launch started and ended (TL3D_PAIRS_EXP=32), and how the waves of the workgroups at or
// above `late_from` (8 x CUs: those the chip cannot hold from the start) fared
void tsdf_debug_print_spans(int nwaves, int late_from) {
    static unsigned long long h[UPD_SPAN_WAVES][2];
    if (nwaves > (int)UPD_SPAN_WAVES) nwaves = (int)UPD_SPAN_WAVES;
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_upd_span), sizeof(h)) != hipSuccess) return;
    unsigned long long t0 = ~0ull, t1 = 0;
    for (int i = 0; i < nwaves; ++i) if (h[i][0]) { if (h[i][0] < t0) t0 = h[i][0]; if (h[i][1] > t1) t1 = h[i][1]; }
    if (t1 <= t0) return;
    const double span = (double)(t1 - t0);
    int hs[10] = {0}, he[10] = {0}, nlate = 0, nfirst = 0, nidle = 0;
    double late_start = 0, late_life = 0, first_life = 0;
    for (int i = 0; i < nwaves; ++i)
        if (h[i][0]) {
            const int bs = (int)(10.0 * (double)(h[i][0] - t0) / span), be = (int)(10.0 * (double)(h[i][1] - t0) / span);
            const double life = (double)(h[i][1] - h[i][0]);
            hs[bs > 9 ? 9 : bs]++;
            he[be > 9 ? 9 : be]++;
            if (i / 4 < late_from) { nfirst++; first_life += life; }
            else if (life < 100.0) nidle++;                                   // under 1 us: a wave that found the list used up
            else { nlate++; late_start += (double)(h[i][0] - t0); late_life += life; }
        }
    fprintf(stderr, "[tl3d exp] launch %.1f us; waves STARTING in each tenth of it:", span * 0.01);
    for (int i = 0; i < 10; ++i) fprintf(stderr, " %d", hs[i]);
    fprintf(stderr, "; ENDING:");
    for (int i = 0; i < 10; ++i) fprintf(stderr, " %d", he[i]);
    fprintf(stderr, "\n[tl3d exp] waves of workgroups < %d: %d, mean lifetime %.1f us;  >= %d: %d with work, mean start %.1f us, mean lifetime %.1f us, and %d that found none\n",
            late_from, nfirst, nfirst ? first_life * 0.01 / nfirst : 0.0, late_from, nlate, nlate ? late_start * 0.01 / nlate : 0.0,
            nlate ? late_life * 0.01 / nlate : 0.0, nidle);
}
#endif

}  // namespace tl3d
