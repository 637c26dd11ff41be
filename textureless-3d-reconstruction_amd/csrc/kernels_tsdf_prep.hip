// kernels_tsdf_prep.hip -- row a11, the PREP CHAIN of the TSDF integration: what runs in front of the update kernel
// (kernels_tsdf.hip) and decides which bricks and sub-bricks of which frames it visits.  The structures both share are in
// tsdf_batch.h.
//
// tl3d_integrate collects frames into BATCHES of up to 32 (TL3D_TSDF_MAXBATCH).  The per-frame arguments (pose, depth image,
// tile and scratch pointers) of all its frames sit in one descriptor array in device memory and blockIdx.y / a bit index picks
// the frame.  Kernels 1 and 2 depend on the depth image, the scale and the depth limits only: their output is kept with the
// frame's slot and they run only over the frames of the batch whose slot has none for these parameters (no launch if none):
//   1. depth_tiles_kernel     (min, max, all-valid) of the valid scaled depth over 8x8-, 16x16- and 32x32-pixel tiles
//                             (pyramid levels 0-2) of a stale frame, 4 B/pixel read; the 8x8 level once more as 8-B records
//                             for the update kernel's per-voxel test
//   2. tile_pyramid_kernel    1 workgroup per stale frame: 2x2 reductions of level 2 up to a single tile; one valid pixel of the frame
//  2b. batch_begin_kernel     1 workgroup per frame, every batch: the batch's resets (list cursors, ticket counters, histogram
//                             bins), the frame's list of cells in view (pose-dependent), its valid pixel from the slot
//   3. brick_cull_kernel      per frame, one lane per 8^3 brick (one wave per 4x4x4-brick cell) classifies it from <= 16
//                             pyramid lookups:
//        SKIP   outside the view, no valid depth under it, or more than trunc behind every surface it can see
//        FREE   wholly inside the image, every pixel under it valid, and at least trunc in front of every
//               surface: every voxel gets exactly tsdf = 1 (q = 32767): ONE add to the brick's free-space counter
//        MIXED  everything else (near a surface, on the image border, straddling the camera plane): the frame's compact
//               list, its bit in the brick's frame mask, and -- if it is the first frame of the batch to list the brick --
//               the batch's brick list
//   4. subbrick_classify_kernel  per frame, one wave per listed brick: its eight 4x4x4 SUB-BRICKS by the same three rules
//        (8 lanes per sub-brick: one extreme voxel centre each, <= 8 pyramid lookups) -> a (mixed, free) bit mask.  On the
//        headline sequence 3.4 of the 8 sub-bricks of a listed brick stay MIXED.
//        Kernels 3 and 4 depend on the pose, the scale, the depth limits, the slot's tiles and the grid's geometry only: their
//        result is kept with the slot as well (the classification cache, below) and a frame that meets its slot with the same
//        key again is REPLAYED from it by class_replay_kernel, which runs in front of kernel 3; kernels 3 and 4 return at once
//        for such a frame.  The first fusion chain that replays an entry also REFINES its masks (class_refine_kernel, kernels_tsdf.hip): the
//        sub-bricks the update's own per-voxel tile test decides for all 64 voxels leave the MIXED masks for good.
//  4b. batch_hist_kernel, batch_order_kernel  the batch list ordered by cost, dearest bricks first: what the update walks
//   5. tsdf_update_pairs_kernel  the update itself, ONE launch per batch (kernels_tsdf.hip)
// Every classification is conservative with respect to the per-voxel rule (kernels_tsdf.hip: pair_project), so the result is the
// oracle's bit for bit whatever the view.
#include "tl3d_internal.h"
#include "bp_device.h"
#include "tsdf_batch.h"

namespace tl3d {

// The descriptors travel to the device as the ARGUMENTS of a tiny kernel (captured at launch: no staging buffer whose lifetime
// the host would have to track), 16 per launch (kernel arguments are limited to 4 KB).
struct DescChunk { FrameDesc d[16]; };
__global__ __launch_bounds__(256) void desc_upload_kernel(DescChunk c, FrameDesc *__restrict__ dst, int n) {
    const unsigned *src = reinterpret_cast<const unsigned *>(&c);
    unsigned *out = reinterpret_cast<unsigned *>(dst);
    const int words = n * (int)(sizeof(FrameDesc) / 4);
    for (int i = threadIdx.x; i < words; i += 256) out[i] = src[i];
}

// tile = (dmin, dmax, allvalid ? 1 : 0, unused)

// Depth source of the TSDF kernels: the f32 frame, or the 16-bit millimetre image it was converted from (uploads of kind
// TL3D_DEPTH_U16_MM keep it): same value through the same conversion as u16_to_f32_kernel (mm_to_m), half the bytes per pixel and
// so half the cache lines under a brick's footprint.
__device__ __forceinline__ float ld_depth(const float *__restrict__ p, size_t i) { return p[i]; }
__device__ __forceinline__ float ld_depth(const uint16_t *__restrict__ p, size_t i) { return mm_to_m(p[i]); }
__device__ __forceinline__ void ld_depth4(const float *__restrict__ p, size_t i, float dd[4]) {
    const float4 t4 = *reinterpret_cast<const float4 *>(p + i);
    dd[0] = t4.x; dd[1] = t4.y; dd[2] = t4.z; dd[3] = t4.w;
}
__device__ __forceinline__ void ld_depth4(const uint16_t *__restrict__ p, size_t i, float dd[4]) {
    const ushort4 t4 = *reinterpret_cast<const ushort4 *>(p + i);
    dd[0] = mm_to_m(t4.x); dd[1] = mm_to_m(t4.y); dd[2] = mm_to_m(t4.z); dd[3] = mm_to_m(t4.w);
}

// ---- 1. depth tiles --------------------------------------------------------------------------------------
// One 32x32-pixel region per WAVE.  Lane (q4 = lane & 7, rq = lane >> 3) holds the 4x4-pixel block at columns 4 q4 .. 4 q4 + 3, rows
// 4 rq .. 4 rq + 3: load i of a lane is row 4 rq + i, so every load instruction of the wave covers eight whole 128-byte row
// segments, and the lane's four 16-B loads are issued before the first is looked at.  The block is reduced inside the lane; an 8x8
// tile is 2 x 2 lanes (lane bits 0 and 3), a 16x16 tile 4 x 4 (+ bits 1 and 4), the region all of them (+ bits 2 and 5): SIX
// butterfly steps for the three levels.  (Round 3 gave a lane four rows 8 apart: every row of 8x8 tiles was a 16-lane
// reduction of its own, 19 steps; the kernel's 33 M vector instructions per 32 frames were a sixth of the batch's -- and the batch is
// bound by exactly those)  min / max over the VALID pixels: an invalid one enters as NaN, which v_min_f32 / v_max_f32
// pass over.  No LDS, no workgroup barrier.
// The tiles, the pyramid and the valid pixel are functions of the depth image, the scale and the depth limits alone: they live with
// the frame's SLOT (Slot::tiles, tl3d_internal.h) and are built only for the frames of a batch whose slot holds none for these
// parameters -- the STALE frames, by their index in the batch (blockIdx.y picks an entry of the list).
struct StaleList { unsigned char idx[TL3D_TSDF_MAXBATCH]; };
template <typename DT>
__global__ __launch_bounds__(256) void depth_tiles_kernel(Cam cam, BatchBufs B, Pyramid py, int nrx, int nry, StaleList stale) {
    const DescPtr F = const_descs(B) + stale.idx[blockIdx.y];
    const TsdfConst c = desc_const(F);
    const DT *__restrict__ depth = static_cast<const DT *>(F->depth);
    float4 *__restrict__ tiles = F->tiles;
    float2 *__restrict__ vtile = F->vtile;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int q4 = lane & 7, rq = lane >> 3;
    const bool vec = (cam.W & 3) == 0;                              // rows are 16-B aligned
    const float qnan = __uint_as_float(0x7fc00000u);
    for (int region = blockIdx.x * 4 + wid; region < nrx * nry; region += gridDim.x * 4) {
        const int rx = region % nrx, ry = region / nrx;
        const int u0 = rx * REGION + q4 * 4, v0 = ry * REGION + rq * 4;
        // the lane's block: lowest / highest VALID scaled depth, and whether a pixel of it (inside the image) is not valid
        float mn = qnan, mx = qnan;
        bool bad = false;
        if (vec && (rx + 1) * REGION <= cam.W && (ry + 1) * REGION <= cam.H) {
            // (wave-uniform) the region lies wholly inside the image -- all but the last region column and row: no per-pixel
            // in-image tests, one 64-bit row address per lane
            const DT *__restrict__ p = depth + ((size_t)v0 * (unsigned)cam.W + (unsigned)u0);
            float dd[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) ld_depth4(p, (size_t)i * (unsigned)cam.W, dd[i]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float t[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = dd[i][k] * c.sc;
                    const bool ok = d > c.mind && d < c.maxd;
                    t[k] = ok ? d : qnan;
                    bad = bad || !ok;
                }
                mn = fminf(fminf(mn, t[0]), fminf(t[1], fminf(t[2], t[3])));    // (NaN operands are passed over)
                mx = fmaxf(fmaxf(mx, t[0]), fmaxf(t[1], fmaxf(t[2], t[3])));
            }
        } else {
            const int nv = min(4, cam.W - u0);
            float dd[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dd[i][0] = dd[i][1] = dd[i][2] = dd[i][3] = 0.0f;
                if (v0 + i < cam.H && u0 < cam.W) {
                    if (vec) {
                        ld_depth4(depth, (size_t)(v0 + i) * cam.W + u0, dd[i]);
                    } else {
                        for (int k = 0; k < 4; ++k) dd[i][k] = (k < nv) ? ld_depth(depth, (size_t)(v0 + i) * cam.W + u0 + k) : 0.0f;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float t[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = dd[i][k] * c.sc;
                    const bool in_img = (v0 + i < cam.H) && (k < nv) && (u0 < cam.W);
                    const bool ok = d > c.mind && d < c.maxd;
                    t[k] = (ok && in_img) ? d : qnan;
                    bad = bad || (in_img && !ok);
                }
                mn = fminf(fminf(mn, t[0]), fminf(t[1], fminf(t[2], t[3])));    // (NaN operands are passed over)
                mx = fmaxf(fmaxf(mx, t[0]), fmaxf(t[1], fmaxf(t[2], t[3])));
            }
        }
        // from here on: +inf / -inf for "no valid pixel" (the format of the pyramid), the flag as a number
        mn = (mn == mn) ? mn : INFINITY;
        mx = (mx == mx) ? mx : -INFINITY;
        int bd = bad ? 1 : 0;
        auto combine = [&](int d) {
            mn = fminf(mn, __shfl_xor(mn, d));
            mx = fmaxf(mx, __shfl_xor(mx, d));
            bd |= __shfl_xor(bd, d);
        };
        combine(1); combine(8);                                     // level 0: 8x8 pixels
        if ((lane & 9) == 0) {
            const int tx = rx * 4 + (q4 >> 1), ty = ry * 4 + (rq >> 1);
            if (tx < py.ntx[0] && ty < py.nty[0]) {
                tiles[py.off[0] + ty * py.ntx[0] + tx] = make_float4(mn, mx, bd ? 0.0f : 1.0f, 0.0f);
                // (lowest depth if EVERY pixel is valid, else -inf: "never surely free"; highest valid depth, -inf if none: "skip")
                vtile[ty * py.ntx[0] + tx] = make_float2(bd ? -INFINITY : mn, mx);
            }
        }
        combine(2); combine(16);                                    // level 1: 16x16
        if ((lane & 27) == 0 && py.nlev > 1) {
            const int tx = rx * 2 + (q4 >> 2), ty = ry * 2 + (rq >> 2);
            if (tx < py.ntx[1] && ty < py.nty[1]) tiles[py.off[1] + ty * py.ntx[1] + tx] = make_float4(mn, mx, bd ? 0.0f : 1.0f, 0.0f);
        }
        combine(4); combine(32);                                    // level 2: the region
        if (lane == 0 && py.nlev > 2) tiles[py.off[2] + ry * py.ntx[2] + rx] = make_float4(mn, mx, bd ? 0.0f : 1.0f, 0.0f);
    }
}

__device__ __forceinline__ bool sphere_in_view(const Frustum &fr, float x, float y, float z, float rad) {
    return (z + rad > 0.0f) && (fr.lx * x + fr.lz * z >= -rad) && (fr.rx * x + fr.rz * z >= -rad) &&
           (fr.ty * y + fr.tz * z >= -rad) && (fr.by * y + fr.bz * z >= -rad);
}

// The valid pixel is kept in the first word of the float4 behind the pyramid's last level (the slot's buffer has that one more).
__device__ __forceinline__ int pyramid_total(const Pyramid &py) { return py.off[py.nlev - 1] + py.ntx[py.nlev - 1] * py.nty[py.nlev - 1]; }

// ---- 2b. what every batch does for every frame, cached tiles or not: 1 workgroup per frame --------------------------------------
// The RESETS of the batch (the frame's list cursors; in workgroup 0 the batch list's length, the update's ticket counters and the
// ordering pass's bins): ahead of the brick classification in stream order, whether or not a tile build ran.  The frame's CELL
// LIST: the 4x4x4-brick cells whose bounding sphere meets the view (one in five on the headline orbit), so that the brick
// classification starts waves only for those -- it depends on the pose.  And the slot's valid pixel, copied to where the update
// kernel reads it.
__global__ __launch_bounds__(256) void batch_begin_kernel(Grid g, Frustum fr, Pyramid py, BatchBufs B) {
    __shared__ unsigned s_ncell;
    const DescPtr F = const_descs(B) + blockIdx.x;
    if (threadIdx.x < 2) F->counts[threadIdx.x] = 0u;                            // reset the frame's list cursors
    if (threadIdx.x >= REFINE_COUNTS && threadIdx.x < REFINE_COUNTS + 4) F->counts[threadIdx.x] = 0u;      // and its refinement counts
    if (blockIdx.x == 0) {                                                       // and the batch list's, the update's ticket counters, the ordering pass's bins
        if (threadIdx.x == 2) B.hdr[0] = 0u;
        if (threadIdx.x >= 64 && threadIdx.x < 64 + TICKET_GROUPS) B.hdr[HDR_TICKETS + 16u * (threadIdx.x - 64)] = 0u;
        if (threadIdx.x >= 128) B.hdr[HDR_HIST + (threadIdx.x - 128)] = 0u;
    }
    if (threadIdx.x == 0) s_ncell = 0u;
    __syncthreads();
    {
        const PoseF pose = desc_pose(F);
        unsigned *__restrict__ cells = F->cells;
        const int ncx = (g.nbx + 3) >> 2, ncy = (g.nby + 3) >> 2, ncz = (g.nbz + 3) >> 2;
        const float crad = 27.712812f * g.vs * 1.01f;               // half diagonal of a 32^3-voxel cell, +1 % (the cull kernel's own test)
        for (int c0 = 0; c0 < ncx * ncy * ncz; c0 += 256) {
            const int cell = c0 + (int)threadIdx.x;
            bool in = false;
            if (cell < ncx * ncy * ncz) {
                const int ccx = cell % ncx, ccy = (cell / ncx) % ncy, ccz = cell / (ncx * ncy);
                const float qx = fmaf((float)(g.vox + ccx * 32 + 16), g.vs, g.ox), qy = fmaf((float)(g.voy + ccy * 32 + 16), g.vs, g.oy);
                const float qz = fmaf((float)(g.voz + ccz * 32 + 16), g.vs, g.oz);
                const float ex = pose.r[0] * qx + pose.r[1] * qy + pose.r[2] * qz + pose.t[0];
                const float ey = pose.r[3] * qx + pose.r[4] * qy + pose.r[5] * qz + pose.t[1];
                const float ez = pose.r[6] * qx + pose.r[7] * qy + pose.r[8] * qz + pose.t[2];
                in = sphere_in_view(fr, ex, ey, ez, crad);
            }
            const unsigned long long m = __ballot(in);
            unsigned base = 0;
            if ((threadIdx.x & 63) == 0 && m) base = atomicAdd(&s_ncell, (unsigned)__popcll(m));
            base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
            if (in) cells[base + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull))] = (unsigned)cell;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            F->counts[CELL_COUNT] = s_ncell;
            const unsigned vp = *reinterpret_cast<const unsigned *>(F->tiles + pyramid_total(py));
            F->counts[VALID_PIXEL] = vp;
            const_cast<FrameDesc *>(B.frames)[blockIdx.x].valid_pix = vp;      // (the update kernel of this batch reads it as a scalar)
        }
    }
}

// ---- 2. pyramid: levels 3 .. from level 2; 1 workgroup per STALE frame ----------------------------------------------------------
// Also finds ONE PIXEL OF THE FRAME THAT IS VALID (the top-left pixel of an all-valid tile): where the update kernel sends the
// lanes whose depth value cannot matter (below).
__global__ __launch_bounds__(256) void tile_pyramid_kernel(Cam cam, Pyramid py, BatchBufs B, StaleList stale) {
    float4 *__restrict__ tiles = const_descs(B)[stale.idx[blockIdx.x]].tiles;
    __shared__ unsigned s_found;
    if (threadIdx.x == 0) s_found = 0xffffffffu;
    __syncthreads();
    for (int L = min(2, py.nlev - 1); L >= 0; L -= 2) {           // 32-pixel tiles first; only a frame full of holes needs the 8-pixel ones
        const int n = py.ntx[L] * py.nty[L];
        for (int i = threadIdx.x; i < n; i += 256)
            if (tiles[py.off[L] + i].z > 0.5f) {
                const unsigned x = (unsigned)(i % py.ntx[L]) << (TILE0_SHIFT + L), y = (unsigned)(i / py.ntx[L]) << (TILE0_SHIFT + L);
                atomicMin(&s_found, y * (unsigned)cam.W + x);
                break;
            }
        __syncthreads();
        if (s_found != 0xffffffffu) break;                        // (uniform: read after the barrier)
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned vp = s_found == 0xffffffffu ? 0u : s_found;
        *reinterpret_cast<unsigned *>(tiles + pyramid_total(py)) = vp;     // with the slot: batch_begin_kernel hands it to each batch
    }
    for (int L = 3; L < py.nlev; ++L) {
        const int n = py.ntx[L] * py.nty[L];
        const float4 *__restrict__ src = tiles + py.off[L - 1];
        float4 *__restrict__ dst = tiles + py.off[L];
        for (int i = threadIdx.x; i < n; i += 256) {
            const int x = i % py.ntx[L], y = i / py.ntx[L];
            float4 r = make_float4(INFINITY, -INFINITY, 1.0f, 0.0f);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int sx = 2 * x + dx, sy = 2 * y + dy;
                    if (sx < py.ntx[L - 1] && sy < py.nty[L - 1]) {
                        const float4 s = src[sy * py.ntx[L - 1] + sx];
                        r.x = fminf(r.x, s.x);
                        r.y = fmaxf(r.y, s.y);
                        r.z = fminf(r.z, s.z);
                    }
                }
            dst[i] = r;
        }
        __syncthreads();        // level L complete (and visible to the block) before level L+1 reads it
    }
}

// ---- 3. brick classification ------------------------------------------------------------------------------
// One wave per LISTED cell of 4x4x4 bricks (the frame's cell list: cells whose bounding sphere meets the view), one lane per brick; the four waves of a workgroup pool their survivors so the list
// cursors see one atomic per workgroup, not per wave (same-address returning atomics retire at ~90 per microsecond).
// Margins: 1.5 px on projected bounds, 1 % of a voxel on depths, 0.1 % on the truncation distance.
// The three rules on one box of voxels, given what the pyramid says about the pixels under it: a = (min, max, all-valid) of
// the valid scaled depth over a superset of the box's pixel footprint, [zmin, zmax] the camera depths of its voxel centres,
// inside = the footprint (widened by 1.5 px) lies wholly in the image.  0 skip, 1 mixed, 2 free.
__device__ __forceinline__ int classify_box(const Grid &g, float4 a, float zmin, float zmax, bool inside) {
    const float m = 0.01f * g.vs;
    if (!(a.y > -INFINITY) || (zmin - m > a.y + g.trunc)) return 0;      // no valid depth under the box, or > trunc behind all it can see
    if (inside && a.z > 0.5f && (a.x - (zmax + m) >= g.trunc * 1.001f)) return 2;   // every voxel: in image, valid depth, sdf >= trunc => tsdf == 1 exactly
    return 1;
}

// ---- the classification cache ------------------------------------------------------------------------------------------
// What the cull and the sub-brick classification find for a frame depends on its pose, scale and depth limits, the camera, the
// slot's tiles and the grid's geometry -- not on the grid's records, nor on any earlier batch.  A slot keeps the result of the
// last classification made for it (Slot::cls; the host holds the key, api_fuse.hip: class_cache_lookup) and a batch that meets
// the slot again with the same key REPLAYS it: class_replay_kernel walks the cached lists through the very tail the cull ends
// with.  Buffer: [header: CC_HDR_WORDS] [entries: cap words, the MIXED bricks from the front as F->list gets them, the FREE
// bricks from the back] [cap 16-bit sub-brick masks, one per MIXED entry, as F->sub[brick] holds them].  Only the device knows
// how many bricks a frame lists: class_finish_kernel marks the header complete only if MIXED + FREE <= cap, a frame that did
// not fit is classified every time, and each kernel takes its path for a frame from the mode and that header alone (uniform
// over the frame's workgroups; no host wait).  Level 1 = lists and counts, level 2 = + masks: a classify-only chain
// (tl3d_count_bricks) fills level 1, and the fusion that follows replays it, runs the sub-brick classification over the
// cached list and leaves level 2.  Level 3 = masks refined by class_refine_kernel (kernels_tsdf.hip, beside the
// update kernel whose tile test it shares); it serves every chain as level 2 does.  Whether frame f of a plan is replayed:
// class_replays(P, f), tsdf_batch.h.

// The TAIL of a brick's classification for frame `frame`, shared by the cull and the replay: one lane per (brick, class), the
// whole workgroup calls it.  MIXED (cls 1): the brick's bit in the frame mask; the first frame of the batch to set a bit takes
// the brick's pool slot and puts it on the batch list; the frame's own list.  FREE (cls 2): one add to the brick's free-space
// counter.  The four waves pool their survivors so that the list cursors see one atomic per workgroup, not per wave.
// save: the frame's cache buffer if this classification is to be recorded, else null.
struct ClassTailLds { unsigned cnt[4][3], base[3]; };
__device__ __forceinline__ void class_tail(const Grid &g, const BatchBufs &B, DescPtr F, unsigned *__restrict__ free_cnt, unsigned frame, int cls, unsigned brick,
                                           unsigned *__restrict__ save, unsigned cap, ClassTailLds &S) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned *__restrict__ list = F->list;
    // MIXED: the brick's bit in the frame mask; the first frame of the batch to set a bit also puts the brick on the batch list
    bool first = false;
    if (cls == 1) {
        first = atomicOr(B.framemask + brick, 1u << frame) == 0u;
        if (first) (void)brick_slot_ensure(g.tsdf_tab, g.cursors, g.tsdf_cap, brick);     // sparse grid: records on first touch
    }
    // Free space: every voxel of the brick gets exactly (+32767, +1).  That is ONE integer add here instead of a 4 KB read +
    // 4 KB write by the update kernel; the counters are folded into the records before anything reads them (fold_free_kernel).
    if (cls == 2) atomicAdd(free_cnt + brick, 1u);
    const unsigned long long mm = __ballot(cls == 1), mf = __ballot(cls == 2), m1 = __ballot(first);
    if (lane == 0) { S.cnt[wid][0] = (unsigned)__popcll(mm); S.cnt[wid][1] = (unsigned)__popcll(mf); S.cnt[wid][2] = (unsigned)__popcll(m1); }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned tot = S.cnt[0][threadIdx.x] + S.cnt[1][threadIdx.x] + S.cnt[2][threadIdx.x] + S.cnt[3][threadIdx.x];
        unsigned *cur = threadIdx.x < 2 ? F->counts + threadIdx.x : B.hdr;      // [1]: free-space bricks, counted (listed only in the cache)
        S.base[threadIdx.x] = tot ? atomicAdd(cur, tot) : 0u;
    }
    __syncthreads();
    unsigned bm = S.base[0], b1 = S.base[2];
    for (int w = 0; w < wid; ++w) { bm += S.cnt[w][0]; b1 += S.cnt[w][2]; }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (cls == 1) list[bm + __popcll(mm & below)] = brick;
    if (first) B.list[b1 + __popcll(m1 & below)] = brick;
    if (save) {                                                    // (uniform) the same entry, and the FREE bricks, into the slot's buffer
        unsigned bf = S.base[1];
        for (int w = 0; w < wid; ++w) bf += S.cnt[w][1];
        const unsigned pm = bm + (unsigned)__popcll(mm & below), pf = bf + (unsigned)__popcll(mf & below);
        if (cls == 1 && pm < cap) save[CC_HDR_WORDS + pm] = brick;
        if (cls == 2 && pf < cap) save[CC_HDR_WORDS + (cap - 1u - pf)] = brick;
    }
    __syncthreads();                                               // S is reused by the next trip
}

// CACHE = false: for chains none of whose frames uses the cache (ClassPlan::modes == 0: the cache is off) -- the kernel as it was
// before the cache existed, without the plan among its arguments (brick_cull_kernel; brick_cull_cached_kernel is the other).
template <bool CACHE>
__device__ __forceinline__ void brick_cull(const Cam &cam, const Grid &g, const BatchBufs &B, const Frustum &fr, const Pyramid &py,
                                           unsigned *__restrict__ free_cnt, const ClassPlan &P) {
    unsigned *__restrict__ save = nullptr;
    if (CACHE) {
        if (class_replays(P, blockIdx.y)) return;                   // (class_replay_kernel has listed this frame's bricks)
        const unsigned mode = class_mode(P, blockIdx.y);
        if (mode == CC_SAVE) save = P.cache[blockIdx.y];
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            atomicAdd(P.stats + 0, 1ull);
            if (mode == CC_REPLAY) atomicAdd(P.stats + 2, 1ull);    // its entry did not fit: classified every time
        }
    }
    const DescPtr F = const_descs(B) + blockIdx.y;
    const PoseF pose = desc_pose(F);
    const float4 *__restrict__ tiles = F->tiles;
    __shared__ ClassTailLds S;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int ncx = (g.nbx + 3) >> 2, ncy = (g.nby + 3) >> 2, ncz = (g.nbz + 3) >> 2;
    // the frame's cell list (tile_pyramid_kernel): four cells per workgroup and trip
    const unsigned ncell = min(F->counts[CELL_COUNT], (unsigned)(ncx * ncy * ncz));
    const unsigned *__restrict__ cells = F->cells;
    for (unsigned quad = blockIdx.x; quad * 4u < ncell; quad += gridDim.x) {
    const unsigned li = quad * 4u + (unsigned)wid;
    const int cell = li < ncell ? (int)min(cells[li], (unsigned)(ncx * ncy * ncz - 1)) : -1;
    int cls = 0;                                                  // 0 skip, 1 mixed, 2 free
    int brick = 0;
    if (cell >= 0) {
        const int ccx = cell % ncx, ccy = (cell / ncx) % ncy, ccz = cell / (ncx * ncy);
        const int bx = ccx * 4 + (lane & 3), by = ccy * 4 + ((lane >> 2) & 3), bz = ccz * 4 + (lane >> 4);
        const bool in_grid = bx < g.nbx && by < g.nby && bz < g.nbz;
        brick = (bz * g.nby + by) * g.nbx + bx;
        const float crad = 27.712812f * g.vs * 1.01f;               // half diagonal of a 32^3-voxel cell, +1 %
        const float qx = fmaf((float)(g.vox + ccx * 32 + 16), g.vs, g.ox), qy = fmaf((float)(g.voy + ccy * 32 + 16), g.vs, g.oy);
        const float qz = fmaf((float)(g.voz + ccz * 32 + 16), g.vs, g.oz);
        const float ex = pose.r[0] * qx + pose.r[1] * qy + pose.r[2] * qz + pose.t[0];
        const float ey = pose.r[3] * qx + pose.r[4] * qy + pose.r[5] * qz + pose.t[1];
        const float ez = pose.r[6] * qx + pose.r[7] * qy + pose.r[8] * qz + pose.t[2];
        if (sphere_in_view(fr, ex, ey, ez, crad) && in_grid) {
            const float rad = 6.9282032f * g.vs * 1.01f;             // half diagonal of a brick, +1 %
            const float wx = fmaf((float)(g.vox + bx * 8 + 4), g.vs, g.ox);
            const float wy = fmaf((float)(g.voy + by * 8 + 4), g.vs, g.oy);
            const float wz = fmaf((float)(g.voz + bz * 8 + 4), g.vs, g.oz);
            const float cxm = pose.r[0] * wx + pose.r[1] * wy + pose.r[2] * wz + pose.t[0];
            const float cym = pose.r[3] * wx + pose.r[4] * wy + pose.r[5] * wz + pose.t[1];
            const float czm = pose.r[6] * wx + pose.r[7] * wy + pose.r[8] * wz + pose.t[2];
            if (sphere_in_view(fr, cxm, cym, czm, rad)) {
                cls = 1;
                if (czm - rad > 1e-3f) {
                    // all 8 corners are in front of the camera: the voxel centres project inside the corners' pixel box
                    const float h = 4.0f * g.vs;
                    float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY, zmin = INFINITY, zmax = -INFINITY;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float sx = (k & 1) ? h : -h, sy = (k & 2) ? h : -h, sz = (k & 4) ? h : -h;
                        const float x = cxm + pose.r[0] * sx + pose.r[1] * sy + pose.r[2] * sz;
                        const float y = cym + pose.r[3] * sx + pose.r[4] * sy + pose.r[5] * sz;
                        const float z = czm + pose.r[6] * sx + pose.r[7] * sy + pose.r[8] * sz;
                        const float iz = __builtin_amdgcn_rcpf(z);     // 1 ulp; the 1.5 px margin absorbs it
                        const float u = cam.fx * x * iz + cam.cx, v = cam.fy * y * iz + cam.cy;
                        umin = fminf(umin, u); umax = fmaxf(umax, u);
                        vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
                        zmin = fminf(zmin, z); zmax = fmaxf(zmax, z);
                    }
                    umin -= 1.5f; umax += 1.5f; vmin -= 1.5f; vmax += 1.5f;
                    if (umax < 0.0f || vmax < 0.0f || umin > (float)(cam.W - 1) || vmin > (float)(cam.H - 1)) {
                        cls = 0;
                    } else {
                        const bool inside = umin >= 0.0f && vmin >= 0.0f && umax <= (float)(cam.W - 1) && vmax <= (float)(cam.H - 1);
                        const int pu0 = max(0, (int)floorf(umin)), pu1 = min(cam.W - 1, (int)ceilf(umax));
                        const int pv0 = max(0, (int)floorf(vmin)), pv1 = min(cam.H - 1, (int)ceilf(vmax));
                        // finest level at which the pixel box spans at most 4 tiles per axis: 16 independent lookups
                        int L = 0;
                        while (L < py.nlev - 1 && (((pu1 >> (TILE0_SHIFT + L)) - (pu0 >> (TILE0_SHIFT + L))) > 3 ||
                                                   ((pv1 >> (TILE0_SHIFT + L)) - (pv0 >> (TILE0_SHIFT + L))) > 3))
                            ++L;
                        const int tu0 = pu0 >> (TILE0_SHIFT + L), tu1 = pu1 >> (TILE0_SHIFT + L);
                        const int tv0 = pv0 >> (TILE0_SHIFT + L), tv1 = pv1 >> (TILE0_SHIFT + L);
                        const float4 *__restrict__ lv = tiles + py.off[L];
                        const int nt = py.ntx[L];
                        float4 a = make_float4(INFINITY, -INFINITY, 1.0f, 0.0f);
#pragma unroll
                        for (int dv = 0; dv < 4; ++dv)
#pragma unroll
                            for (int du = 0; du < 4; ++du) {
                                const float4 b = lv[min(tv0 + dv, tv1) * nt + min(tu0 + du, tu1)];   // clamped: repeats are harmless
                                a.x = fminf(a.x, b.x);
                                a.y = fmaxf(a.y, b.y);
                                a.z = fminf(a.z, b.z);
                            }
                        cls = classify_box(g, a, zmin, zmax, inside);
                        // (A SPARSE grid classifies exactly as a dense one.  Until round 3 a brick that every VALID pixel under it
                        // put in free space, but whose footprint had holes or left the image, was skipped there -- "records for free
                        // space only" -- and the voxels of such a brick that came within the band in another frame lost those
                        // observations.  Such bricks take a pool slot now and the sparse grid is the oracle's grid bit for bit.)
                    }
                }
            }
        }
    }
    class_tail(g, B, F, free_cnt, blockIdx.y, cls, (unsigned)brick, save, CACHE ? P.cap : 0u, S);
    }
}
__global__ __launch_bounds__(256) void brick_cull_kernel(Cam cam, Grid g, BatchBufs B, Frustum fr, Pyramid py, unsigned *__restrict__ free_cnt) {
    brick_cull<false>(cam, g, B, fr, py, free_cnt, ClassPlan());
}

// records += count x (32767, 1) for every brick with a pending free-space count; the count returns to zero (exchanged, so a
// count that lands between the read and the reset cannot be lost).  One wave per brick, 16 B per lane.  Runs on the main
// stream before anything reads the TSDF channel (download, merge, extraction, weight check), i.e. once per scan, not per frame.
// A brick WITHOUT records (sparse grid: free space nobody ever saw a surface in) keeps its count: readers add it (tsdf_record).
__global__ __launch_bounds__(256) void fold_free_kernel(Grid g, int2 *__restrict__ grid, unsigned *__restrict__ free_cnt, unsigned nbricks) {
    const int lane = threadIdx.x & 63;
    for (unsigned b = blockIdx.x * 4u + (threadIdx.x >> 6); b < nbricks; b += gridDim.x * 4u) {
        if (__builtin_amdgcn_readfirstlane(free_cnt[b]) == 0u) continue;
        const unsigned slot = (unsigned)__builtin_amdgcn_readfirstlane((int)brick_slot(g.tsdf_tab, b));
        if (slot >= SLOT_FULL) continue;
        unsigned c = 0;
        if (lane == 0) c = atomicExch(free_cnt + b, 0u);
        c = __builtin_amdgcn_readfirstlane(c);
        if (c == 0u) continue;
        int4 *__restrict__ recs = reinterpret_cast<int4 *>(grid + ((size_t)slot << 9));
        const int dq = (int)(c * 32767u), dw = (int)c;
        int4 r0 = recs[lane], r1 = recs[64 + lane], r2 = recs[128 + lane], r3 = recs[192 + lane];
        r0.x += dq; r0.y += dw; r0.z += dq; r0.w += dw;
        r1.x += dq; r1.y += dw; r1.z += dq; r1.w += dw;
        r2.x += dq; r2.y += dw; r2.z += dq; r2.w += dw;
        r3.x += dq; r3.y += dw; r3.z += dq; r3.w += dw;
        recs[lane] = r0; recs[64 + lane] = r1; recs[128 + lane] = r2; recs[192 + lane] = r3;
    }
}

// ---- 4. sub-brick classification ------------------------------------------------------------------------------------------
// Class of ONE 4x4x4 sub-brick (the lane's): its 8 extreme voxel centres by the per-voxel position sequence (they span the box
// of all 64: a projective map keeps convexity while every depth is positive, so all 64 project inside the 8 projections' pixel
// box), then <= 8 pyramid tiles that cover the box (finest level at which it spans <= 8 tiles).  0 skip, 1 mixed, 2 free.
__device__ __forceinline__ int classify_subbrick(const Cam &cam, const Grid &g, const Pyramid &py, const PoseF &pose,
                                                 const float4 *__restrict__ tiles, int i0, int j0, int k0) {
    float wx[2], wy[2], wz[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        wx[h] = fmaf((float)(g.vox + i0 + 3 * h) + 0.5f, g.vs, g.ox);
        wy[h] = fmaf((float)(g.voy + j0 + 3 * h) + 0.5f, g.vs, g.oy);
        wz[h] = fmaf((float)(g.voz + k0 + 3 * h) + 0.5f, g.vs, g.oz);
    }
    float x[8], y[8], z[8];
    float zmin = INFINITY, zmax = -INFINITY;
#pragma unroll
    for (int hz = 0; hz < 2; ++hz) {
        const float ax0 = fmaf(pose.r[2], wz[hz], pose.t[0]), ay0 = fmaf(pose.r[5], wz[hz], pose.t[1]), az0 = fmaf(pose.r[8], wz[hz], pose.t[2]);
#pragma unroll
        for (int hy = 0; hy < 2; ++hy) {
            const float ax = fmaf(pose.r[1], wy[hy], ax0), ay = fmaf(pose.r[4], wy[hy], ay0), az = fmaf(pose.r[7], wy[hy], az0);
#pragma unroll
            for (int hx = 0; hx < 2; ++hx) {
                const int c = hz * 4 + hy * 2 + hx;
                x[c] = fmaf(pose.r[0], wx[hx], ax);
                y[c] = fmaf(pose.r[3], wx[hx], ay);
                z[c] = fmaf(pose.r[6], wx[hx], az);
                zmin = fminf(zmin, z[c]);
                zmax = fmaxf(zmax, z[c]);
            }
        }
    }
    if (!(zmin > 1e-3f)) return 1;                                  // touches the camera plane: per-voxel rule decides
    float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float iz = __builtin_amdgcn_rcpf(z[c]);                // 1 ulp; the 1.5 px margin absorbs it
        const float u = cam.fx * x[c] * iz + cam.cx, v = cam.fy * y[c] * iz + cam.cy;
        umin = fminf(umin, u); umax = fmaxf(umax, u);
        vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
    }
    umin -= 1.5f; umax += 1.5f; vmin -= 1.5f; vmax += 1.5f;
    if (umax < 0.0f || vmax < 0.0f || umin > (float)(cam.W - 1) || vmin > (float)(cam.H - 1)) return 0;
    const bool inside = umin >= 0.0f && vmin >= 0.0f && umax <= (float)(cam.W - 1) && vmax <= (float)(cam.H - 1);
    const int pu0 = max(0, (int)floorf(umin)), pu1 = min(cam.W - 1, (int)ceilf(umax));
    const int pv0 = max(0, (int)floorf(vmin)), pv1 = min(cam.H - 1, (int)ceilf(vmax));
    // finest level at which the box spans at most 8 tiles; level geometry by arithmetic (no table lookups per lane)
    int L = 0, off = 0, ntx = py.ntx[0], nty = py.nty[0];
    int tu0, tv0, nu, nv;
    for (;;) {
        tu0 = pu0 >> (TILE0_SHIFT + L); tv0 = pv0 >> (TILE0_SHIFT + L);
        nu = (pu1 >> (TILE0_SHIFT + L)) - tu0 + 1; nv = (pv1 >> (TILE0_SHIFT + L)) - tv0 + 1;
        if (nu * nv <= 8 || L >= py.nlev - 1) break;
        off += ntx * nty;
        ntx = (ntx + 1) >> 1; nty = (nty + 1) >> 1;
        ++L;
    }
    const float4 *__restrict__ lv = tiles + off;
    float4 a = make_float4(INFINITY, -INFINITY, 1.0f, 0.0f);
    int du = 0, dv = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {                                   // tiles (du, dv) row by row; beyond the box: the last one again (harmless)
        const float4 b = lv[(tv0 + dv) * ntx + (tu0 + du)];
        a.x = fminf(a.x, b.x);
        a.y = fmaxf(a.y, b.y);
        a.z = fminf(a.z, b.z);
        if (du + 1 < nu) ++du;
        else if (dv + 1 < nv) { du = 0; ++dv; }
    }
    return classify_box(g, a, zmin, zmax, inside);
}

// Prep kernel 4: sub-brick masks of the listed bricks of every frame; one lane per sub-brick, 8 bricks per wave.
// A frame that was replayed at level 2 has its masks already; one replayed at level 1 is classified over the CACHED list (the
// same bricks as F->list, in the order the masks are kept in); a frame that is being saved keeps a copy of each mask.
template <bool CACHE>
__device__ __forceinline__ void subbrick_classify(const Cam &cam, const Grid &g, const Pyramid &py, const BatchBufs &B, const ClassPlan &P) {
    const DescPtr F = const_descs(B) + blockIdx.y;
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned nbricks = (unsigned)(g.nbx * g.nby * g.nbz);
    unsigned n = min(F->counts[0], nbricks);
    const unsigned *__restrict__ list = F->list;
    unsigned short *__restrict__ csub = nullptr;                    // the masks' copy in the slot's buffer, by list index
    if (CACHE) {
        const bool replayed = class_replays(P, blockIdx.y);
        if (replayed) {
            if (P.cache[blockIdx.y][2] >= 2u) return;
            list = P.cache[blockIdx.y] + CC_HDR_WORDS;
            n = min(n, P.cap);
        }
        if (replayed || class_mode(P, blockIdx.y) == CC_SAVE) csub = reinterpret_cast<unsigned short *>(P.cache[blockIdx.y] + CC_HDR_WORDS + P.cap);
    }
    const PoseF pose = desc_pose(F);
    const float4 *__restrict__ tiles = F->tiles;
    unsigned short *__restrict__ sub = F->sub;
    const int j = lane >> 3, sb = lane & 7;
    for (unsigned base = (blockIdx.x * 4u + (unsigned)wid) * 8u; base < n; base += gridDim.x * 32u) {
        const unsigned t = base + (unsigned)j;
        int cls = 0;
        unsigned brick = 0;
        if (t < n) {
            brick = min(list[t], nbricks - 1u);
            const int bx = (int)(brick % (unsigned)g.nbx), by = (int)((brick / (unsigned)g.nbx) % (unsigned)g.nby), bz = (int)(brick / (unsigned)(g.nbx * g.nby));
            cls = classify_subbrick(cam, g, py, pose, tiles, bx * 8 + (sb & 1) * 4, by * 8 + ((sb >> 1) & 1) * 4, bz * 8 + (sb >> 2) * 4);
        }
        const unsigned long long mm = __ballot(cls == 1), mf = __ballot(cls == 2);
        if (sb == 0 && t < n) {
            const unsigned short m = (unsigned short)(((mm >> (8 * j)) & 0xffull) | (((mf >> (8 * j)) & 0xffull) << 8));
            sub[brick] = m;
            if (CACHE && csub && t < P.cap) csub[t] = m;
        }
    }
}
__global__ __launch_bounds__(256) void subbrick_classify_kernel(Cam cam, Grid g, Pyramid py, BatchBufs B) {
    subbrick_classify<false>(cam, g, py, B, ClassPlan());
}

// ---- 4b. the batch list, dearest bricks first -------------------------------------------------------------------------------
// A brick costs the update one pipeline step per (frame, MIXED sub-brick): 1 ... 256.  The list comes out of the classification
// in order of first listing, a wave takes ~5 bricks of it, and the launch lasts as long as its unluckiest wave: the longest wave
// ran 1.9 x the mean (stamps, experiments flavour), i.e. half of the chip idled through the second half of the launch.  Ordered
// by cost, dearest first, the tickets hand the cheap bricks out last and the waves end together.  Cost proxy: the number of frames
// that list the brick (1 ... 32, known from the frame mask); a counting sort in two small launches of the prep chain:
// histogram, then scatter (every workgroup reserves its range of each bin with one atomic per bin).
constexpr int ORDER_BLOCKS = 64;
__device__ __forceinline__ unsigned brick_cost_bin(const unsigned *__restrict__ framemask, unsigned brick) {
    const unsigned c = (unsigned)__popc(framemask[brick]);
    return c > 32u ? 32u : c;                                          // bin 0: nobody lists it any more (cannot happen; kept last)
}
__global__ __launch_bounds__(256) void batch_hist_kernel(Grid g, BatchBufs B) {
    __shared__ unsigned h[33];
    if (threadIdx.x < 33) h[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned nbricks = (unsigned)(g.nbx * g.nby * g.nbz);
    const unsigned n = min(B.hdr[0], nbricks);
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
        atomicAdd(&h[brick_cost_bin(B.framemask, min(B.list[i], nbricks - 1u))], 1u);
    __syncthreads();
    if (threadIdx.x < 33 && h[threadIdx.x]) atomicAdd(B.hdr + HDR_HIST + threadIdx.x, h[threadIdx.x]);
}
__global__ __launch_bounds__(256) void batch_order_kernel(Grid g, BatchBufs B) {
    __shared__ unsigned h[33], base[33];
    if (threadIdx.x < 33) h[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned nbricks = (unsigned)(g.nbx * g.nby * g.nbz);
    const unsigned n = min(B.hdr[0], nbricks);
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
        atomicAdd(&h[brick_cost_bin(B.framemask, min(B.list[i], nbricks - 1u))], 1u);
    __syncthreads();
    if (threadIdx.x < 33) {
        // bins in descending order of cost: 32, 31, ..., 1, then 0; this workgroup's range inside its bins
        unsigned start = 0;
        for (unsigned c = 32u; c > threadIdx.x; --c) start += B.hdr[HDR_HIST + c];
        if (threadIdx.x == 0) { start = 0; for (unsigned c = 1u; c <= 32u; ++c) start += B.hdr[HDR_HIST + c]; }
        base[threadIdx.x] = start + (h[threadIdx.x] ? atomicAdd(B.hdr + HDR_CURSOR + threadIdx.x, h[threadIdx.x]) : 0u);
    }
    __syncthreads();
    if (threadIdx.x < 33) h[threadIdx.x] = 0u;
    __syncthreads();
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const unsigned b = min(B.list[i], nbricks - 1u);
        const unsigned c = brick_cost_bin(B.framemask, b);
        const unsigned pos = base[c] + atomicAdd(&h[c], 1u);
        if (pos < nbricks + 64u) B.order[pos] = b;                     // (always: the bins partition the list)
    }
}

// ---- the kernels of the classification cache ------------------------------------------------------------------------------
// The entry points that take a ClassPlan (the bodies they share with the plain kernels are above), the replay and the finish.
__global__ __launch_bounds__(256) void brick_cull_cached_kernel(Cam cam, Grid g, BatchBufs B, Frustum fr, Pyramid py, unsigned *__restrict__ free_cnt,
                                                                ClassPlan P) {
    brick_cull<true>(cam, g, B, fr, py, free_cnt, P);
}
__global__ __launch_bounds__(256) void subbrick_classify_cached_kernel(Cam cam, Grid g, Pyramid py, BatchBufs B, ClassPlan P) {
    subbrick_classify<true>(cam, g, py, B, P);
}
// The replay of a frame whose slot holds its classification: every cached entry through class_tail, 256 per workgroup and trip,
// and at level 2 the sub-brick masks.  Indices read from the buffer are clamped as list entries are everywhere.
__global__ __launch_bounds__(256) void class_replay_kernel(Grid g, BatchBufs B, unsigned *__restrict__ free_cnt, ClassPlan P) {
    if (!class_replays(P, blockIdx.y)) return;
    const unsigned *__restrict__ C = P.cache[blockIdx.y];
    const DescPtr F = const_descs(B) + blockIdx.y;
    __shared__ ClassTailLds S;
    const unsigned nbricks = (unsigned)(g.nbx * g.nby * g.nbz), cap = P.cap;
    const unsigned nm = min(C[0], cap), nf = min(C[1], cap - nm);
    const bool masks = !P.classify_only && C[2] >= 2u;
    const unsigned short *__restrict__ cm = reinterpret_cast<const unsigned short *>(C + CC_HDR_WORDS + cap);
    unsigned short *__restrict__ sub = F->sub;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(P.stats + 1, 1ull);
    for (unsigned i0 = blockIdx.x * 256u; i0 < nm + nf; i0 += gridDim.x * 256u) {
        const unsigned i = i0 + threadIdx.x;
        int cls = 0;
        unsigned brick = 0;
        if (i < nm) {
            brick = min(C[CC_HDR_WORDS + i], nbricks - 1u);
            cls = 1;
            if (masks) sub[brick] = cm[i];
        } else if (i < nm + nf) {
            brick = min(C[CC_HDR_WORDS + (cap - 1u - (i - nm))], nbricks - 1u);
            cls = 2;
        }
        class_tail(g, B, F, free_cnt, blockIdx.y, cls, brick, nullptr, cap, S);
    }
}

// The last kernel of a chain that wrote cache entries, one workgroup per frame: the header of a saved frame (complete only if
// the frame fit), level 2 for an entry that was replayed at level 1 and got its masks from this chain, level 3 for one that this
// chain refined.
__global__ __launch_bounds__(64) void class_finish_kernel(BatchBufs B, ClassPlan P) {
    if (threadIdx.x != 0) return;
    const DescPtr F = const_descs(B) + blockIdx.x;
    unsigned *C = P.cache[blockIdx.x];
    if (class_mode(P, blockIdx.x) == CC_SAVE) {
        const unsigned nm = F->counts[0], nf = F->counts[1];
        const bool fit = nm <= P.cap && nf <= P.cap - nm;
        C[0] = nm; C[1] = nf; C[2] = P.classify_only ? 1u : 2u; C[3] = fit ? 1u : 0u;
        if (!fit) atomicAdd(P.stats + 2, 1ull);
    } else if (class_replays(P, blockIdx.x) && !P.classify_only) {
        if (C[2] < 2u) C[2] = 2u;
        else if (C[2] == 2u && ((P.refine >> blockIdx.x) & 1u)) {
            C[2] = 3u;
            for (int k = 0; k < 4; ++k)
                if (F->counts[REFINE_COUNTS + k]) atomicAdd(P.stats + 4 + k, (unsigned long long)F->counts[REFINE_COUNTS + k]);
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// (the camera is part of the public signature; the layout of a batch scratch does not depend on it)
size_t tsdf_batch_scratch_bytes(const Cam &, const Grid &g, int max_frames) { return batch_layout(g, max_frames).total; }

// One slot's classification buffer for `entries` bricks: header, entries, 16-bit masks (6 B per entry)
size_t tsdf_class_cache_bytes(unsigned entries) { return up256(CC_HDR_WORDS * sizeof(unsigned) + (size_t)entries * (sizeof(unsigned) + sizeof(unsigned short))); }

// One slot's tile buffer: [tile pyramid, float4 per tile, + one float4 whose first word is the valid pixel] [8-B level-0 tiles at *vtile_off]
size_t tsdf_tile_cache_bytes(const Cam &cam, size_t *vtile_off, size_t *vpix_off) {
    const Pyramid p = make_pyramid(cam);
    const size_t off = up256((pyramid_tiles(p) + 1) * sizeof(float4));
    if (vtile_off) *vtile_off = off;
    if (vpix_off) *vpix_off = pyramid_tiles(p) * sizeof(float4);
    return off + up256((size_t)p.ntx[0] * p.nty[0] * sizeof(float2));
}

// bytes of a batch scratch that must be zero before its first use (the frame masks; the update kernel re-arms them)
void tsdf_batch_scratch_zero_range(const Cam &, const Grid &g, int max_frames, size_t *off, size_t *bytes) {
    const BatchLayout L = batch_layout(g, max_frames);
    *off = L.off_mask;
    *bytes = L.off_frames - L.off_mask;
}

// The whole prep of the chain c (c.n frames, one depth kind) on stream s: descriptor upload, depth tiles and pyramid of the
// c.n_stale frames c.stale[] (the others' slots hold them already), resets + cell lists, brick classification, sub-brick masks --
// or, for the frames c.plan marks CC_REPLAY and whose buffer is complete, the replay of both, and for those of c.plan.refine the
// refinement of the replayed masks; c.class_writes != 0: the chain writes cache entries (class_finish_kernel closes it).  `scratch` is a batch scratch of at least c.n frames (tsdf_batch_scratch_bytes).
int launch_tsdf_prepare(hipStream_t s, const Cam &cam, const Grid &g, const Frustum &fr, const PrepChain &c, int max_frames, void *scratch,
                        unsigned *free_cnt, bool classify_only) {
    const int n = c.n, n_stale = c.n_stale;
    const bool class_writes = c.class_writes != 0u;
    if (n < 1 || n > max_frames || n > TL3D_TSDF_MAXBATCH) return set_err(TL3D_E_INVALID, "bad batch size %d", n);
    if (n_stale < 0 || n_stale > n) return set_err(TL3D_E_INVALID, "bad stale count %d", n_stale);
    size_t vt_off = 0;
    (void)tsdf_tile_cache_bytes(cam, &vt_off, nullptr);
    const BatchLayout L = batch_layout(g, max_frames);
    const Pyramid py = make_pyramid(cam);
    char *base = static_cast<char *>(scratch);
    FrameDesc d[TL3D_TSDF_MAXBATCH];
    memset(d, 0, sizeof(d));
    for (int i = 0; i < n; ++i) {
        char *fb = base + L.off_frames + L.per_frame * (size_t)i;
        d[i].pose = c.pose[i];
        d[i].c.mind = c.mind; d[i].c.maxd = c.maxd; d[i].c.sc = c.scale[i];      // (d was zeroed: so are the two unused words)
        d[i].depth = c.depth[i];
        d[i].counts = reinterpret_cast<unsigned *>(fb + L.f_counts);
        d[i].tiles = reinterpret_cast<float4 *>(c.tiles[i]);
        d[i].list = reinterpret_cast<unsigned *>(fb + L.f_list);
        d[i].sub = reinterpret_cast<unsigned short *>(fb + L.f_sub);
        d[i].vtile = reinterpret_cast<float2 *>(static_cast<char *>(c.tiles[i]) + vt_off);
        d[i].cells = reinterpret_cast<unsigned *>(fb + L.f_cells);
    }
    for (int i0 = 0; i0 < n; i0 += 16) {
        DescChunk ch;
        const int m = n - i0 < 16 ? n - i0 : 16;
        memcpy(ch.d, d + i0, (size_t)m * sizeof(FrameDesc));
        if (m < 16) memset(ch.d + m, 0, (size_t)(16 - m) * sizeof(FrameDesc));
        hipLaunchKernelGGL(desc_upload_kernel, dim3(1), dim3(256), 0, s, ch, reinterpret_cast<FrameDesc *>(base + L.off_desc) + i0, m);
        TL3D_HIP(hipGetLastError());
    }
    const BatchBufs B = batch_bufs(L, scratch, n);
    const int nrx = (cam.W + REGION - 1) / REGION, nry = (cam.H + REGION - 1) / REGION;
    const int nreg = nrx * nry;
    if (n_stale > 0) {                                   // the build: only over the frames whose slot has no tiles for these parameters
        StaleList sl;
        memset(&sl, 0, sizeof(sl));
        for (int i = 0; i < n_stale; ++i) {
            if (c.stale[i] >= n) return set_err(TL3D_E_INVALID, "bad stale index %d", (int)c.stale[i]);
            sl.idx[i] = c.stale[i];
        }
        if (c.depth_u16)
            hipLaunchKernelGGL(depth_tiles_kernel<uint16_t>, dim3((nreg + 3) / 4 < 512 ? (nreg + 3) / 4 : 512, n_stale), dim3(256), 0, s, cam, B, py, nrx, nry, sl);
        else
            hipLaunchKernelGGL(depth_tiles_kernel<float>, dim3((nreg + 3) / 4 < 512 ? (nreg + 3) / 4 : 512, n_stale), dim3(256), 0, s, cam, B, py, nrx, nry, sl);
        TL3D_HIP(hipGetLastError());
        hipLaunchKernelGGL(tile_pyramid_kernel, dim3(n_stale), dim3(256), 0, s, cam, py, B, sl);
        TL3D_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(batch_begin_kernel, dim3(n), dim3(256), 0, s, g, fr, py, B);      // (always: resets, cell lists, valid pixels)
    TL3D_HIP(hipGetLastError());
    const int ncells = ((g.nbx + 3) / 4) * ((g.nby + 3) / 4) * ((g.nbz + 3) / 4);
    const int nquad = (ncells + 3) / 4;                 // the cells in view are known only on the device: a fixed grid strides over each frame's list
    // The classification cache (plan: the host's look-up): frames whose slot holds their classification are replayed, the cull
    // and the sub-brick classification return at once for them -- and the other way round.
    const int nbricks = g.nbx * g.nby * g.nbz;
    ClassPlan P = c.plan;
    P.cap = P.cap < (unsigned)nbricks ? P.cap : (unsigned)nbricks;
    P.classify_only = classify_only ? 1 : 0;
    bool any_replay = false;
    for (int i = 0; i < n; ++i) {
        if (class_mode(P, i) != CC_CLASSIFY && (!P.cache[i] || P.cap == 0u)) return set_err(TL3D_E_INVALID, "frame %d: no classification buffer", i);
        any_replay = any_replay || class_mode(P, i) == CC_REPLAY;
    }
    if (n < TL3D_TSDF_MAXBATCH) P.modes &= (1ull << (2 * n)) - 1ull;
    const bool cached = P.modes != 0ull;                 // (else the kernels as they were without the cache; the caller counts the frames as classified)
    if (any_replay) {
        const unsigned trips = (P.cap + 255u) / 256u;
        hipLaunchKernelGGL(class_replay_kernel, dim3(trips < 16u ? trips : 16u, n), dim3(256), 0, s, g, B, free_cnt, P);
        TL3D_HIP(hipGetLastError());
        if (n < TL3D_TSDF_MAXBATCH) P.refine &= (1u << n) - 1u;
        if (P.refine != 0u && !classify_only) {
            const int rc = launch_class_refine(s, cam, g, B, P);
            if (rc != TL3D_OK) return rc;
        }
    }
    if (cached)
        hipLaunchKernelGGL(brick_cull_cached_kernel, dim3(nquad < 256 ? nquad : 256, n), dim3(256), 0, s, cam, g, B, fr, py, free_cnt, P);
    else
        hipLaunchKernelGGL(brick_cull_kernel, dim3(nquad < 256 ? nquad : 256, n), dim3(256), 0, s, cam, g, B, fr, py, free_cnt);
    TL3D_HIP(hipGetLastError());
    if (classify_only) {                                  // (tl3d_count_bricks: which bricks WOULD get records is all that is asked)
        if (class_writes) {
            hipLaunchKernelGGL(class_finish_kernel, dim3(n), dim3(64), 0, s, B, P);
            TL3D_HIP(hipGetLastError());
        }
        return TL3D_OK;
    }
    // The batch list ordered by cost, dearest bricks first (a one-frame batch: every brick costs the same; the update walks the list).
    // A brick's cost is the number of frames that list it -- the frame masks, which the cull has just finished -- so the two small
    // kernels go BEFORE the sub-brick classification, not behind it: beside an update kernel the classification stretches over the
    // whole update period and ends when the update drains, and whatever follows it in the chain sits in front of the next update
    // (12-37 us per 400 us step in the timeline of round 4).  Measured: 78.6-79.0 k frames/s either way (three
    // interleaved runs each) -- the step is bound by the sum of the work, not by that gap; the shorter tail is kept.
    if (n > 1) {
        hipLaunchKernelGGL(batch_hist_kernel, dim3(ORDER_BLOCKS), dim3(256), 0, s, g, B);
        hipLaunchKernelGGL(batch_order_kernel, dim3(ORDER_BLOCKS), dim3(256), 0, s, g, B);
        TL3D_HIP(hipGetLastError());
    }
    // sub-brick masks of the listed bricks (their number is known only on the device: a fixed grid strides over each list)
    int ncb = (nbricks + 31) / 32;                       // 8 bricks per wave, 4 waves per workgroup
    const int cap = n >= 8 ? 128 : 512;
    if (ncb > cap) ncb = cap;
    if (cached)
        hipLaunchKernelGGL(subbrick_classify_cached_kernel, dim3(ncb, n), dim3(256), 0, s, cam, g, py, B, P);
    else
        hipLaunchKernelGGL(subbrick_classify_kernel, dim3(ncb, n), dim3(256), 0, s, cam, g, py, B);
    TL3D_HIP(hipGetLastError());
    if (class_writes) {
        hipLaunchKernelGGL(class_finish_kernel, dim3(n), dim3(64), 0, s, B, P);
        TL3D_HIP(hipGetLastError());
    }
    return TL3D_OK;
}

int launch_fold_free(hipStream_t s, const Grid &g, int2 *grid, unsigned *free_cnt) {
    const unsigned nbricks = (unsigned)(g.nbx * g.nby * g.nbz);
    const unsigned nb = (nbricks + 3u) / 4u < 2048u ? (nbricks + 3u) / 4u : 2048u;
    hipLaunchKernelGGL(fold_free_kernel, dim3(nb ? nb : 1), dim3(256), 0, s, g, grid, free_cnt, nbricks);
    TL3D_HIP(hipGetLastError());
    return TL3D_OK;
}

}  // namespace tl3d
