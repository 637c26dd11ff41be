// tsdf_batch.h -- what the TSDF prep chain (kernels_tsdf_prep.hip) and the TSDF update (kernels_tsdf.hip) share: the layout of a
// batch in device memory (frame descriptors, batch header, counts blocks, scratch) and the tile pyramid's geometry.
#pragma once
#include <string.h>

#include "tl3d_internal.h"

namespace tl3d {

struct TsdfConst {
    float mind, maxd, sc;
    float unused[2];                     // (keeps FrameDesc at 128 bytes and every field behind at its offset)
};

constexpr int TILE0 = 8;                 // level-0 tiles are 8x8 pixels
constexpr int TILE0_SHIFT = 3;
constexpr int REGION = 32;               // one workgroup pass of the tiles kernel: 32x32 pixels = levels 0, 1, 2 of that region
constexpr int MAX_LEVELS = 14;           // 8 px << 13 = 65 536 px
constexpr int TICKET_GROUPS = 64;        // ticket counters of the update kernel (one per group of workgroups)
constexpr unsigned HDR_TICKETS = 64;     // batch header (unsigned words): [0] batch list length, [64 + 16 g] ticket counter of group g
constexpr unsigned HDR_HIST = HDR_TICKETS + 16 * TICKET_GROUPS;      // [33] bricks of the batch list by the number of frames that list them ...
constexpr unsigned HDR_CURSOR = HDR_HIST + 64;                       // [33] ... and the cursors of the counting sort (batch_order_kernel)
constexpr unsigned HDR_WORDS = HDR_CURSOR + 64;

struct Pyramid {
    int nlev;
    int ntx[MAX_LEVELS], nty[MAX_LEVELS], off[MAX_LEVELS];     // per level: tiles in x / y, offset into the float4 array
};

// One frame of a batch.  The array of a batch's descriptors is written by the host and copied to the device in front of the
// batch's first kernel; every kernel indexes it with a wave-uniform frame number (scalar loads).
struct FrameDesc {
    PoseF pose;                          // [0, 48)
    TsdfConst c;                         // [48, 68)
    unsigned valid_pix;                  // [68] index of ONE pixel of the frame that is valid (written by tile_pyramid_kernel); the update
                                         //      kernel sends the lanes whose depth value cannot matter there
    const void *depth;                   // [72] f32 metres, or the 16-bit millimetre image (one kind per batch)
    float2 *vtile;                       // [80] level-0 tiles, 8 B each, as the update kernel's per-voxel test wants them (below)
    float4 *tiles;                       // the frame's tile pyramid
    unsigned *list;                      // its listed (MIXED) bricks, for the sub-brick classification
    unsigned *counts;                    // [0] listed bricks, [1] free-space bricks (counted)
    unsigned short *sub;                 // [nbricks] sub-brick masks of its listed bricks: bits 0-7 mixed, bits 8-15 free
    unsigned *cells;                     // the 4x4x4-brick cells whose bounding sphere meets the view (the cull kernel's work list); count: counts[CELL_COUNT]
};
static_assert(sizeof(FrameDesc) == 128, "FrameDesc: 16 of them travel as one kernel argument block");

// what all frames of a batch share
struct BatchBufs {
    const FrameDesc *frames;             // [n_frames]
    unsigned *hdr;                       // [0] length of the batch list (reset by batch_begin_kernel)
    unsigned *list;                      // bricks that at least one frame of the batch lists, in order of first listing
    unsigned *order;                     // the same bricks, dearest first (by the number of frames that list them): what the update walks
    unsigned *framemask;                 // [nbricks] bit f: frame f lists the brick; all zero between batches (the update re-arms it)
    int n_frames;
};

// The descriptors do not change while a kernel that reads them runs: read through the constant address space, a wave-uniform
// index turns into scalar loads (pose and limits live in SGPRs) -- through a plain pointer the compiler must assume that the
// kernel's own stores could alias them and uses vector loads, 17 VGPRs per frame in flight.
typedef const FrameDesc __attribute__((address_space(4))) *DescPtr;
__device__ __forceinline__ DescPtr const_descs(const BatchBufs &B) { return (DescPtr)(B.frames); }
__device__ __forceinline__ PoseF desc_pose(DescPtr d) {
    PoseF p;
#pragma unroll
    for (int i = 0; i < 9; ++i) p.r[i] = d->pose.r[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) p.t[i] = d->pose.t[i];
    return p;
}
__device__ __forceinline__ TsdfConst desc_const(DescPtr d) {
    TsdfConst c;
    c.mind = d->c.mind; c.maxd = d->c.maxd; c.sc = d->c.sc; c.unused[0] = c.unused[1] = 0.0f;
    return c;
}

// words of a frame's counts block beyond [0] and [1]
constexpr int REFINE_COUNTS = 8;         // words 8-11: what class_refine_kernel decided for the frame's pairs (reset with the list cursors)
constexpr int VALID_PIXEL = 32;          // ONE PIXEL OF THE FRAME THAT IS VALID (tile_pyramid_kernel)
constexpr int CELL_COUNT = 48;           // length of the frame's cell list

// frame f of the plan is replayed from its slot's classification entry, and the entry is complete (the cache: kernels_tsdf_prep.hip)
__device__ __forceinline__ bool class_replays(const ClassPlan &P, int f) {
    return class_mode(P, f) == CC_REPLAY && P.cache[f][3] == 1u;
}

// class_refine_kernel is a link of the prep chain, launched by launch_tsdf_prepare, and lives in kernels_tsdf.hip beside the
// update kernel whose stage A and tile test it shares (the reason is given there)
int launch_class_refine(hipStream_t s, const Cam &cam, const Grid &g, const BatchBufs &B, const ClassPlan &P);

// ---- host side: the pyramid's geometry and the layout of a batch scratch ----------------------------------------------------------
static inline Pyramid make_pyramid(const Cam &cam) {
    Pyramid p;
    memset(&p, 0, sizeof(p));
    int nx = (cam.W + TILE0 - 1) / TILE0, ny = (cam.H + TILE0 - 1) / TILE0, off = 0, L = 0;
    for (;;) {
        p.ntx[L] = nx; p.nty[L] = ny; p.off[L] = off;
        off += nx * ny;
        ++L;
        if ((nx == 1 && ny == 1) || L == MAX_LEVELS) break;
        nx = (nx + 1) / 2;
        ny = (ny + 1) / 2;
    }
    p.nlev = L;
    return p;
}

static inline size_t pyramid_tiles(const Pyramid &p) { return (size_t)p.off[p.nlev - 1] + (size_t)p.ntx[p.nlev - 1] * p.nty[p.nlev - 1]; }

static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// Scratch of ONE batch in flight (the context keeps two and alternates):
//   [descriptors (max_frames)] [header 256 B] [batch list] [frame masks] then per frame [counts 256 B] [list] [sub-brick masks] [cell list]
// (the tile pyramid and the 8-B level-0 tiles of a frame live with its slot: tsdf_tile_cache_bytes)
struct BatchLayout {
    size_t off_desc, off_hdr, off_list, off_order, off_mask, off_frames, per_frame, f_counts, f_list, f_sub, f_cells, total;
};
static inline BatchLayout batch_layout(const Grid &g, int max_frames) {
    const size_t nbricks = (size_t)g.nbx * g.nby * g.nbz;
    BatchLayout L;
    L.off_desc = 0;
    L.off_hdr = up256((size_t)max_frames * sizeof(FrameDesc));
    L.off_list = L.off_hdr + up256(HDR_WORDS * sizeof(unsigned));
    L.off_order = L.off_list + up256((nbricks + 64) * sizeof(unsigned));
    L.off_mask = L.off_order + up256((nbricks + 64) * sizeof(unsigned));
    L.off_frames = L.off_mask + up256(nbricks * sizeof(unsigned));
    L.f_counts = 0;
    L.f_list = 256;
    L.f_sub = L.f_list + up256((nbricks + 64) * sizeof(unsigned));
    L.f_cells = L.f_sub + up256(nbricks * sizeof(unsigned short));
    const size_t ncells = (size_t)((g.nbx + 3) / 4) * ((g.nby + 3) / 4) * ((g.nbz + 3) / 4);
    L.per_frame = L.f_cells + up256((ncells + 4) * sizeof(unsigned));
    L.total = L.off_frames + L.per_frame * (size_t)max_frames;
    return L;
}

static inline BatchBufs batch_bufs(const BatchLayout &L, void *scratch, int n) {
    char *base = static_cast<char *>(scratch);
    BatchBufs B;
    B.frames = reinterpret_cast<const FrameDesc *>(base + L.off_desc);
    B.hdr = reinterpret_cast<unsigned *>(base + L.off_hdr);
    B.list = reinterpret_cast<unsigned *>(base + L.off_list);
    B.order = reinterpret_cast<unsigned *>(base + L.off_order);
    B.framemask = reinterpret_cast<unsigned *>(base + L.off_mask);
    B.n_frames = n;
    return B;
}

}  // namespace tl3d
