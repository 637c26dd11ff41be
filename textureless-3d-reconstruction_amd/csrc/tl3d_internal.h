// tl3d_internal.h -- shared declarations of libtl3d.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tl3d.h"

namespace tl3d {

// ---- parameter blocks passed to kernels by value ---------------------------------------------
struct Cam {
    int W, H;
    float fx, fy, cx, cy;        // f32 path (TSDF, normals, ICP)
    double fxd, fyd, cxd, cyd;   // fp64 path (reference-exact back-projection)
};

// PHASE-MAJOR ROWS (normal maps and window-averaged depth: what the registration gathers from).  Pixel u of a row sits at
// (u & 3) * W4 + (u >> 2), W4 = ceil(W / 4): the row is kept as its four pixel phases one after the other.  A registration level
// samples every stride-th pixel (stride 4 and 2 in the pipeline's schedule) and the projected targets of neighbouring samples keep
// the stride over long runs, so in a row-major map every sample pays a 64-B sector of its own for a 16-B entry (8.3 MB fetched
// per 1080p pair-iteration at stride 4 for 2.1 MB used); here samples 4 px apart are neighbours in memory: four entries per
// sector.  Stride-1 accesses cost the same sectors as before (64 consecutive pixels = four runs of 16 entries).  Same values,
// another address: every result is bit for bit what the row-major map gave.
__host__ __device__ __forceinline__ int pm_w4(int W) { return (W + 3) >> 2; }
__host__ __device__ __forceinline__ size_t pm_pixels(int W, int H) { return (size_t)4 * pm_w4(W) * H; }
__host__ __device__ __forceinline__ size_t pm_index(int u, int v, int w4) { return (size_t)v * (size_t)(4 * w4) + (size_t)((u & 3) * w4 + (u >> 2)); }

struct Grid {
    int nx, ny, nz;              // voxels
    int nbx, nby, nbz;           // bricks (8^3 voxels)
    float ox, oy, oz, vs;        // f32 origin / voxel size (TSDF path)
    double oxd, oyd, ozd, vsd;   // fp64 (centroid path, Open3D index semantics)
    double offx, offy, offz;     // the grid's voxel (0,0,0) is voxel (offx, offy, offz) of the lattice that starts at the origin (integers; centroid path)
    int vox, voy, voz;           // the same offset as integers (TSDF path: a voxel centre is fma((float)(off + i) + 0.5f, vs, origin), exact below 2^23)
    int clo[3], chi[3];          // block core, grid-local voxels [clo, chi) (tl3d_set_block_core); [0, n) without one
    float trunc, inv_trunc;
    // Brick tables: the records of virtual brick b of a channel sit in pool slot table[b] (512 records each).  A dense grid has
    // the identity table and a pool of every brick; a SPARSE grid starts with an empty table and hands out slots on first
    // touch (brick_slot_ensure) until its pool is full.  cursors: [0] TSDF slots handed out, [1] TSDF refusals (pool full),
    // [2] / [3] the same for the centroid channel.
    unsigned *tsdf_tab, *cen_tab, *cursors;
    unsigned tsdf_cap, cen_cap;
    const unsigned *free_cnt;    // per-brick free-space counts not yet folded into records (readers add them: see tsdf_record)
};
constexpr unsigned SLOT_EMPTY = 0xffffffffu;    // no records yet
constexpr unsigned SLOT_PENDING = 0xfffffffeu;  // a wave is drawing the brick's slot right now (inside the allocating kernel only)
constexpr unsigned SLOT_FULL = 0xfffffffdu;     // the pool had no slot left when the brick was first touched: its updates are dropped (counted)
                                                // (every value >= SLOT_FULL reads as "no records")

struct PoseF {                   // world->camera, f32 (or src->tgt for ICP)
    float r[9];
    float t[3];
};

struct PoseD {                   // fp64 R (row-major) and ct = R^T t, for the back-projection path
    double r[9];
    double ct[3];
};

struct BpArgs {                  // back-projection arguments common to count / write / centroid kernels
    int sub, Ws, Hs;             // stride and subsampled extent (ceil)
    unsigned flags;
    double scale, min_d, max_d;
    unsigned long long zero;     // 0 the compiler cannot see: fetch_add(p, zero) stays a read-modify-write (a fresh read, see bp look-back)
};

// one frame of a batch of voxel-centroid accumulations (kernels_centroid.hip)
constexpr int TL3D_CEN_MAXBATCH = 32;
struct CenFrame {
    PoseD p;
    BpArgs a;
    const float *depth;
    const uint8_t *bgr;
};

// frustum side planes for brick culling: inside iff nx*x + nz*z >= -rad (left/right), ny*y + nz*z >= -rad
struct Frustum {
    float lx, lz, rx, rz, ty, tz, by, bz;
};

struct IcpState {                // lives in device memory for the whole ICP run (no host round trips)
    double T[16];
    double sums[40];             // last reduced sums: a[21] b[6] e cnt nsrc . . c[6] cc bc (scale column, Sim(3) runs only)
    double scale;                // metric scale of the source depth: the caller's value, updated by runs that estimate it
    int done;                    // set on convergence or failure: remaining iteration kernels exit at once
    int status;
    int iters_run;
    int over;                    // batched runs: no further level follows (last level done, failed, or < 8 correspondences)
};
constexpr int ICP_SUM_E = 27, ICP_SUM_CORR = 28, ICP_SUM_SRC = 29;   // e, cnt and nsrc of IcpState::sums, for the host's read-outs (api_register.hip)

// What a pass of tracking, colour or cloud registration (and the step behind it) is.  STEP_ITERATE: sums, solve, pose update; skipped
// once the level is done.  STEP_END_LEVEL: sums only, at the level's last pose, and another level follows: the run is over when the
// level failed or ended with fewer than 8 correspondences, else done / status / iters_run are re-armed (what a host does between
// tl3d_icp_p2plane calls).  STEP_END_RUN: sums only; nothing follows.  (The pairwise ICP's own final_pass is a 0 / 1 flag.)
enum StepKind : int { STEP_ITERATE = 0, STEP_END_LEVEL = 1, STEP_END_RUN = 2 };
// pass `it` of a level with `updates` update passes: those iterate, the one after them ends the level; an evaluation is that last pass alone
inline StepKind step_kind(int it, int updates, bool last_level, bool evaluate) {
    if (!evaluate && it < updates) return STEP_ITERATE;
    return last_level || evaluate ? STEP_END_RUN : STEP_END_LEVEL;
}

struct IcpRun {                  // per-run arguments of the ICP kernels, read from device memory so that a lane's
    const float *depth_src;      // kernel chain has constant launch arguments and can be replayed as a hipGraph
    const float4 *nmap_tgt;
    float scale, md2, mind, maxd;
    int stride, Ws, Hs, est_scale;   // est_scale: the source depth's scale is a 7th unknown (Sim(3))
    double damping, eps, eig_rel;
    int src_pm, pad;             // src_pm: depth_src is a window-averaged depth in phase-major rows (pm_index), else the frame's row-major image
};

// Batched registration (icp_batch_kernel): every pair of a batch runs ALL its levels and iterations inside one launch.
constexpr int ICP_MAX_LEVELS = 4;
constexpr int ICP_BATCH_MAX_MEMBERS = 64;    // workgroups that may share one pair (what the buffers are sized for)
// Samples per member and pass.  A member's pass costs ~4.5 us whatever it accumulates (wave + workgroup reduction, partial store,
// arrival, barriers, poll) plus ~0.55 us per sample and thread; measured on 255 pairs of 1080p frames (tools/bench_icp.py, round 4,
// two slots per workgroup): stride 4 at 32 / 16 / 8 members per pair 1.35 / 1.03 / 0.92 us per pair-iteration, the two-level
// schedule 57 / 66 / 65 k pairs/s (45 k with the 64 members of round 3).  16 members at 1080p stride 4, at most 32: a pair
// registered alone still spreads over 16-32 CUs.  A function of the level geometry only, never of the batch: a pair's sums (and
// pose) do not depend on the batch it is in.
constexpr int ICP_BATCH_SAMPLES_PER_MEMBER = 8192;
constexpr int ICP_BATCH_MEMBERS_CAP = 32;
struct IcpBatchPair { const float *depth_src; const float4 *nmap_tgt; float scale; int src_pm; };    // src_pm: as IcpRun::src_pm
struct IcpLevel { float md2; int stride, Ws, Hs, iters, est_scale; double damping, eps, eig_rel; };
struct IcpBatchArgs {
    const IcpBatchPair *pairs;   // [n_pairs]
    IcpState *states;            // [n_pairs] initial pose in, result out
    unsigned *sync;              // two arrays of 64 x sync_rows 64-B lines: arrival counters, then generation lines (zero at launch);
                                 // pair p owns line (p % 64) * sync_rows + p / 64 of each
    double *slab;                // [n_pairs][members][ICP_SLAB] partial sums of the current pass
    unsigned *ctl;               // [0] workgroup tickets handed out, [1] error (a wait timed out); zero at launch
    int n_pairs, members, n_levels, sync_rows, zero;    // zero: 0 the compiler cannot see (an add of it stays a read-modify-write)
    float mind, maxd;
    unsigned *stage;             // experiments: [n_pairs * members][4] progress markers (null in production)
    unsigned long long *dbg;     // experiments: [members][16 passes][8] timestamps of pair 0 (null in production)
    IcpLevel lv[ICP_MAX_LEVELS];
};

// Evaluation of pairs at given poses (kernels_icp_eval.hip, tl3d_icp_evaluate_pairs): one pass, no update.  Workgroups per pair: a
// function of the level geometry only (a pair's sums do not depend on the batch it is in); 8192 samples per workgroup = 32 per
// thread, eight trips of the sample loop, against one partial of 256 B written and read back.
constexpr int ICP_EVAL_SAMPLES_PER_MEMBER = 8192;
constexpr int ICP_EVAL_MEMBERS_CAP = 256;
constexpr int ICP_EVAL_SUMS = 32;            // doubles per partial and per result: a[21] b[6] e cnt nsrc 0 0 (the head of IcpState::sums)
constexpr size_t ICP_EVAL_SLAB_DOUBLES = (size_t)1 << 23;   // partials of one chunk of pairs: 64 MB at most (a chunk is never less than one pair)
struct IcpEvalPair { const float *depth_src; const float4 *nmap_tgt; float scale; int src_pm; float T[12]; };    // T: rows 0..2 of the pose, f32

// Point-to-SDF tracking (kernels_track.hip): the arguments of one pass; the pose is read from an IcpState in device memory
struct TrackArgs {
    const float *depth;          // the slot's f32 depth, row-major [H][W]
    float scale, mind, maxd;
    float ivs;                   // (float)(1 / voxel size), as RayArgs
    float gate;                  // |F| <= gate: min((float)max_dist / trunc, 0.98f)
    float nk;                    // trunc * ivs: a per-voxel gradient of F -> metres per metre
    int mw;                      // max(1, min_weight)
    int stride, Ws, Hs, tx, ty;  // sampled extent (ceil) and its 8 x 8 tiles
};
constexpr int TRACK_SUMS = 32;   // doubles per partial: the head of IcpState::sums

// Joint point-to-plane + photometric registration (kernels_rgbd.hip).  A partial and a pair's totals are 64
// doubles: [0, 32) the geometric system laid out as the head of IcpState::sums (a[21] b[6] e n_corr n_src), [30] the geometric
// correspondences whose two intensity records qualify (before the photometric gate); [32, 64) the photometric system a_p[21] b_p[6]
// e_p n_photo 0 0 0.  The two systems stay apart until the step kernel forms a + weight * a_p.
constexpr int RGBD_SUMS = 64;
constexpr int RGBD_SUM_ELIG = 30, RGBD_SUM_E_P = 32 + 27, RGBD_SUM_PHOTO = 32 + 28;
constexpr int RGBD_SAMPLES_PER_MEMBER = 4096;   // workgroups per pair: a function of the level geometry only (rgbd_members)
constexpr int RGBD_MEMBERS_CAP = 64;
struct RgbdPair {                // what the pass reads of a pair
    const float *depth_src;      // as IcpBatchPair: the slot's depth, or its window-averaged one in phase-major rows (src_pm)
    const float4 *nmap_tgt;      // phase-major rows
    const float4 *imap_src, *imap_tgt;   // intensity maps (S, Sx, Sy, flag), phase-major rows
    float scale;
    int src_pm;
};
struct RgbdState {               // per pair, in device memory for the whole run
    IcpState icp;                // pose, geometric sums (sums[30]: the qualifying correspondences), done / status / iters_run / over
    double photo[32];            // a_p[21] b_p[6] e_p n_photo 0 0 0
};
struct RgbdLevel {               // one level as the pass takes it
    float md2, photo_gate, mind, maxd;
    int stride, Ws, Hs, members;
};

// Everything the TSDF brick and sub-brick classification of a frame depends on besides the slot's tiles and the camera, as the
// kernels get it (f32 words after the double -> float conversions); compared bitwise.
struct ClassKey {
    uint32_t w[26] = {};         // pose r[9] t[3], scale, min / max depth, nbx nby nbz, vox voy voz, ox oy oz vs, trunc
};
// How the classification kernels of one prep chain treat each frame (a kernel argument, indexed by the frame number).
constexpr unsigned char CC_CLASSIFY = 0;    // classify, as without the cache
constexpr unsigned char CC_SAVE = 1;        // classify and record the result in cache[f]
constexpr unsigned char CC_REPLAY = 2;      // replay cache[f] if its header says the frame fit (the device knows), else classify
constexpr int CC_HDR_WORDS = 16;            // header of a buffer: [0] MIXED entries, [1] FREE entries, [2] level, [3] 1 = complete
struct ClassPlan {
    unsigned *cache[32];         // [TL3D_TSDF_MAXBATCH] the slot's buffer: header, entries[cap] (MIXED from the front, FREE from the back), u16 masks[cap]
    unsigned long long modes;    // two bits per frame (class_mode): a shift and a mask on the scalar unit; 0 = no frame of the chain uses the cache
    unsigned cap;               // entries a buffer holds for this grid: min(configured entries, bricks of the grid)
    int classify_only;
    unsigned refine;             // bit f: the chain refines frame f's replayed level-2 entry and leaves level 3 (class_refine_kernel)
    unsigned long long *stats;   // device counters: [0] frames classified, [1] replayed, [2] of the classified: did not fit (tl3d_class_cache_info);
                                 // [4..8] of the refinement: pairs seen, dropped, turned FREE, decided with both kinds of lane, masks that did not fit (tl3d_class_refine_info)
};
__host__ __device__ __forceinline__ unsigned class_mode(const ClassPlan &P, int f) { return (unsigned)(P.modes >> (2 * f)) & 3u; }
inline void class_set_mode(ClassPlan &P, int f, unsigned mode) { P.modes = (P.modes & ~(3ull << (2 * f))) | ((unsigned long long)mode << (2 * f)); }
static_assert(sizeof(ClassPlan) <= 320, "ClassPlan travels as a kernel argument beside Grid, Cam and Pyramid (4 KB in all)");

// A product kept in a slot's cache block (Slot::tc: the tiles, Slot::cc: the classification), beside its key: who wrote it and who
// used it last.  What a prep chain waits for before it reads or overwrites the product follows from these four (api_fuse.hip: ChainOrder).
struct Cached {
    bool valid = false;          // the product is there, made under the key beside it
    bool used = false;           // some chain has read or written it (the tiles: since the slot's last upload): use_batch is the last one's number
    unsigned write_batch = 0, use_batch = 0;    // tl3d_ctx::tsdf_batch_no of the batch whose chain wrote it last / used it last
};

// The frames of one prep chain and what the cache look-ups decided for them (api_fuse.hip: issue_prep_chain, launch_tsdf_prepare)
struct PrepChain {
    int n;                       // frames
    bool depth_u16;              // depth[] are millimetre images (one depth kind and one pair of limits per chain)
    float mind, maxd;
    int slot[32];                // [TL3D_TSDF_MAXBATCH], as the next five
    PoseF pose[32];
    float scale[32];
    const void *depth[32];
    void *tiles[32];             // the slot's tile buffer (tsdf_tile_cache_bytes); frames of one slot share it and at most one of them is stale
    unsigned char stale[32];     // the n_stale frames (indices into the chain, one per slot) that build their tiles
    int n_stale;
    ClassPlan plan;
    unsigned class_writes;       // bit i: the chain writes frame i's classification entry (class_finish_kernel closes it)
};

// Frame buffers come from slabs, not one hipMalloc per buffer: a 1000-frame context used to make (and, slower, free) 4000
// allocations.  One pool per buffer kind (equal-sized blocks); a slab holds up to 64 blocks and lives until tl3d_destroy.
constexpr int FRAME_SLAB_BLOCKS = 64;
struct FramePool {
    size_t block = 0;             // bytes per block, rounded up to 256
    int remaining = 0;            // blocks this pool may still hand out (= frame slots without a buffer of this kind)
    char *cur = nullptr;          // next free block of the newest slab
    int cur_left = 0;
    void **slabs = nullptr;       // [max_slabs]
    size_t *slab_bytes = nullptr; // [max_slabs] size of each slab (they go back to the process-wide slab cache by size)
    int n_slabs = 0, max_slabs = 0;
    int device = 0;
};

struct Slot {
    float *depth = nullptr;      // [H][W] f32
    uint16_t *depth_u16 = nullptr;   // [H][W] millimetres, kept when the frame was uploaded as TL3D_DEPTH_U16_MM (TSDF gathers read it)
    bool has_u16 = false;
    uint8_t *bgr = nullptr;      // [H][W][3]
    float4 *nmap = nullptr;      // [H][4 * W4] (nx,ny,nz,d) in phase-major rows (pm_index), lazily allocated
    float *sdepth = nullptr;     // [H][4 * W4], phase-major rows: window-averaged depth the normal map was taken from (tl3d_set_normal_smoothing > 0); registration reads it as the source depth too
    int smooth_radius = 0;       // radius sdepth / nmap were built with (0: nmap from the depth image itself)
    hipEvent_t ev_upload = nullptr;   // recorded on the main stream after the slot's last upload
    hipEvent_t ev_normals = nullptr;  // recorded on the main stream after the slot's normal map was built
    bool has_color = false;
    bool loaded = false;
    bool has_normals = false;
    // Intensity map of the colour image (kernels_rgbd.hip: S, Sx, Sy, flag per pixel, phase-major rows), lazily allocated from
    // tl3d_ctx::pool_imap; it is made from the slot's depth AND colour: slot_rewritten voids it with the normal map.
    float4 *imap = nullptr;
    bool has_intensity = false;
    hipEvent_t ev_intensity = nullptr;   // recorded on the main stream after the slot's intensity map was built
    // TSDF tile cache: what the TSDF prep derives from the depth image, the scale and the depth limits alone (kernels_tsdf_prep.hip:
    // depth_tiles_kernel, tile_pyramid_kernel).  One lazily allocated block (tl3d_ctx::pool_tiles, tsdf_tile_cache_bytes) and the
    // key it was built with; every writer of `depth` calls slot_rewritten (tl3d_api.hip), which clears tc.  The u16 and f32 images give
    // the same tiles (mm_to_m is the conversion the f32 copy was made with, no contraction, no fast math): the depth kind is no part of the key.
    float4 *tiles = nullptr;     // pyramid, all levels; the float4 behind the last level holds ...
    unsigned *vpix = nullptr;    // ... the frame's valid pixel (device word)
    float2 *vtile = nullptr;     // level-0 tiles as 8-B records
    uint32_t tc_scale_bits = 0;  // key: bits of the f32 scale, the depth limits
    float tc_mind = 0, tc_maxd = 0;
    Cached tc;
    // TSDF classification cache: the brick cull's and the sub-brick classification's result for ONE key (ClassKey: pose, scale,
    // depth limits, grid geometry), replayed when a batch meets the slot again with that key (kernels_tsdf_prep.hip:
    // class_replay_kernel).  It lives behind the tiles in the slot's block of tl3d_ctx::pool_tiles (tsdf_class_cache_bytes).  It is made from the
    // slot's tiles: every rebuild of those drops it (api_fuse.hip: tile_cache_lookup).  cc_level: 1 = lists and counts (what a
    // classify-only chain can fill), 2 = + sub-brick masks, 3 = masks refined by the per-voxel tile test (class_refine_kernel: the first
    // fusion chain that replays a level-2 entry and holds the slot once).  Whether the frame FIT is known to the device alone (the buffer's header).
    unsigned *cls = nullptr;
    ClassKey cc_key;             // key, with cc_level
    int cc_level = 0;
    Cached cc;
};

// One part of a mesh weld (kernels_meshweld.hip) as the kernels see it: the part's arrays in device memory and the vertices and
// triangles of the parts in front of it.  The list has one entry more than parts: its v0 / t0 are the totals.
struct WeldPart {
    const float *xyz;
    const uint8_t *rgb;          // null in every part or in none
    const long long *key;
    const unsigned *tri;
    unsigned long long v0, t0;
    long long lo[3], hi[3];      // the core [lo, hi) in lattice voxels
};

constexpr int ICP_MAX_BLOCKS = 256;     // one reduce workgroup per CU; the solve sums the slab serially
constexpr int ICP_SLAB = 40;     // doubles per block partial: 30 sums of the pose system (+ 2 unused), 8 of the scale column

}  // namespace tl3d

// TSDF updates are issued in batches of up to TL3D_TSDF_MAXBATCH frames (one bit per frame in a brick's frame mask): one prep
// chain (5 launches) for the whole batch on the side stream, then ONE update launch on the main stream that reads and writes
// every touched record once per batch.  Four batch scratch buffers are taken in turn (three prep streams), so the prep chains of
// the next batches run beside the update of batch k.
#define TL3D_TSDF_MAXBATCH 32
constexpr int TSDF_SCRATCHES = 4;

// Everything that lives exactly as long as the context's grid (tl3d_create with channels / tl3d_attach_grid ... tl3d_detach_grid /
// tl3d_destroy): the channels, their brick tables, and every buffer, event and cached result whose size or meaning depends on the
// grid.  All zero = "no grid".  release_grid (tl3d_api.hip) is the one place that frees it, and it resets the whole struct, so a
// new grid-sized member needs a line there only if it owns something.
struct tl3d_grid_state {
    tl3d::Grid grid;
    size_t nvox;
    int2 *tsdf;                  // record pool of the TSDF channel: [tsdf_cap bricks][512] {sum_q, weight}; a dense grid's pool is the grid
    unsigned long long *centroid;// record pool of the centroid channel: [cen_cap bricks][512][4]
    bool own_tsdf, own_centroid;
    bool sparse;                 // pools smaller than the grid, slots handed out on first touch (tl3d_config.pool_bricks_*)
    unsigned *brick_tabs;        // one allocation: TSDF table [nbricks], centroid table [nbricks], cursors [4]
    void *tsdf_scratch[TSDF_SCRATCHES];   // batch scratch (descriptors, tile pyramids, brick lists, frame masks, sub-brick masks), one per batch in
                                          // flight: the update of batch k on the main stream, the prep chains of the next batches on the prep streams
    void *tsdf_scratch_slab;              // the one allocation they are carved from
    hipEvent_t ev_upd[TSDF_SCRATCHES];                 // the update of the last batch that used scratch h is done (main stream)
    bool upd_recorded[TSDF_SCRATCHES];
    // extraction is called twice (size query, then with buffers): the block counts of the query are kept while nothing
    // has touched the grids in between (every grid-modifying or pointer-exposing call bumps tl3d_ctx::grid_epoch)
    unsigned long long ext_epoch, ext_total;
    int ext_mode, ext_min_count, ext_min_weight;
    double ext_max_abs;
    bool ext_valid;
    unsigned *block_counts;      // compaction counts
    unsigned long long *block_offsets;
    size_t scratch_blocks;       // capacity of both, in blocks
    // tl3d_extract_mesh: counts of the size query (same reuse rule), per-block vertex / triangle counts and their offsets,
    // and each vertex owner's first vertex id ([TSDF pool slots][512] u32, grown on demand)
    unsigned long long mesh_epoch, mesh_nv, mesh_nt;
    int mesh_min_weight;
    bool mesh_valid;
    unsigned *mesh_counts;                  // [2][blocks]: vertices, then triangles
    unsigned long long *mesh_offsets;       // [2][blocks]
    size_t mesh_blocks;                     // capacity of both, in entries (two per block)
    unsigned *mesh_first;
    size_t mesh_first_n;
    // The device scratch of the mesh calls (api_mesh.hip) and of the calls on the uniform cell index (kernels_sor.hip,
    // kernels_nearest.hip, kernels_normals.hip, kernels_planes.hip): the two grow-on-demand buffers every call carves its arrays
    // from (scratch_carve, api_host.h; nothing in them is live across calls) and the fixed slab (CELL_SLAB_BYTES) of the cell-index calls' block partials.  None of it
    // depends on the grid (the calls work without one): it lives here so that tl3d_detach_grid gives the memory back.
    char *scratch[2];
    size_t scratch_bytes[2];                // capacities
    void *cg_slab;
    // The eight report words of a mesh call's carve, zeroed by the call before its first kernel:
    //   word   tl3d_mesh_components / _filter_components       tl3d_mesh_simplify_clusters   tl3d_mesh_smooth_taubin / _vertex_normals
    //   [0]    largest triangle index (its low u32 word)       the same                      the same
    //   [1]    components                                      vertices without a cell       vertices out of range
    //   [2]    key of the largest component (cc_roots_kernel)  degenerate triangles          unique edges
    //   [3]    kept components                                 duplicate triangles           a step left the range / zero normals
    //   [4]                                                    corners skipped (quadric)     a step left the range (steps take [3], [4] in turn)
    //   [5]                                                    clusters placed by a quadric
    //   [6]                                                    clusters clamped
    // tl3d_mesh_weld_keyed: [0] indices out of range, [1] keys out of range, [2] the largest offending (part << 32 | index),
    // [3] vertices owned twice, [4] unowned corners
    // tl3d_set_block_core: the grid is one block of a lattice of lat[] voxels and emits only what its core (grid.clo / chi) owns
    bool has_core;
    long long lat[3];
    // Free-space counters: a brick that is wholly free space in a frame gets +1 here (one integer add by the classification
    // kernel) instead of (+32767, +1) on each of its 512 records; the pending counts are folded into the records before
    // anything reads the TSDF channel.
    unsigned *free_cnt;
    bool free_dirty;
    // int32 headroom of the TSDF sums: |sum_q| <= weight * 32767 stays below 2^31 while weight <= TL3D_TSDF_MAX_WEIGHT.
    // tsdf_w_upper bounds the largest voxel weight from above (+1 per integrated frame); when it reaches the limit, or after
    // a merge the library could not see (grid upload, grid pointer handed out), it is re-measured by a reduction over the grid
    long long tsdf_w_upper;
    bool tsdf_w_unknown;
};

struct tl3d_ctx : tl3d_grid_state {
    tl3d_config cfg;
    int device;
    hipStream_t stream;
    bool own_stream;
    tl3d::Cam cam;
    tl3d::Slot *slots;
    tl3d::FramePool pool_depth, pool_u16, pool_bgr, pool_nmap, pool_sdepth, pool_tiles, pool_imap;
    int normal_radius;           // tl3d_set_normal_smoothing: window radius of the next normal maps (0: none)
    // scratch
    // TSDF integration: the prep chain of a batch (tiles, pyramid, cull, brick classes) runs on a prep stream while the update
    // kernel of the batch before it streams the grid on the main stream.
    hipStream_t prep_stream[4];  // consecutive BATCHES take them in turn (three by default: one per batch scratch)
    int n_prep_streams;
    bool tsdf_pairing;                    // frames of a batch share ONE update launch (tl3d_set_tsdf_pairing(ctx, 0): one frame per launch)
    hipEvent_t ev_prep[TSDF_SCRATCHES];                // prep of the batch using scratch h is done (recorded on its prep stream)
    bool tsdf_use_u16;                    // gather from the millimetre image when the slot has one (env TL3D_U16_GATHER=0: never)
    int tsdf_batch;                       // frames per batch (env TL3D_TSDF_BATCH, default 32; 1 = no deferral)
    unsigned tsdf_batch_no;
    // TSDF tile cache (Slot::tiles): off = every look-up is a miss (env TL3D_TILE_CACHE=0, read when the context is created);
    // every batch numbered below tc_done_before is known complete on the device (the host has waited since); per-frame builds
    // and look-ups that found tiles (tl3d_tile_cache_info)
    bool tile_cache;
    unsigned tc_done_before;
    unsigned long long tc_builds, tc_hits;
    // TSDF classification cache (Slot::cls): off = every look-up classifies (env TL3D_CLASS_CACHE=0, or the tile cache off);
    // entries per slot buffer (env TL3D_CLASS_CACHE_ENTRIES); both read when the context is created
    bool class_cache;
    bool class_refine;                    // a replayed level-2 entry is refined to level 3 (env TL3D_CLASS_REFINE=0: never), read like its siblings
    unsigned cc_entries;
    size_t tc_bytes, cc_bytes;            // of a slot's block in pool_tiles: the tiles' part, the classification buffer behind it (0: cache off)
    unsigned long long *d_cc_stats;       // ClassPlan::stats (the sixteen words behind d_counters' sixteen: four of the cache, five of the refinement)
    unsigned long long cc_classified_host;  // frames of chains in which no frame used the cache: their kernels are the plain ones and do not count
    tl3d::PrepChain pend;                 // the batch being collected (tl3d_integrate fills slot, pose, scale, depth and depth_u16; the rest is flush_updates')
    tl3d::CenFrame cen_pend[tl3d::TL3D_CEN_MAXBATCH];   // voxel-centroid accumulations not yet launched (one stride per batch)
    int n_cen_pend = 0;
    tl3d::CenFrame *d_cen_frames = nullptr;              // their descriptors on the device
    int n_pend;                           // frames of the batch being collected
    unsigned long long grid_epoch;        // bumped by every call that changes a grid or hands out a pointer into one (see ext_epoch / mesh_epoch)
    // tl3d_raycast: device staging of the outputs a caller wants on the host ([H][W] f32, [H][W][3] f32, [H][W][3] u8; grown on demand)
    float *ray_depth, *ray_nrm;
    uint8_t *ray_bgr;
    unsigned long long *bp_state;        // one-launch back-projection: ticket, error word, per-tile granules, [bp_state_words - 1] = total
    size_t bp_state_words;
    float *bp_stage_xyz;                 // staging for host-side outputs, sized for a full frame at subsample 1
    uint8_t *bp_stage_rgb;
    bool bp_async_pending;
    double *bp_factors;                  // projection factors (D2R:287-295): [0, W) xf[u] = (u - cx) / fx, [W, W + H) yf[v] = (v - cy) / fy
    hipEvent_t ev_free;                   // recorded on the main stream behind its last write to free_cnt (clear, fold); prep chains wait for it
    bool ev_free_recorded;
    int tsdf_max_blocks;                  // launch geometry of the update kernel (32 workgroups per CU)
    bool tsdf_single_stream;
    void *rccl_comm;             // ncclComm_t of tl3d_rccl_init (RCCL is dlopen'ed: tl3d_api.hip)
    int rccl_world;
    int *d_maxw;
    unsigned long long *d_counters;   // device counters [16]
    unsigned long long *d_cen_counters;   // centroid statistics, sharded: [256 lines][8] (points kept, points dropped)
    struct IcpLane {             // one in-flight ICP run: own stream, device state, partial-sum slab, pinned read-back (api_register.hip, as the next three)
        hipStream_t stream;
        double *slab;            // [ICP_MAX_BLOCKS][ICP_SLAB]
        unsigned *ticket;        // arrival counter of the iteration kernel (64-B block of its own; 0 between launches)
        tl3d::IcpState *state;
        tl3d::IcpState *host;    // pinned: initial state in, final state out
        tl3d::IcpRun *run;       // device descriptor of the current run
        tl3d::IcpRun *run_host;  // pinned
        // captured chains: descriptor + state upload, ticket re-arm, (iters+1) iteration kernels, state download -- one per
        // iteration count used lately (a coarse-to-fine caller alternates between two or three)
        hipGraphExec_t graphs[4];
        int graph_iters[4];
        int graph_next;          // slot the next new iteration count replaces
        bool busy;               // a run was enqueued and not collected yet
        hipEvent_t ev_done;      // recorded on the lane's stream behind the run: writers of the slots it reads wait on it
        int src_slot, tgt_slot;  // the run reads slots[src].depth and slots[tgt].nmap
    };
    IcpLane icp_lanes[TL3D_ICP_LANES];
    struct IcpBatch {            // one batch of registrations in flight, on its own stream
        hipStream_t stream;
        hipEvent_t ev_ready, ev_done;
        int cap_pairs; size_t cap_slab;          // capacities of the buffers below
        int sync_rows;                           // geometry of `sync` (see IcpBatchArgs)
        tl3d::IcpBatchPair *pairs, *pairs_host;  // device / pinned
        tl3d::IcpState *states, *states_host;
        unsigned *sync, *ctl, *ctl_host;
        double *slab;
        int n_pairs;             // of the run in flight
        tl3d_icp_pair *req_pairs;                // the request as the caller made it: the fallback of a timed-out launch re-registers from it
        int req_cap, req_n_levels;
        tl3d_icp_params req_levels[TL3D_ICP_MAX_LEVELS];
        unsigned *stage; size_t stage_n;  // experiments (TL3D_ICP_STAGES)
        unsigned long long *dbg; // experiments (TL3D_ICP_TRACE)
        int dbg_members;
        bool busy;
    } icp_batch;
    struct IcpEval {             // tl3d_icp_evaluate_pairs: device buffers of one chunk of pairs (main stream), grown on demand
        tl3d::IcpEvalPair *pairs;
        double *slab;                            // [pairs][members][ICP_EVAL_SUMS] partials
        double (*sums)[tl3d::ICP_EVAL_SUMS];     // [pairs] totals
        size_t cap_pairs, cap_slab;              // of pairs and sums, in pairs; of slab, in doubles
    } icp_eval;
    struct Track {               // tl3d_track_*: device state, partial-sum slab, pinned state for the way in and out (main stream)
        tl3d::IcpState *state, *host;
        double *slab;            // [track_members][TRACK_SUMS]
    } track;
    struct Rgbd {                // tl3d_rgbd_*: device buffers of one chunk of pairs (main stream), grown on demand
        tl3d::RgbdPair *pairs;
        tl3d::RgbdState *states;
        size_t cap_pairs;        // of pairs and states
        double *slab;            // [pairs][members][RGBD_SUMS] partials of the current pass
        size_t cap_slab;         // in doubles
    } rgbd;
    struct Cloud {               // tl3d_cloud_*: device state and its pinned copy for the way in and out (main stream)
        tl3d::IcpState *state, *host;
    } cloud;
    float *bounds_slab;
    bool nn_input_order;         // tl3d_set_nearest_query_order(ctx, 0): nearest-neighbour queries run in input order, not bucketed by cell
    // stats / profiling
    tl3d_stats stats;
    bool count_records, time_kernels;
    hipEvent_t ev[2];
    struct KTimer { hipEvent_t a, b; int launches; };   // one event pair around `launches` back-to-back update kernels
    KTimer *ktimers;
    int n_ktimers, ktimers_used;
};

namespace tl3d {

int set_err(int code, const char *fmt, ...);

#define TL3D_HIP(x)                                                                          \
    do {                                                                                     \
        hipError_t e__ = (x);                                                                \
        if (e__ != hipSuccess) return tl3d::set_err(TL3D_E_HIP, "%s failed: %s (%s:%d)", #x, \
                                                    hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

// ---- device helpers ---------------------------------------------------------------------------
__device__ __forceinline__ size_t brick_base(int bx, int by, int bz, int nbx, int nby) {
    return (((size_t)bz * (size_t)nby + (size_t)by) * (size_t)nbx + (size_t)bx) << 9;
}
// Record order inside a brick: eight 4x4x4 sub-bricks (sub-brick = x >> 2 | (y >> 2) << 1 | (z >> 2) << 2) of 64 contiguous records
// each, x fastest inside a sub-brick.  A sub-brick is the unit the TSDF update classifies and touches: 64 records = one 8-B-per-lane
// access of a wave = 512 contiguous bytes of the TSDF channel (2 KB of the centroid channel).
__host__ __device__ __forceinline__ int in_brick_index(int i, int j, int k) {
    return ((k & 4) << 6) | ((j & 4) << 5) | ((i & 4) << 4) | ((k & 3) << 4) | ((j & 3) << 2) | (i & 3);
}
__host__ __device__ __forceinline__ void in_brick_coords(int l, int &i, int &j, int &k) {
    i = ((l >> 4) & 4) | (l & 3);
    j = ((l >> 5) & 4) | ((l >> 2) & 3);
    k = ((l >> 6) & 4) | ((l >> 4) & 3);
}
__device__ __forceinline__ size_t vox_index(int i, int j, int k, int nbx, int nby) {
    return brick_base(i >> 3, j >> 3, k >> 3, nbx, nby) + (size_t)in_brick_index(i, j, k);
}

// coordinates of virtual record index idx (brick-major, in-brick order above); extraction and mesh kernels
__device__ __forceinline__ void rec_coords(size_t idx, int nbx, int nby, int &i, int &j, int &k) {
    const size_t b = idx >> 9;
    const int l = (int)(idx & 511);
    const int bx = (int)(b % (size_t)nbx), by = (int)((b / (size_t)nbx) % (size_t)nby);
    const int bz = (int)(b / ((size_t)nbx * (size_t)nby));
    in_brick_coords(l, i, j, k);
    i |= bx << 3;
    j |= by << 3;
    k |= bz << 3;
}

__host__ __device__ __forceinline__ bool in_core(const Grid &g, int i, int j, int k) {
    return i >= g.clo[0] && i < g.chi[0] && j >= g.clo[1] && j < g.chi[1] && k >= g.clo[2] && k < g.chi[2];
}

__device__ __forceinline__ void mean_colour(const unsigned long long *__restrict__ rec, unsigned long long n, uint8_t c[3]) {
    c[0] = (uint8_t)((rec[2] & 0xffffffffull) / n);
    c[1] = (uint8_t)((rec[2] >> 32) / n);
    c[2] = (uint8_t)((rec[3] & 0xffffffffull) / n);
}

// ---- brick tables ---------------------------------------------------------------------------------------------------------
// The table is read and written by kernels that run side by side: agent-scope accesses only (a CU's L1 would go on showing
// SLOT_EMPTY after another CU -- or this one, through the L2 -- filled the entry, and every such stale read would take, and
// leak, a fresh slot).
__device__ __forceinline__ unsigned brick_slot(const unsigned *table, unsigned brick) {
    return __hip_atomic_load(table + brick, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Slot of `brick`, handing one out on first touch -- exactly one per brick: the wave that turns the entry from EMPTY to PENDING
// draws the slot and publishes it; a wave that finds PENDING waits for that store (the drawing wave waits for nobody: an atomic add
// and a store, so the wait ends; it is bounded all the same -- ~30 ms -- and then gives up as if the pool were full, counted).
// Until round 3 every contender drew a slot and the losers of the compare-and-swap lost theirs to the pool: with 32 frames per
// accumulation launch, first touches of one brick by a dozen workgroups at once, a tenth of the centroid pool leaked, and a pool
// sized by a count (tl3d_count_bricks) must not leak.  SLOT_FULL when the pool is exhausted (sticky: later touches see it).
__device__ __forceinline__ unsigned brick_slot_ensure(unsigned *table, unsigned *cursor, unsigned cap, unsigned brick) {
    for (unsigned spin = 0; spin < (1u << 20); ++spin) {
        const unsigned s = brick_slot(table, brick);
        if (s < SLOT_PENDING) return s;                            // a slot, or SLOT_FULL
        if (s == SLOT_EMPTY) {
            const unsigned old = atomicCAS(table + brick, SLOT_EMPTY, SLOT_PENDING);
            if (old == SLOT_EMPTY) {
                unsigned n = atomicAdd(cursor, 1u);
                if (n >= cap) {
                    n = SLOT_FULL;
                    atomicAdd(cursor + 1, 1u);
                }
                __hip_atomic_store(table + brick, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return n;
            }
            if (old < SLOT_PENDING) return old;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    atomicAdd(cursor + 1, 1u);
    return SLOT_FULL;
}
// the same for every lane of a wave at once (want: the lane needs its brick's slot): one leader per distinct brick draws, the
// lanes that share the brick take its answer.  Every lane of the wave must call it.
__device__ __forceinline__ unsigned wave_slots(unsigned *table, unsigned *cursor, unsigned cap, unsigned brick, bool want) {
    unsigned slot = want ? brick_slot(table, brick) : 0u;          // the common case: every brick has its slot already
    unsigned long long todo = __ballot(want && slot >= SLOT_PENDING);
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const unsigned b = (unsigned)__builtin_amdgcn_readlane((int)brick, leader);
        unsigned s = 0;
        if ((threadIdx.x & 63) == leader) s = brick_slot_ensure(table, cursor, cap, b);
        s = (unsigned)__builtin_amdgcn_readlane((int)s, leader);
        const bool mine = want && slot >= SLOT_PENDING && brick == b;
        todo &= ~__ballot(mine);
        if (mine) slot = s;
    }
    return slot;
}
// TSDF record of virtual record index idx as a reader must see it: the stored sums plus the brick's pending free-space count
// (count x (32767, 1)); a brick without records reads as free space only
__device__ __forceinline__ int2 tsdf_record(const Grid &g, const int2 *__restrict__ pool, size_t idx) {
    const unsigned brick = (unsigned)(idx >> 9);
    const unsigned s = brick_slot(g.tsdf_tab, brick);
    int2 r = make_int2(0, 0);
    if (s < SLOT_FULL) r = pool[((size_t)s << 9) | (idx & 511)];
    if (g.free_cnt) {
        const unsigned c = g.free_cnt[brick];
        r.x += (int)(c * 32767u);
        r.y += (int)c;
    }
    return r;
}
// centroid record (4 words) of virtual record index idx, nullptr when its brick has none
__device__ __forceinline__ const unsigned long long *cen_record(const Grid &g, const unsigned long long *__restrict__ pool, size_t idx) {
    const unsigned s = brick_slot(g.cen_tab, (unsigned)(idx >> 9));
    return s < SLOT_FULL ? pool + 4 * (((size_t)s << 9) | (idx & 511)) : nullptr;
}

// ---- kernel launchers (one per .hip file) -----------------------------------------------------
// frames
int launch_u16_to_f32(hipStream_t s, const uint16_t *in, float *out, size_t n);
// compaction (kernels_compact.hip; the device half is compact.h)
int launch_scan(hipStream_t s, const unsigned *counts, unsigned long long *offsets, int n, unsigned long long *total);
int launch_scan(hipStream_t s, const unsigned long long *counts, unsigned long long *offsets, int n, unsigned long long *total);
// back-projection
int launch_bp_bounds(hipStream_t s, const Cam &cam, const BpArgs &a, const PoseD &p, const float *depth, const double *xf, const double *yf,
                     float *slab, int nblocks);
int bp_fused_tiles(const BpArgs &a);
int bp_state_words(const BpArgs &a);
int launch_bp_fused(hipStream_t s, const Cam &cam, const BpArgs &a, const PoseD &p, const float *depth, const uint8_t *bgr,
                    const double *xf, const double *yf, unsigned long long *state, float *xyz, uint8_t *rgb, unsigned long long cap,
                    unsigned long long *total_out, bool force_dynamic = false);
// centroid
int launch_centroid_batch(hipStream_t s, const Cam &cam, const Grid &g, int n, const CenFrame *host, CenFrame *dev, const double *xf, const double *yf,
                          unsigned long long *grid, unsigned long long *counters);
int launch_centroid_points(hipStream_t s, const Grid &g, const float *xyz, const uint8_t *rgb, long long n,
                           unsigned long long *grid, unsigned long long *counters);
int launch_bounds(hipStream_t s, const float *xyz, long long n, float *slab, int nblocks);
// tsdf
size_t tsdf_batch_scratch_bytes(const Cam &cam, const Grid &g, int max_frames);
void tsdf_batch_scratch_zero_range(const Cam &cam, const Grid &g, int max_frames, size_t *off, size_t *bytes);
int launch_tsdf_prepare(hipStream_t s, const Cam &cam, const Grid &g, const Frustum &fr, const PrepChain &c, int max_frames, void *scratch,
                        unsigned *free_cnt, bool classify_only);
size_t tsdf_tile_cache_bytes(const Cam &cam, size_t *vtile_off, size_t *vpix_off);
size_t tsdf_class_cache_bytes(unsigned entries);
int launch_centroid_mark(hipStream_t s, const Cam &cam, const Grid &g, const BpArgs &a, const PoseD &p, const float *depth, const double *xf, const double *yf);
#ifdef TL3D_EXPERIMENTS
void tsdf_debug_print_spans(int nwaves, int late_from);
#endif
int launch_tsdf_update(hipStream_t s, const Cam &cam, const Grid &g, int n, int max_frames, bool depth_u16, float mind, float maxd, int2 *grid,
                       void *scratch, unsigned long long *counters, bool count, int max_blocks);
int launch_fold_free(hipStream_t s, const Grid &g, int2 *grid, unsigned *free_cnt);
// normals + icp
int launch_nmap_rowmajor(hipStream_t s, const Cam &cam, const float4 *nmap, float4 *out);
int launch_normals(hipStream_t s, const Cam &cam, const float *depth, float scale, float mind, float maxd, float jump, int radius, float *sdepth,
                   float4 *nmap);
int launch_icp_batch(hipStream_t s, const Cam &cam, const IcpBatchArgs &a);
int launch_icp_iteration(hipStream_t s, const Cam &cam, const IcpRun *run, int final_pass, double *slab, IcpState *state, int nblocks,
                         unsigned *ticket);
int icp_eval_members(int Ws, int Hs);
int launch_icp_eval(hipStream_t s, const Cam &cam, const IcpEvalPair *pairs, int n_pairs, int members, float mind, float maxd, float md2, int stride,
                    int Ws, int Hs, double *slab, double *out);
// tracking against the TSDF (kernels_track.hip: the pass; kernels_regstep.hip: the step)
int track_members(int Ws, int Hs);
int launch_track_pass(hipStream_t s, const Cam &cam, const Grid &g, const float *depth, float scale, float mind, float maxd, int min_weight,
                      int stride, double max_dist, const int2 *tsdf, const IcpState *state, StepKind kind, double *slab);
int launch_track_step(hipStream_t s, const double *slab, int members, IcpState *state, double damping, double eps, double eig_rel, StepKind kind);
// joint point-to-plane + photometric registration (kernels_rgbd.hip: the intensity maps and the pass; kernels_regstep.hip: the step)
int launch_intensity(hipStream_t s, const Cam &cam, const float *depth, const uint8_t *bgr, int radius, float jump, float4 *imap);
int rgbd_members(int Ws, int Hs);
int launch_rgbd_pass(hipStream_t s, const Cam &cam, const RgbdPair *pairs, int n_pairs, const RgbdLevel &L, const RgbdState *states,
                     StepKind kind, double *slab);
int launch_rgbd_step(hipStream_t s, const double *slab, int n_pairs, int members, RgbdState *states, double photo_weight, double damping,
                     double eps, double eig_rel, StepKind kind);
// extraction
int launch_extract_count(hipStream_t s, const Grid &g, int mode, int min_count, int min_weight, double max_abs,
                         const int2 *tsdf, const unsigned long long *cen, unsigned *block_counts, int nblocks);
int launch_extract_write(hipStream_t s, const Grid &g, int mode, int min_count, int min_weight, double max_abs,
                         const int2 *tsdf, const unsigned long long *cen, const unsigned long long *offsets, int nblocks,
                         float *xyz, uint8_t *rgb, unsigned long long cap);
// mesh
int launch_mesh_count(hipStream_t s, const Grid &g, int min_weight, const int2 *tsdf, unsigned *vcounts, unsigned *tcounts,
                      int nblocks);
int launch_mesh_write(hipStream_t s, const Grid &g, int min_weight, const int2 *tsdf, const unsigned long long *cen,
                      const unsigned long long *voffsets, const unsigned long long *toffsets, int nblocks, unsigned *first_id,
                      float *xyz, uint8_t *rgb, unsigned long long vcap, unsigned *tris, unsigned long long tcap,
                      long long *keys = nullptr, const long long *lat = nullptr);
// ray casting
int launch_raycast(hipStream_t s, const Cam &cam, const Grid &g, const double R[9], const double t[3], int min_weight, float z_near,
                   float z_far, const int2 *tsdf, const unsigned long long *cen, float *depth, float *depth2, float *nrm, uint8_t *bgr,
                   uint8_t *bgr2);
// grids
int launch_max_weight(hipStream_t s, const Grid &g, const int2 *pool, int *d_out);
int launch_max_weight_dense(hipStream_t s, const int2 *grid, size_t nvox, int *d_out);
int launch_touched_bricks(hipStream_t s, const Grid &g, const int2 *tsdf, const unsigned long long *cen, unsigned nbricks, unsigned char *map, bool sub = false);
int launch_brick_rows(hipStream_t s, const Grid &g, int mode, bool is_tsdf, void *pool, const unsigned *idx, long long n, void *rows, bool add_free, bool sub = false);
int launch_iota(hipStream_t s, unsigned *t, unsigned n);
int probe_hw_queues(int n_streams, double spin_ms, double *elapsed_ms);
int launch_add_i32(hipStream_t s, int *dst, const int *src, size_t n);
int launch_add_u64(hipStream_t s, unsigned long long *dst, const unsigned long long *src, size_t n);
// mesh components (kernels_meshcc.hip)
int launch_cc_validate(hipStream_t s, const unsigned *tri, long long n_tri, unsigned long long *info);
int launch_cc_label(hipStream_t s, const unsigned *tri, long long n_tri, long long n_vert, unsigned *parent, unsigned *count,
                    unsigned long long *info);
int launch_cc_keep_count(hipStream_t s, long long min_tri, int largest, const unsigned *tri, long long n_tri, long long n_vert,
                         const unsigned *label, const unsigned *count, unsigned *vcounts, unsigned *tcounts, uint8_t *keep_out,
                         unsigned long long *info);
int launch_cc_compact(hipStream_t s, long long min_tri, int largest, const unsigned *tri, long long n_tri, long long n_vert,
                      const unsigned *label, const unsigned *count, const unsigned long long *voffsets, const unsigned long long *toffsets,
                      const float *xyz, const uint8_t *rgb, float *out_xyz, uint8_t *out_rgb, unsigned long long vcap, unsigned *out_tri,
                      unsigned long long tcap, unsigned *remap, const unsigned long long *info);
// vertex clustering (kernels_meshsimplify.hip)
int launch_ms_validate(hipStream_t s, double cell, const double o[3], const float *xyz, long long n_vert, unsigned long long *info);
int launch_ms_cluster(hipStream_t s, double cell, const double o[3], const float *xyz, const uint8_t *rgb, long long n_vert,
                      unsigned long long *keys, unsigned *leader, unsigned long long vcap, unsigned *slot, unsigned *vmap,
                      unsigned long long *acc, unsigned *vcounts, unsigned long long *voffsets);
int launch_ms_quadrics(hipStream_t s, double cell, const double o[3], const float *xyz, const unsigned *tri, long long n_tri,
                       const unsigned *vmap, unsigned long long *qacc, unsigned long long *info);
int launch_ms_triangles(hipStream_t s, const unsigned *tri, long long n_tri, const unsigned *vmap, unsigned *ttab, unsigned long long tcap,
                        uint8_t *flag, unsigned *tcounts, unsigned long long *toffsets, unsigned long long *info);
int launch_ms_write(hipStream_t s, double cell, const double o[3], const float *xyz, bool colours, long long n_vert, const unsigned *slot,
                    const unsigned *leader, const unsigned *vmap, const unsigned long long *acc, float *out_xyz, uint8_t *out_rgb,
                    unsigned long long vcap, const unsigned *tri, long long n_tri, const uint8_t *flag, const unsigned long long *toffsets,
                    unsigned *out_tri, unsigned long long tcap, const unsigned long long *qacc = nullptr, double reg = 0.0,
                    unsigned long long *info = nullptr);
// the uniform cell index (kernels_cellgrid.hip; the device half is cellgrid.h)
struct CellGrid;
constexpr size_t CELL_SLAB_BYTES = 128 << 10;
inline size_t cell_chunks(long long ncell) { return (size_t)((ncell + 1023) / 1024); }
bool cell_grid_make(const double mn[3], const double mx[3], double cell, CellGrid *g);
void cell_grid_fit(const double mn[3], const double mx[3], double cell, CellGrid *g);
void launch_cell_count(hipStream_t s, const CellGrid &g, const float *xyz, long long n, unsigned *cnt);
int launch_cell_scan(hipStream_t s, const unsigned *cnt, long long ncell, unsigned *chunk_sums, unsigned long long *chunk_off, unsigned *start);
int cell_slab(tl3d_ctx *ctx);
// The four tables of one index (cell_index_build, cellgrid.h), in the order a caller appends their sizes to its own carve list:
// cnt[ncell] (zero in front of a count and again behind the fill), start[ncell + 1], and the scan's chunk sums and offsets.
struct CellTables {
    unsigned *cnt, *start, *chunk_sums;
    unsigned long long *chunk_off;
    static CellTables at(void *const p[4]) { return {(unsigned *)p[0], (unsigned *)p[1], (unsigned *)p[2], (unsigned long long *)p[3]}; }
};
inline void cell_table_bytes(long long ncell, size_t bytes[4]) {
    bytes[0] = (size_t)ncell * sizeof(unsigned);
    bytes[1] = (size_t)(ncell + 1) * sizeof(unsigned);
    bytes[2] = cell_chunks(ncell) * sizeof(unsigned);
    bytes[3] = (cell_chunks(ncell) + 1) * sizeof(unsigned long long);
}
// The first step of every build: the box of a device list's finite points and the number of points with a non-finite coordinate.
// points_bounds_finite is the whole pass (waits for the stream).  The searches run it for two lists under one wait: nn_bounds_launch
// leaves a list's block partials (nn_red_blocks(n) x 8 floats) in the slab, nn_bounds_fold folds their host copy and returns the count.
constexpr int NN_RED = 1024;            // blocks of the reductions (fixed: the partial sums do not depend on the device)
unsigned nn_red_blocks(long long n);
void nn_bounds_launch(hipStream_t s, const float *xyz_dev, long long n, float *slab);
unsigned long long nn_bounds_fold(const float *h, long long n, double mn[3], double mx[3]);
int points_bounds_finite(tl3d_ctx *ctx, const float *xyz_dev, long long n, double mn[3], double mx[3], unsigned long long *bad);
// outlier filter (kernels_sor.hip): the k-NN mean-distance stage alone (*mean_dev: n doubles, or null: carved with the call's scratch
// and returned), and the whole filter, which thresholds it
int sor_mean_distance(tl3d_ctx *ctx, const float *xyz_dev, long long n, int k, double cell, double **mean_dev);
int sor_run(tl3d_ctx *ctx, const float *xyz_dev, long long n, int k, double std_ratio, double cell, uint8_t *keep_dev, long long *kept);

// nearest neighbours from one set to another and the distance summary (kernels_nearest.hip); device pointers, outputs may be null
int nearest_points_run(tl3d_ctx *ctx, const float *query, long long nq, const float *target, long long nt, double cell, double max_dist,
                       double *dist, int *index);
int nearest_triangles_run(tl3d_ctx *ctx, const float *query, long long nq, const float *xyz, long long nv, const unsigned *tri, long long n_tri,
                          double cell, double max_dist, double *dist, int *index);
int distance_summary_run(tl3d_ctx *ctx, const double *dist, long long n, const double *thresholds, int nthr, tl3d_distance_stats *out);
double nn_default_cell_points(const double mn[3], const double mx[3], long long n);

// registration of two point clouds (kernels_cloudicp.hip; the step kernel is kernels_regstep.hip's): device pointers; the run starts at
// the pose in *state (device memory) and leaves its result there, enqueued on the context's stream behind one wait for the bounds
constexpr int CLOUD_SUMS = 40;           // doubles per block partial: IcpState::sums, [30] the correspondences dropped for a zero normal
constexpr int CLOUD_SUM_NO_NORMAL = 30;
int cloud_members(long long n_src);
int cloud_icp_run(tl3d_ctx *ctx, const float *src, long long n_src, const float *tgt, long long n_tgt, const float *tgt_normals,
                  const tl3d_icp_params *levels, int n_levels, bool evaluate, double cell, IcpState *state, int *index_out);
int launch_cloud_step(hipStream_t s, const double *slab, int members, IcpState *state, int est_scale, double damping, double eps,
                      double eig_rel, StepKind kind);

// normals and surface variation by k-NN PCA (kernels_normals.hip); device pointers but the viewpoints (host), curvature may be null
int normals_run(tl3d_ctx *ctx, const float *xyz, long long n, int k, double max_radius, double cell, const double *vp_host, long long n_vp,
                float *normal, float *curvature, long long *degenerate);

// global registration (kernels_cloudglobal.hip): device pointers but the RANSAC's params and result (host).  slots: kt_slots(n).
int voxel_subsample_run(tl3d_ctx *ctx, const float *xyz, long long n, double voxel, size_t slots, int *index_out, long long *kept);
int fpfh_run(tl3d_ctx *ctx, const float *xyz, const float *nrm, long long n, int k, double max_radius, double cell, float *fpfh_out, int *spfh_out);
int feature_match_run(tl3d_ctx *ctx, const float *fa, long long na, const float *fb, long long nb, int dim, int *index_out, double *dist2_out);
int ransac_run(tl3d_ctx *ctx, const float *src, long long n_src, const float *tgt, long long n_tgt, const int *corr, long long m,
               const tl3d_ransac_params &prm, tl3d_ransac_result *out, int *count_out);

// planar regions of a cloud (kernels_planes.hip); device pointers but planes_hd (host or device) and counts (host); curvature may be null
int planes_run(tl3d_ctx *ctx, const float *xyz, const float *nrm, const float *curv, long long n, const tl3d_plane_params &prm, double cell,
               int *plane_id, tl3d_plane *planes_hd, long long plane_cap, long long counts[4], bool *short_cap);

// depth-image filter (kernels_depthfilter.hip): n images of the context's W x H, filtered in place on its stream; device pointers but
// counts (host, [n][4], may be null: then the call does not wait); f32[i] is a u16 image's f32 copy to zero with it, or null
constexpr int DF_MAXBATCH = 16;      // frames that may share a launch (blockIdx.z)
int depth_filter_run(tl3d_ctx *ctx, int n, void *const *img, float *const *f32, const int *kinds, const tl3d_depth_filter_params &prm,
                     long long *counts);

// mesh smoothing and vertex normals (kernels_meshsmooth.hip)
int launch_msm_validate(hipStream_t s, const float *xyz, long long n_vert, unsigned long long *info);
int launch_msm_edges(hipStream_t s, const unsigned *tri, long long n_tri, unsigned long long *keys, unsigned long long slots, unsigned *deg,
                     unsigned long long *info);
int launch_msm_rows(hipStream_t s, const unsigned *cnt, long long n_vert, unsigned long long *ccounts, unsigned long long *coffs,
                    unsigned long long *row, unsigned *cursor);
int launch_msm_edge_fill(hipStream_t s, const unsigned long long *keys, unsigned long long slots, const unsigned *deg,
                         const unsigned long long *row, unsigned *cursor, unsigned *nbr);
int launch_msm_step(hipStream_t s, const float *in, float *out, long long n_vert, const unsigned *deg, const unsigned long long *row,
                    const unsigned *nbr, double factor, const unsigned long long *flag_in, unsigned long long *flag_out);
int launch_msm_corners(hipStream_t s, const unsigned *tri, long long n_tri, long long n_vert, unsigned *cnt, unsigned long long *ccounts,
                       unsigned long long *coffs, unsigned long long *row, unsigned *cursor, unsigned *inc);
int launch_msm_normals(hipStream_t s, const float *xyz, const unsigned *tri, long long n_vert, const unsigned *cnt, const unsigned long long *row,
                       const unsigned *inc, float *out, unsigned long long *info);

// mesh weld (kernels_meshweld.hip)
int launch_wm_validate(hipStream_t s, const WeldPart *parts, int n_parts, unsigned long long n_vert, unsigned long long n_tri,
                       unsigned long long key_end, unsigned long long *info);
int launch_wm_own_count(hipStream_t s, const WeldPart *parts, int n_parts, unsigned long long n_vert, const long long lat[3], unsigned *counts,
                        unsigned long long *offsets);
int launch_wm_own_write(hipStream_t s, const WeldPart *parts, int n_parts, unsigned long long n_vert, const long long lat[3],
                        const unsigned long long *offsets, float *out_xyz, uint8_t *out_rgb, long long *out_key, unsigned long long vcap,
                        unsigned *vert_map, unsigned long long *keys, unsigned *vals, unsigned long long slots, unsigned long long *info);
int launch_wm_resolve(hipStream_t s, const WeldPart *parts, int n_parts, unsigned long long n_tri, const unsigned *vert_map,
                      const unsigned long long *keys, const unsigned *vals, unsigned long long slots, unsigned *out_tri, unsigned long long *info);

constexpr int EXTRACT_CHUNK = 2048;   // elements per block in the compaction passes (compact.h)
inline unsigned blocks_of(unsigned long long n, unsigned per) { return (unsigned)((n + per - 1) / per); }
inline int chunks_of(unsigned long long n) { return (int)blocks_of(n, EXTRACT_CHUNK); }

}  // namespace tl3d
