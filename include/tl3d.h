/*
 * tl3d.h -- C-ABI of the MI355X depth-fusion back end (libtl3d.so).
 *
 * The reference (kamalnath26/textureless-3d-reconstruction) is pure Python and has no FFI of its
 * own; the seam this library sits under is the Python method surface of its dense back end
 * (SURVEY.md section 8b).  Each entry point below names the reference code it replaces
 * (file:line relative to the reference checkout).  INTEGRATION.md shows the ctypes stubs a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns int: 0 = TL3D_OK, negative = error; no exception crosses the boundary;
 *     tl3d_last_error() returns a thread-local message for the last failing call.
 *   - the caller owns every host buffer it passes in or out for the duration of the call; the library
 *     owns all device memory inside a tl3d_ctx.  "hd" pointers may be host OR device pointers
 *     (copied with hipMemcpyDefault).
 *   - arrays are C-contiguous row-major: depth [H][W], bgr [H][W][3], poses fp64 row-major.
 *   - a pose is world->camera  X_cam = R X_world + t  (depth_to_reconstruction.py:373-376, 543-546).
 *   - one tl3d_ctx per GPU per process; a ctx is not thread-safe; calls enqueue on the ctx's HIP
 *     stream and return, every call with a host output blocks until that output is ready.
 */
#ifndef TL3D_H
#define TL3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TL3D_ABI_VERSION 5

/* error codes */
#define TL3D_OK 0
#define TL3D_E_INVALID (-1)     /* bad argument / shape / slot                       */
#define TL3D_E_HIP (-2)         /* a HIP runtime call failed                         */
#define TL3D_E_NOMEM (-3)       /* device allocation failed                          */
#define TL3D_E_CAPACITY (-4)    /* output buffer too small; *out_n holds the need    */
#define TL3D_E_STATE (-5)       /* call not valid in this state (channel disabled..) */
#define TL3D_E_NODEVICE (-6)    /* no usable GPU                                     */

/* grid channels */
#define TL3D_CH_TSDF 1u         /* {int32 sum of quantised tsdf, int32 weight}         8 B/voxel  */
#define TL3D_CH_CENTROID 2u     /* {sx|sy<<32, sz|n<<32, sr|sg<<32, sb} u64 x4         32 B/voxel */
#define TL3D_CH_FREE 4u         /* the per-brick free-space counts (uint32 [nx ny nz / 512]; tl3d_integrate).  tl3d_grid_device_ptr: the
                                   counts as they stand, pending ones included -- a merge sums them like records (afterwards they are
                                   pending on every rank and fold into the records at the next read).  OR-ed into the channel mask
                                   of tl3d_grid_touched_bricks / _pack_bricks / _unpack_bricks: pending counts stay pending and mark
                                   no brick, i.e. the free-space observations travel as 4 bytes per brick, not as 4 KB of records */
#define TL3D_CH_SUB 8u          /* with the merge helpers below: the unit is a 4x4x4 SUB-BRICK (64 contiguous records), ids = brick * 8 + sub-brick */

/* fixed-point formats of the accumulators (exact, order-free sums => bit-identical multi-GPU merge) */
#define TL3D_TSDF_QSCALE 32767          /* tsdf in [-1,1] -> rint(tsdf * 32767)                  */
#define TL3D_TSDF_MAX_WEIGHT 65536      /* observations one voxel may hold: |sum| <= weight * 32767 < 2^31.  Free-space
                                           voxels seen by every camera reach it first.  tl3d_integrate and tl3d_grid_add
                                           return TL3D_E_STATE instead of wrapping; a merge done outside the library
                                           (all-reduce on tl3d_grid_device_ptr memory) must check the sum of the ranks'
                                           tl3d_grid_max_weight itself (tl3d.distributed does).  The centroid channel's
                                           limit is 2^20 points per voxel.                                        */
#define TL3D_CENTROID_FRAC_BITS 12      /* in-voxel offset in units of voxel/4096                */
#define TL3D_BRICK 8                    /* grid is stored brick-major, 8x8x8 voxels per brick    */

/* depth upload kinds (depth_to_reconstruction.py:80-97) */
#define TL3D_DEPTH_F32_M 0      /* float32 metres (or relative units), as np.load().astype(f32) */
#define TL3D_DEPTH_U16_MM 1     /* uint16 millimetres; converted on device as f32(u16)/1000.0f  */

/* flags of tl3d_backproject / tl3d_accumulate_centroid */
#define TL3D_F_SCALE_F64 1u     /* depth*scale and the range compares run in fp64 (numpy-2 promotion when
                                   `scale` is an np.float64: depth_to_reconstruction.py:356 with :323) */
#define TL3D_F_NO_POSE 2u       /* pose=None: points stay in the camera frame (D2R:377-378)            */

/* extraction modes */
#define TL3D_EXTRACT_CENTROID 0 /* one point per occupied voxel = centroid (Open3D voxel_down_sample)   */
#define TL3D_EXTRACT_TSDF 1     /* zero crossings of the TSDF along +x,+y,+z edges                      */

typedef struct tl3d_ctx tl3d_ctx;

/* Replaces ReconstructionConfig (depth_to_reconstruction.py:45-73) and CameraIntrinsics
 * (depth_enhanced_reconstruction.py:57-80) for the device path, plus the grid geometry. */
typedef struct tl3d_config {
    int32_t abi_version;        /* = TL3D_ABI_VERSION                                              */
    int32_t width, height;      /* W, H of every frame of this ctx                                 */
    double fx, fy, cx, cy;      /* intrinsics; pixel centres sit on integer (u,v) (D2R:291-293)    */
    double min_depth, max_depth;/* strict validity range (D2R:359-361); 0.1/50 D2R, 0.1/100 DER    */
    int32_t n_slots;            /* resident frame slots                                            */
    uint32_t channels;          /* TL3D_CH_* bit mask; 0 = no grid (back-projection / ICP only)    */
    int32_t nx, ny, nz;         /* voxels per axis, multiples of TL3D_BRICK                        */
    double origin[3];           /* world position of the min corner of voxel (0,0,0)               */
    double voxel_size;          /* metres (D2R:64: 0.005)                                          */
    double sdf_trunc;           /* metres                                                          */
    void *ext_tsdf;             /* optional caller-owned device memory for the grids (e.g. a torch */
    void *ext_centroid;         /*   tensor's data_ptr, so torch.distributed can all-reduce it)    */
    void *stream;               /* optional hipStream_t to enqueue on; NULL = library-owned stream */
    int64_t pool_bricks_tsdf;   /* SPARSE grid: the channel holds records for at most this many 8^3 bricks (4 KB each), handed out */
    int64_t pool_bricks_centroid; /* on first touch through a brick table; 0 = dense (every brick has records, 16 KB each for the
                                   centroid channel).  What the reference's hash-map merge gives for free (any extent at any voxel
                                   size, D2R:404-410): nx ny nz may describe a volume far larger than memory.  Bricks that are only
                                   ever free space hold a 4-byte count, no records.  When the pool runs out further new bricks are
                                   refused and counted (tl3d_stats.pool_refused): nothing is written out of bounds.             */
    int64_t voxel_offset[3];    /* the grid is a BLOCK of a larger voxel lattice: its voxel (0,0,0) is voxel voxel_offset of the lattice that
                                   starts at `origin` (multiples of TL3D_BRICK).  Voxel indices are computed against `origin` as ever (Open3D:
                                   floor((p - origin) / voxel), D2R:404-410) and the offset is subtracted: a lattice of more than 2^32
                                   voxels is fused block by block with identical voxels (DenseReconstructor.merge_pointclouds does).  Both
                                   channels: the TSDF kernels place voxel i at the lattice index offset + i, so a block's TSDF records are
                                   the single lattice's bit for bit; a grid with a TSDF channel must end within 2^23 voxels of the lattice
                                   origin on every axis (offset + n <= 2^23: the f32 index arithmetic stays exact).  tl3d_raycast refuses
                                   a grid with an offset.                                                                            */
} tl3d_config;

/* Result of an ICP run (device solve, read back once at the end). */
typedef struct tl3d_icp_result {
    double T[16];               /* src-camera -> tgt-camera, row-major 4x4                         */
    double fitness;             /* correspondences / valid source samples, at T                    */
    double rmse;                /* sqrt(mean r^2) over correspondences, at T                       */
    int64_t n_corr;             /* correspondences at T                                            */
    int64_t n_src;              /* valid source samples                                            */
    int32_t iters_run;          /* iterations that produced an update                              */
    int32_t status;             /* 0 ok, 1 converged early, 2 singular system (T from last good)   */
    double scale;               /* metric scale of the source depth at the end: the caller's scale_src, or the estimate
                                   of a run with estimate_scale (replaces the SfM scale of D2R:297-326 / DER:659-697) */
} tl3d_icp_result;

typedef struct tl3d_icp_params {
    int32_t iters;              /* maximum Gauss-Newton iterations                                 */
    int32_t stride;             /* source pixel stride                                             */
    double max_dist;            /* correspondence gate |p-q| (metres)                              */
    double damping;             /* Levenberg factor: A += damping * trace(A)/6 * I                 */
    double eps;                 /* stop when |update|_inf < eps                                    */
    double eig_rel;             /* drop directions with eigenvalue < eig_rel * largest (unobservable DOFs) */
    int32_t estimate_scale;     /* 1: Sim(3) -- the metric scale of the SOURCE depth is a 7th unknown (sigma <- sigma
                                   exp(alpha), Jacobian column n . (R sigma p)), solved with the pose under the same
                                   eigenvalue cutoff: where the geometry does not observe it, it keeps scale_src    */
    int32_t reserved;
} tl3d_icp_params;

/* per-launch statistics of the fusion kernels, for roofline accounting */
typedef struct tl3d_stats {
    uint64_t tsdf_launches;
    uint64_t tsdf_records_read;      /* voxel records loaded by tl3d_integrate kernels (counting mode) */
    uint64_t tsdf_records_written;
    uint64_t tsdf_bricks_visited;    /* bricks that passed culling                                      */
    uint64_t tsdf_bricks_free;       /* of those: free-space bricks (no depth lookups)                   */
    uint64_t tsdf_bricks_free_counted; /* of those: handled by ONE add to the brick's free-space counter instead of a
                                          read-modify-write of its 512 records (8 B instead of 8 KB; counting mode)   */
    uint64_t centroid_launches;
    uint64_t centroid_points;        /* points accumulated                                              */
    uint64_t centroid_dropped;       /* valid points that fell outside the grid                         */
    double tsdf_kernel_ms;           /* summed hipEvent time of the integrate kernels (profile mode)    */
    uint64_t tsdf_kernel_timed;      /* launches contributing to tsdf_kernel_ms                         */
    uint64_t tsdf_batch_bricks;      /* bricks the update launches visited (a brick once per batch of frames; counting mode) */
    uint64_t bp_lookback_retries;    /* tl3d_backproject calls repeated in dynamic tile order after a look-back time-out */
    uint64_t icp_batch_timeouts;     /* batched registrations whose in-launch barrier timed out ...                  */
    uint64_t icp_batch_fallback_pairs; /* ... and the pairs re-registered through the per-iteration kernel instead   */
    uint64_t merge_bricks_sent;      /* tl3d_allreduce_grid: bricks whose records went over the wire (all merges so far) ... */
    uint64_t merge_bricks_total;     /* ... of this many bricks in the grid                                              */
    uint64_t pool_slots_tsdf;        /* sparse grids: brick slots handed out so far, per channel (dense: every brick)             */
    uint64_t pool_slots_centroid;
    uint64_t pool_refused;           /* first touches refused because a pool was full: > 0 means the result lacks those bricks   */
    uint64_t centroid_record_updates; /* 32-B centroid records added to in the grid (counted: one per distinct voxel and tile of samples) */
} tl3d_stats;

const char *tl3d_last_error(void);
int tl3d_version(void);
int tl3d_device_count(int *n);
/* HIP_VERSION the library was compiled with, and the runtime / driver versions it is running on (the binding refuses a
 * different major version: PyTorch-ROCm wheels bundle their own runtime and both must resolve to one copy). */
int tl3d_runtime_info(int *hip_compiled, int *hip_runtime, int *hip_driver);
/* Measurement aid: n_streams one-wave kernels of spin_ms each, one per fresh stream; elapsed_ms ~ ceil(n_streams / Q) *
 * spin_ms where Q is the number of hardware queues the runtime really multiplexes streams onto (GPU_MAX_HW_QUEUES is
 * read when the HIP runtime initialises -- setting it later has no effect; the ICP lanes and prep streams want >= 20). */
int tl3d_probe_hw_queues(int device, int n_streams, double spin_ms, double *elapsed_ms);

/* lifetime */
int tl3d_create(const tl3d_config *cfg, int device, tl3d_ctx **out);
int tl3d_destroy(tl3d_ctx *ctx);
int tl3d_sync(tl3d_ctx *ctx);
/* The hipStream_t the context enqueues on (the caller's, tl3d_config.stream, or the library's own): so that a caller can put ITS device
 * work -- a collective on the grid memory -- in the same order instead of waiting for the device (tl3d.distributed does). */
int tl3d_get_stream(tl3d_ctx *ctx, void **stream);
/* The frame buffers of a destroyed context stay in a process-wide cache (by device and size, at most 64 GiB) for the next context
 * of the same shape: the reference's process reconstructs one sequence per run (D2R:705-808), a service reconstructs many, and
 * memory the driver has just taken back is slow to come out of it again.  This call returns all of it to the driver (a host that
 * shares the GPU with another allocator calls it between batches of sequences); an allocation that fails does so by itself. */
int tl3d_release_cached_memory(void);

/* a2: frames.  Replaces DepthImageLoader.load_depth's dtype handling (D2R:80-97) and the in-RAM frame
 * lists self.images/self.depths (D2R:434-437).  bgr may be NULL (colour (0,0,0)). */
int tl3d_upload_frame(tl3d_ctx *ctx, int slot, const void *depth_hd, int depth_kind, const uint8_t *bgr_hd);
int tl3d_download_depth(tl3d_ctx *ctx, int slot, float *depth_out_hd);
/* f2: decode/upload pipeline (replaces holding every decoded frame in host RAM, D2R:434-437, 469-470).
 * Pinned staging buffers + an upload that returns at once: the host buffers must stay untouched until
 * tl3d_slot_wait(slot) returns.  Kernels that read the slot are ordered after the copy on the device. */
int tl3d_pinned_alloc(size_t bytes, void **out);
int tl3d_pinned_free(void *p);
int tl3d_upload_frame_async(tl3d_ctx *ctx, int slot, const void *depth_hd, int depth_kind, const uint8_t *bgr_hd);
int tl3d_slot_wait(tl3d_ctx *ctx, int slot);

/* Depth-frame filter: flying pixels and small regions (no reference code: the reference fuses its depth maps as
 * they come -- the rules are ours, the question librealsense's and Open3D's depth clean-ups answer).  The filter only ever
 * INVALIDATES pixels (writes 0); it never smooths or alters a value, and its result is an exact function of the image.
 * The image is one depth image of the context's W x H, f32 or u16 millimetres.  All arithmetic is f32, on the f32 pixel itself or on
 * the u16 value converted exactly to f32 -- never on the metres copy -- so the array call and the slot call agree bit for bit.
 * valid p: d_p is finite and d_p > 0.  An invalid pixel is never changed, whatever its bytes are (NaN payloads, -0, inf, negatives).
 * linked p, q: both valid and fabsf(d_q - d_p) <= jump * fminf(d_p, d_q), jump = jump_rel rounded once to f32: one rounded
 * subtraction, one rounded product, one compare; nothing to contract, no fast math.  The test is relative: the depth scale and the
 * choice of mm or m do not matter, and relative (unscaled) depth can be filtered.
 * Stage A, flying pixels: S_p = the number of pixels q != p of the (2 radius + 1)^2 window, inside the image, linked to p on the
 * INPUT image; a valid p with S_p < min_support becomes 0.  Pixels outside the image support nobody.
 * Stage B, small regions, on stage A's result (min_region > 1): horizontally or vertically adjacent survivors are joined when
 * linked; the regions are the transitive closure of the joins (a~b and b~c make one region even when a and c are not linked); a
 * survivor whose region has fewer than min_region pixels becomes 0.
 * counts, per image: {valid in, removed by A, regions after A, removed by B}; regions is 0 when stage B is off.
 * Parameters: jump_rel > 0 and finite (default 0.05), radius 1..3 (1), min_support 0..(2 radius + 1)^2 - 1 (4), min_region >= 0
 * (0; 0 or 1: stage B off), reserved 0.
 * tl3d_filter_depth: a pure function of one image; depth_in / depth_out are host or device pointers of depth_kind (the output has
 * the kind of the input), counts_out [4] is host memory; depth_out == depth_in is allowed, any other overlap is refused; needs no
 * grid and touches no slot.
 * tl3d_filter_depth_slots: filters the resident frames slots[0..n) in place, each as a new upload of the slot would be ordered
 * (behind the deferred TSDF updates and every uncollected ICP run that reads the slot) and with what a new upload voids: the normal
 * map, the averaged depth, the TSDF tile and classification caches.  A u16 slot is filtered on its millimetres, and both the
 * millimetres and the f32 copy are zeroed; colour is untouched.  counts_out [n][4] (host) may be NULL.  n == 0 is TL3D_OK; a slot
 * that holds no frame is TL3D_E_STATE.
 * TL3D_E_INVALID before any device work, with nothing written: a null argument, a bad depth_kind, a parameter outside its range,
 * reserved != 0, n < 0, a slot out of range or named twice, overlapping images.
 * Tests (tests/test_gpu_depth_filter*.py): output bits and counts equal two numpy formulations on crafted images (tile seams,
 * link decisions one f32 ulp apart, union-find topologies, invalid bit patterns); stale slot state; the pipeline option. */
typedef struct tl3d_depth_filter_params {
    double jump_rel;
    int32_t radius;
    int32_t min_support;
    int64_t min_region;
    int32_t reserved;
} tl3d_depth_filter_params;
int tl3d_filter_depth(tl3d_ctx *ctx, const void *depth_in_hd, int depth_kind, const tl3d_depth_filter_params *params,
                      void *depth_out_hd, int64_t *counts_out /* [4] */);
int tl3d_filter_depth_slots(tl3d_ctx *ctx, int n, const int32_t *slots, const tl3d_depth_filter_params *params,
                            int64_t *counts_out /* [n][4] or NULL */);

/* a3+a4/a5: DenseReconstructor.depth_to_pointcloud (depth_to_reconstruction.py:328-384) and
 * DensePointCloudGenerator.depth_to_pointcloud (depth_enhanced_reconstruction.py:554-613).
 * Writes the surviving points in row-major pixel order.  cap = capacity in points; on
 * TL3D_E_CAPACITY *out_n is the required count.  out_* may be host or device pointers. */
int tl3d_backproject(tl3d_ctx *ctx, int slot, const double R[9], const double t[3], double scale,
                     uint32_t flags, int subsample, double min_depth, double max_depth,
                     float *out_xyz_hd, uint8_t *out_rgb_hd, int64_t cap, int64_t *out_n);

/* The same, asynchronous and device-only: points, colours AND the count go to device memory (out_n_dev: one int64),
 * nothing is read back and the call returns as soon as its one kernel is enqueued.  cap is the capacity of the buffers in
 * points (ceil(H/s) * ceil(W/s) always suffices); points beyond cap are not written, the count is the true one. */
int tl3d_backproject_device(tl3d_ctx *ctx, int slot, const double R[9], const double t[3], double scale,
                            uint32_t flags, int subsample, double min_depth, double max_depth,
                            float *out_xyz_dev, uint8_t *out_rgb_dev, int64_t cap, int64_t *out_n_dev);

/* Extent of the points tl3d_backproject would emit for this frame, without emitting them: out_min / out_max = component-wise
 * min / max of the float32 points (+inf / -inf when no pixel survives).  What `p.min(0)`, `p.max(0)` give the reference when it
 * bounds a cloud for Open3D's voxel origin (D2R:404-410). */
int tl3d_frame_bounds(tl3d_ctx *ctx, int slot, const double R[9], const double t[3], double scale, uint32_t flags,
                      int subsample, double min_depth, double max_depth, double out_min[3], double out_max[3],
                      int64_t *out_reserved /* may be NULL */);

/* The same over n_frames frames with ONE read-back per 16 frames: R = n_frames x 9, t = n_frames x 3 (NULL with
 * TL3D_F_NO_POSE), scales = n_frames entries (NULL = 1.0).  The scene-bounding pass of the pipeline (D2R:404-410 bounds the
 * merged cloud; the extent of the union is the union of the extents). */
int tl3d_frames_bounds(tl3d_ctx *ctx, int n_frames, const int32_t *slots, const double *R, const double *t, const double *scales,
                       uint32_t flags, int subsample, double min_depth, double max_depth, double out_min[3], double out_max[3]);

/* How many 8^3 bricks a fusion of these frames into the grid `grid` describes (its geometry fields only: channels, nx ny nz, origin,
 * voxel_size, sdf_trunc; no grid need be attached) WOULD give records to, per channel: the TSDF classification of every frame
 * and the bricks the frames' samples (stride centroid_subsample; < 1: not counted) fall into, without touching a record.  What
 * the pools of a sparse grid must hold (tl3d_config.pool_bricks_*): Open3D's hash map sizes itself as the merged cloud is inserted
 * (D2R:404-410); a pool is allocated before the first frame, and this is how to know its size -- a few microseconds per frame.
 * Exact: the fusion of the same frames takes exactly these many slots (one per brick, however many waves touch it first). */
int tl3d_count_bricks(tl3d_ctx *ctx, const tl3d_config *grid, int n_frames, const int32_t *slots, const double *R, const double *t,
                      const double *scales, int centroid_subsample, double min_depth, double max_depth, int64_t *bricks_tsdf,
                      int64_t *bricks_centroid);

/* a7 (fusion half): accumulate the same points straight into the centroid channel, no point list
 * (replaces np.vstack + Open3D voxel_down_sample's hash-map insert, D2R:401-410). */
int tl3d_accumulate_centroid(tl3d_ctx *ctx, int slot, const double R[9], const double t[3], double scale,
                             uint32_t flags, int subsample, double min_depth, double max_depth);
/* same, from an explicit point list (merge_pointclouds' call shape, D2R:386-420) */
int tl3d_accumulate_points(tl3d_ctx *ctx, const float *xyz_hd, const uint8_t *rgb_hd, int64_t n);
/* min/max bound of a point list (Open3D's voxel origin = min_bound - voxel/2).  Per axis, fminf / fmaxf over the f32 coordinates:
 * a NaN coordinate is ignored (the bounds are those of the axis' other values; numpy's p.min(0) would give NaN), an axis that holds
 * nothing but NaN keeps the empty extent out_min = +inf, out_max = -inf; infinities count as values; denormals are kept as they
 * are; the sign of a bound that is zero is not specified (tests/test_gpu_centroid_accumulate.py pins all of this). */
int tl3d_points_bounds(tl3d_ctx *ctx, const float *xyz_hd, int64_t n, double out_min[3], double out_max[3]);

/* a11: TSDF integration of one frame (no reference code; convention in DESIGN.md).
 * Free space: a brick (8^3 voxels) that lies wholly in front of everything the frame sees would get (+32767, +1) on each
 * of its 512 records; the library adds 1 to a per-brick counter instead and folds the pending counts into the records
 * before anything reads the TSDF channel's records (tl3d_grid_device_ptr, tl3d_grid_download, tl3d_grid_add, tl3d_extract,
 * tl3d_sync), so the channel's contents are the same bit for bit (tl3d_grid_max_weight and the TL3D_CH_FREE forms of the merge
 * calls work on records and counts as they stand).
 * The frame joins a pending BATCH (up to 32 frames, one depth kind): the batch's classification kernels run on a side stream,
 * then ONE update kernel on the context's stream reads and writes every touched record once for all its frames.  A batch is
 * issued when it is full and whenever any other call touches the grid or a slot (tl3d_sync, tl3d_event_record and
 * tl3d_grid_device_ptr included), so results never depend on the batching; a caller that works on a grid pointer obtained
 * EARLIER must call tl3d_grid_device_ptr (or tl3d_sync) again before using it. */
int tl3d_integrate(tl3d_ctx *ctx, int slot, const double R[9], const double t[3], double scale);
/* The fusion loop of a sequence in one call (replaces D2R:625-659 per view): for i in 0..n-1, tl3d_integrate (when the TSDF
 * channel exists) and, when centroid_subsample >= 1 and the centroid channel exists, tl3d_accumulate_centroid of slots[i] with
 * pose (R + 9 i, t + 3 i) and scales[i] (NULL = 1.0).  Same results as the per-frame calls in that order. */
int tl3d_fuse_frames(tl3d_ctx *ctx, int n, const int32_t *slots, const double *R, const double *t, const double *scales,
                     uint32_t flags, int centroid_subsample, double min_depth, double max_depth);

/* a10: vertex/normal map + point-to-plane ICP (no reference code; replaces the SIFT/essential-matrix
 * pose front end D2R:144-215 as the pose source, output in the convention of D2R:618-620). */
int tl3d_build_normals(tl3d_ctx *ctx, int slot, double scale, double depth_jump);
/* the same for n slots in one call (scales: n entries or NULL = 1.0): what a host loop over the frames of a sequence does
 * before registering them (D2R:573 per frame), without a foreign call per frame */
int tl3d_build_normals_many(tl3d_ctx *ctx, int n, const int32_t *slots, const double *scales, double depth_jump);
int tl3d_download_normals(tl3d_ctx *ctx, int slot, float *nmap_out_hd /* [H][W][4] */);
int tl3d_icp_p2plane(tl3d_ctx *ctx, int slot_src, double scale_src, int slot_tgt, const double T_init[16],
                     const tl3d_icp_params *prm, tl3d_icp_result *out);
/* The same registration, asynchronous: one ICP run is a chain of short dependent kernels (latency-bound), but runs
 * for different frame pairs are independent, so up to TL3D_ICP_LANES of them may be in flight, each on its own
 * stream.  enqueue returns at once; collect blocks for that lane's result.  A lane holds one run at a time. */
#define TL3D_ICP_LANES 16
/* A run reads slot_src's depth and slot_tgt's normal map until it is collected.  tl3d_upload_frame* into slot_src and
 * tl3d_build_normals of slot_tgt issued meanwhile are ordered behind the run on the device (they do not corrupt it). */
int tl3d_icp_enqueue(tl3d_ctx *ctx, int lane, int slot_src, double scale_src, int slot_tgt, const double T_init[16],
                     const tl3d_icp_params *prm);
int tl3d_icp_collect(tl3d_ctx *ctx, int lane, tl3d_icp_result *out);

/* a2 (host side of the decode pipeline; no GPU call): the decode workers of a host copy image rows into pinned staging
 * buffers without holding their interpreter's lock (a foreign call releases it).  rows = `height` pointers to image rows as an
 * image library keeps them: R,G,B,X 4-byte pixels -> packed B,G,R (what cv2.imread hands the reference, D2R:454), or rows
 * of row_bytes bytes copied as they are (16-bit depth PNGs, D2R:86-90). */
int tl3d_host_pack_bgr_rows(uint8_t *dst, const uint8_t *const *rows, int height, int width);
int tl3d_host_copy_rows(uint8_t *dst, const uint8_t *const *rows, int height, size_t row_bytes);

/* a10, batched: n_pairs independent registrations, each through ALL of `levels` (coarse to fine: a level starts from the
 * pose the previous one ended with; a pair stops early when a level fails or ends with fewer than 8 correspondences, as
 * the per-level calls above are used by a host) in ONE kernel launch: no host round trip and no launch per iteration.
 * The result of a pair is that of its last level run; it does not depend on which batch the pair is in.  One batch may be
 * in flight per context (own stream); uploads and normal maps issued before the enqueue precede it, slot rewrites issued
 * after it wait for it.  What replaces the reference's per-pair detect_and_match + compute_pose calls (D2R:573-596). */
#define TL3D_ICP_MAX_LEVELS 4
typedef struct tl3d_icp_pair {
    int32_t slot_src, slot_tgt;
    double scale_src;           /* metric scale of the source depth                                */
    double T_init[16];          /* initial src-camera -> tgt-camera pose, row-major 4x4            */
} tl3d_icp_pair;
int tl3d_icp_batch_enqueue(tl3d_ctx *ctx, const tl3d_icp_pair *pairs, int n_pairs, const tl3d_icp_params *levels, int n_levels);
int tl3d_icp_batch_collect(tl3d_ctx *ctx, tl3d_icp_result *out /* [n_pairs] */, int n_pairs);

/* a10, evaluation: ONE point-to-plane pass for each pair at the pose pairs[i].T_init (src camera -> tgt camera), no update: the
 * normal equations a registration pass forms there (same source vertex -- the window-averaged depth when normal smoothing is on --
 * same association, gate, residual and J = [p x n, n] as tl3d_icp_*; f32 values, fp64 sums of fp64 products).  A is the weight of
 * the pair as an edge of a pose graph (the Hessian of its point-to-plane cost at T); n_corr / n_src score a candidate pair without
 * registering it.  One launch per call (chunks of pairs beyond the scratch buffer), then a fixed-order sum per pair: a pair's
 * result is bit for bit the same in every run, whatever n_pairs and wherever the pair stands in the batch.  n_pairs >= 0.  Blocks
 * and fills `out`; ordered behind the uploads and normal maps issued before it.  TL3D_E_STATE while an ICP batch is uncollected or
 * when a slot holds no frame / a target slot has no normal map; TL3D_E_INVALID for slots out of range, stride < 1, max_dist <= 0. */
typedef struct tl3d_icp_eval {
    double A[21];               /* upper triangle of sum J J^T, row-major, J = [p x n, n]          */
    double b[6];                /* sum J r                                                         */
    double e;                   /* sum r^2                                                         */
    int64_t n_corr;             /* correspondences at T                                            */
    int64_t n_src;              /* valid source samples                                            */
} tl3d_icp_eval;
int tl3d_icp_evaluate_pairs(tl3d_ctx *ctx, const tl3d_icp_pair *pairs, int n_pairs, int stride, double max_dist,
                            tl3d_icp_eval *out /* [n_pairs] */);

/* a10, with colour: joint point-to-plane + photometric registration (no reference code: the reference takes its
 * poses from image features).  Beside the geometric residual of tl3d_icp_* a correspondence contributes the difference between the
 * smoothed intensity of its source pixel and that of the target image at its projection, which observes the in-surface motion that
 * point-to-plane cannot (a tube's axis, a wall's plane).
 * tl3d_build_intensity_many: the intensity map of each of the n slots, from its colour image and its f32 depth: per pixel
 * (S, Sx, Sy, flag) with y = 29 B + 150 G + 77 R, S = (float)sum y / (float)(count * 65280) over the pixels of the (2 radius + 1)^2
 * window that are in the image, valid (depth finite and > 0) and linked to the centre (fabsf(a - b) <= depth_jump * fminf(a, b), the
 * depth filter's rule), flag 0 for an invalid centre (the record is zero), 2 when all four axis neighbours are in the image, valid
 * and linked to the centre, else 1; Sx, Sy the central differences of S where flag is 2, else 0.  Bit for bit a function of the two
 * images.  Every rewrite of the slot (upload, tl3d_filter_depth_slots, a ray cast into it) voids the map.  TL3D_E_STATE for a slot
 * without a frame or without colour; TL3D_E_INVALID for a slot out of range, radius outside 0..7, depth_jump not positive. */
int tl3d_build_intensity_many(tl3d_ctx *ctx, int n, const int32_t *slots, int radius, double depth_jump);
/* the slot's intensity map, row-major; host or device memory.  TL3D_E_STATE without a map. */
int tl3d_download_intensity(tl3d_ctx *ctx, int slot, float *imap_out_hd /* [H][W][4] */);
/* ONE pass of both systems for each pair at pairs[i].T_init, no update.  The geometric half is tl3d_icp_evaluate_pairs' (same
 * samples, counts and terms).  A geometric correspondence (source pixel (u, v), target pixel (ut, vt), projection (uf, vf))
 * QUALIFIES when the target record has flag 2 and the source record flag >= 1; it is a photometric correspondence when also
 * |r_I| <= photo_gate, r_I = S_t + Sx_t (uf - ut) + Sy_t (vf - vt) - S_s; J_I = [q x g, g] with g the gradient of r_I with respect
 * to the transformed point q.  f32 values, fp64 sums of fp64 products, the two systems apart; a pair's result is bit for bit the
 * same in every run, whatever n_pairs and wherever the pair stands.  n_pairs >= 0; chunked like tl3d_icp_evaluate_pairs; blocks.
 * TL3D_E_STATE while an ICP batch is uncollected, for a slot without a frame or without an intensity map, a target without a normal
 * map; TL3D_E_INVALID for slots out of range, stride < 1, max_dist or photo_gate not positive. */
typedef struct tl3d_rgbd_eval {
    tl3d_icp_eval geo;          /* the point-to-plane system, as tl3d_icp_evaluate_pairs gives it  */
    double A_p[21];             /* upper triangle of sum J_I J_I^T, row-major                      */
    double b_p[6];              /* sum J_I r_I                                                     */
    double e_p;                 /* sum r_I^2                                                       */
    int64_t n_photo;            /* photometric correspondences                                     */
    int64_t n_qualified;        /* geometric correspondences whose two records qualify             */
} tl3d_rgbd_eval;
int tl3d_rgbd_evaluate_pairs(tl3d_ctx *ctx, const tl3d_icp_pair *pairs, int n_pairs, int stride, double max_dist, double photo_gate,
                             tl3d_rgbd_eval *out /* [n_pairs] */);
/* The registration: every pair through all of `levels`, coarse to fine, every iteration on the device (two launches per iteration
 * for the whole batch), then a final pass at the result.  An iteration solves (A_g + photo_weight A_p + lam I) x = -(b_g +
 * photo_weight b_p) -- damping and the eigenvalue cutoff eig_rel act on the joint system, so a photo_weight too small leaves the
 * photometric directions under the cutoff -- and applies T <- exp(x) T.  Stop, failure and level chaining as the batched ICP above
 * (a pass with fewer than 6 geometric correspondences fails the run, a level that ends with fewer than 8 is the pair's last);
 * photo_weight 0 is the point-to-plane registration.  out as the batched ICP fills it (fitness, rmse, n_corr, n_src geometric);
 * info (may be NULL) adds the photometric statistics of the final pass.  Blocks.  Errors as tl3d_rgbd_evaluate_pairs, and
 * TL3D_E_INVALID for n_levels outside 1..TL3D_ICP_MAX_LEVELS, a negative photo_weight, estimate_scale. */
typedef struct tl3d_rgbd_level {
    tl3d_icp_params icp;        /* iters, stride, max_dist, damping, eps, eig_rel; estimate_scale must be 0 */
    double photo_weight;        /* lambda >= 0: weight of the photometric system                   */
    double photo_gate;          /* |r_I| <= photo_gate, in units of S (0..1)                       */
} tl3d_rgbd_level;
typedef struct tl3d_rgbd_info {
    double photo_rmse;          /* sqrt(e_p / n_photo) of the final pass, 0 without correspondences */
    int64_t n_photo;            /* photometric correspondences of the final pass                   */
    int64_t n_qualified;        /* geometric correspondences whose two records qualify             */
} tl3d_rgbd_info;
int tl3d_rgbd_register_pairs(tl3d_ctx *ctx, const tl3d_icp_pair *pairs, int n_pairs, const tl3d_rgbd_level *levels, int n_levels,
                             tl3d_icp_result *out /* [n_pairs] */, tl3d_rgbd_info *info /* [n_pairs] or NULL */);

/* grids */
/* Give a context created with channels = 0 its grid later (geometry fields of cfg: channels, nx, ny, nz, origin,
 * voxel_size, sdf_trunc, ext_*): frames stay resident while poses and scene bounds are still being computed. */
int tl3d_attach_grid(tl3d_ctx *ctx, const tl3d_config *cfg);
/* Free the grid of a context: channels, brick tables, free-space counters and every grid-sized scratch (pending updates are
 * issued first).  Frames, normal maps and ICP state stay resident, and tl3d_attach_grid works again: one context fuses a lattice
 * of more than 2^32 voxels block after block.  TL3D_E_STATE on a context without a grid.  Clears the block core. */
int tl3d_detach_grid(tl3d_ctx *ctx);
/* Make the attached grid one BLOCK of a lattice of lattice_dims voxels (whose voxel 0 is the grid's voxel -voxel_offset) and give it
 * a CORE [lo, hi) of grid-local voxels (multiples of TL3D_BRICK; the rest of the grid is its halo).  With a core: tl3d_extract emits
 * only the voxels in the core (centroid mode) or the owner voxels in the core (TSDF mode); tl3d_extract_mesh emits the triangles of
 * the cells whose min corner lies in the core (vertices as without a core); tl3d_stats.centroid_points counts the samples that
 * landed in the core and centroid_dropped the rest (samples in the halo are still accumulated).  Disjoint cores that tile the
 * lattice, each with a halo of one brick on the + sides that have a neighbour, give the single lattice's points and mesh
 * (DESIGN §3).  NULL arguments clear the core (tl3d_detach_grid does too).  TL3D_E_INVALID for a lattice of 2^61 voxels or more
 * (mesh keys would overflow); TL3D_E_STATE without a grid. */
int tl3d_set_block_core(tl3d_ctx *ctx, const int64_t lattice_dims[3], const int32_t lo[3], const int32_t hi[3]);
int tl3d_grid_reset(tl3d_ctx *ctx);
int tl3d_grid_device_ptr(tl3d_ctx *ctx, uint32_t channel, void **ptr, size_t *bytes);
int tl3d_grid_download(tl3d_ctx *ctx, uint32_t channel, void *out_hd, size_t bytes);
int tl3d_grid_upload(tl3d_ctx *ctx, uint32_t channel, const void *in_hd, size_t bytes);
int tl3d_grid_add(tl3d_ctx *ctx, uint32_t channel, const void *other_hd, size_t bytes);   /* grid += other (merge) */
/* largest number of observations any voxel of the TSDF channel holds (one reduction over the grid, blocks) */
int tl3d_grid_max_weight(tl3d_ctx *ctx, int64_t *out);

/* Sparse form of the merge (a frame-sharded run touches a few per cent of a large grid): which bricks hold anything, and their
 * records as one contiguous block.  tl3d_grid_touched_bricks ORs 1 into map[b] (one byte per brick, nx ny nz / 512 of them, device
 * memory; the caller zeroes it) for every brick with a TSDF weight or a centroid count in the selected channels; after a MAX
 * all-reduce of the map every rank holds the same brick set.  tl3d_grid_pack_bricks copies the records of bricks[0 .. n) (device
 * memory, ascending brick indices) of ONE channel into `packed` (n x 4 KB for TL3D_CH_TSDF, n x 16 KB for TL3D_CH_CENTROID, device
 * memory); tl3d_grid_unpack_bricks writes such a block back (after the SUM all-reduce).  tl3d.distributed.merge_context_grids and
 * tl3d_allreduce_grid use them when fewer than half of the bricks are touched; tl3d.distributed passes TL3D_CH_FREE with the TSDF
 * channel and sums the counts separately (config-5 shape, 32 frames: 29 % of the bricks hold free-space counts, a few per cent records).
 *
 * The contract (tests/test_gpu_grid_merge.py holds each of these against an integer model):
 *  - row order is record order: the row of brick b is records [512 b, 512 b + 512); with TL3D_CH_SUB the row of id 8 b + s is
 *    records [512 b + 64 s, + 64), the 4x4x4 cube s = x >> 2 | (y >> 2) << 1 | (z >> 2) << 2 of the brick;
 *  - unpack SETS the listed rows to the block (it does not add: the caller has summed) and leaves every other record alone;
 *  - ids must be ascending, unique and below the row count (nx ny nz / 512, times 8 with TL3D_CH_SUB).  n and the pointers are
 *    checked on the host (TL3D_E_INVALID); the ids themselves are NOT validated on the device: an id out of range is an
 *    out-of-bounds access, a duplicate id given to unpack a race between two rows;
 *  - a sparse grid draws pool slots ON RECEIPT: unpack (like tl3d_grid_add and tl3d_grid_upload) gives a brick without records a
 *    slot when its row holds a non-zero word; a row of zeros draws none; pack gives zeros for a brick without records.  With the
 *    pool exhausted the row is dropped and the brick counted once in tl3d_stats.pool_refused (it reads as untouched afterwards);
 *  - without TL3D_CH_FREE the pending free-space counts are folded into the records first (a brick of a sparse grid that has no
 *    records keeps its count: pack gives zeros for it and touched_bricks does not mark it); with TL3D_CH_FREE nothing is folded,
 *    a brick that holds nothing but a count is not marked and its rows are the records alone. */
int tl3d_grid_touched_bricks(tl3d_ctx *ctx, uint32_t channels, uint8_t *map_dev, int64_t n_bricks);
int tl3d_grid_pack_bricks(tl3d_ctx *ctx, uint32_t channel, const uint32_t *bricks_dev, int64_t n, void *packed_dev);
int tl3d_grid_unpack_bricks(tl3d_ctx *ctx, uint32_t channel, const uint32_t *bricks_dev, int64_t n, const void *packed_dev);

/* e: the merge step of the multi-GPU path for hosts WITHOUT torch.distributed (frames shard across
 * ranks, one sum all-reduce of the per-GPU grids at merge time).  One process per GPU; rank 0 obtains an id and hands it
 * to the others by any means (file, socket, MPI); every rank then joins and merges.  RCCL is loaded at run time
 * (librccl.so, the copy already in the process if there is one), so libtl3d.so itself does not depend on it.  The
 * all-reduce runs on the context's stream, in place on the grid memory (int32 / uint64 sums: the merged grid is
 * bit-identical to a single-GPU run); the TSDF channel's int32 headroom (TL3D_TSDF_MAX_WEIGHT) is checked over all ranks
 * first and the merge refused with TL3D_E_STATE if it could wrap.  Python hosts use tl3d.distributed (same operations
 * through torch.distributed on tl3d_grid_device_ptr memory). */
#define TL3D_RCCL_ID_BYTES 128
int tl3d_rccl_unique_id(uint8_t id_out[TL3D_RCCL_ID_BYTES]);
int tl3d_rccl_init(tl3d_ctx *ctx, int world, int rank, const uint8_t id[TL3D_RCCL_ID_BYTES]);
int tl3d_allreduce_grid(tl3d_ctx *ctx, uint32_t channels /* TL3D_CH_* mask; 0 = every channel the grid has */);

/* a7 (read-back half) + N4: fused grid -> point list. min_count: centroid occupancy threshold;
 * tsdf gate (centroid mode, only if the TSDF channel exists and min_weight > 0): keep voxels with
 * weight >= min_weight and |mean tsdf| <= max_abs_tsdf. */
int tl3d_extract(tl3d_ctx *ctx, int mode, int min_count, int min_weight, double max_abs_tsdf,
                 float *out_xyz_hd, uint8_t *out_rgb_hd, int64_t cap, int64_t *out_n);

/* marching cubes over the TSDF channel: vertices = owned zero-crossing edges, record order;
 * triangles by cell, uint32 indices, wound so (v1-v0)x(v2-v0) points to t > 0.
 * Call with NULL buffers for the counts, then with capacities >= the counts (host or device pointers).
 * TL3D_E_STATE without a TSDF channel; TL3D_E_CAPACITY on short buffers, or when the mesh has 2^31 vertices or more
 * (the counts are stored first).  No reference code: the reference has no TSDF. */
int tl3d_extract_mesh(tl3d_ctx *ctx, int min_weight,
                      float *out_xyz_hd, uint8_t *out_rgb_hd, int64_t vert_cap,
                      uint32_t *out_tri_hd, int64_t tri_cap,
                      int64_t *out_n_vert, int64_t *out_n_tri);
/* The same, plus one int64 KEY per vertex: 3 * (lattice linear index of the owner voxel, x fastest, over the lattice of
 * tl3d_set_block_core -- without a core: voxel_offset + grid dims) + axis.  Equal keys = the same vertex in another block: what
 * lets a host weld the meshes of neighbouring blocks exactly. */
int tl3d_extract_mesh_keyed(tl3d_ctx *ctx, int min_weight,
                            float *out_xyz_hd, uint8_t *out_rgb_hd, int64_t vert_cap,
                            uint32_t *out_tri_hd, int64_t tri_cap, int64_t *out_key_hd,
                            int64_t *out_n_vert, int64_t *out_n_tri);

/* Connected components of an indexed triangle list: n_vert vertices, n_tri rows of three uint32 indices, any mesh
 * (the calls need no grid).  Two vertices are connected when one triangle names both; label[v] = the smallest vertex index of v's
 * component; a vertex no triangle names is a component of its own with 0 triangles; a triangle belongs to the component of its
 * vertices, and (a, a, b) counts as one and connects a and b.  Labels, counts and the filtered mesh are functions of the input
 * alone: every run gives the same bytes.  No reference code: the reference has no mesh (Open3D clusters by shared EDGES; this
 * clusters by shared vertices).  Host or device pointers throughout.
 * The labelling call: label_out [n_vert]; tri_count_out [n_vert] or NULL: the component's triangle count at index = label, 0
 * elsewhere; *out_n_components = the number of labels.
 * The filter call keeps the components with at least min_triangles triangles (<= 0: every component, isolated vertices
 * included: the identity; from 1 upward the vertices no triangle uses go); largest_only: only the component with the most
 * triangles (ties: the smaller label), and only if it also passes min_triangles; a mesh without triangles then keeps nothing.
 * Kept vertices (xyz, and rgb unless rgb_hd is NULL) and re-indexed triangles keep their relative order; keep_vert_out [n_vert] or
 * NULL: 1 for a kept vertex.  No size query: pass vert_cap = n_vert and tri_cap = n_tri; short capacities give TL3D_E_CAPACITY
 * with the four counts stored (vertices and triangles kept, components found and kept).
 * TL3D_E_INVALID (decided before any device call, except the index check, which is a pass of its own in front of every indexed
 * access): a null ctx, negative sizes, n_vert >= 2^31, n_tri >= 2^32, an index >= n_vert, an output that overlaps an input.
 * n_tri == 0 or n_vert == 0 is TL3D_OK (n_vert == 0: nothing is read). */
int tl3d_mesh_components(tl3d_ctx *ctx, const uint32_t *tri_hd, int64_t n_tri, int64_t n_vert,
                         uint32_t *label_out_hd, uint32_t *tri_count_out_hd, int64_t *out_n_components);
int tl3d_mesh_filter_components(tl3d_ctx *ctx, const float *xyz_hd, const uint8_t *rgb_hd, int64_t n_vert,
                                const uint32_t *tri_hd, int64_t n_tri, int64_t min_triangles, int largest_only,
                                float *out_xyz_hd, uint8_t *out_rgb_hd, int64_t vert_cap, uint32_t *out_tri_hd, int64_t tri_cap,
                                uint8_t *keep_vert_out_hd,
                                int64_t *out_n_vert, int64_t *out_n_tri, int64_t *out_n_components, int64_t *out_n_kept);

/* Vertex-clustering simplification of an indexed triangle mesh: n_vert vertices (xyz f32 [V][3], rgb u8 [V][3] or
 * NULL), n_tri rows of three uint32 indices, any mesh (the call needs no grid), a cell size in metres and an origin (NULL: 0, 0, 0).
 * No reference code: the reference has no mesh (Open3D's simplify_vertex_clustering is the model); the rules are ours, chosen so
 * that the output is a function of the input alone, bit for bit, in every run.
 * Cell of a vertex, per axis a, in fp64 with every operation rounded once: d = (double)x_a - o_a; i_a = floor(d / cell);
 * r = d - (double)i_a * cell; q_a = (int64)rint((r / cell) * 16777216.0) (half to even; q_a may be slightly negative or slightly
 * above 2^24).  Every vertex, named by a triangle or not, must be finite with -2^20 <= i_a < 2^20.
 * A cluster is the set of vertices with equal (i_x, i_y, i_z): a member count n, exact integer sums S_a = sum q_a and C_c = sum
 * rgb_c.  Clusters are numbered in the order of their smallest member vertex index, and EVERY cluster becomes an output vertex,
 * also one that no surviving triangle names (tl3d_mesh_filter_components with min_triangles = 1 drops those):
 *   position (float)(o_a + ((double)i_a + (double)S_a / ((double)n * 16777216.0)) * cell), operations in that order;
 *   colour (2 C_c + n) / (2 n) in integers: the mean, halves rounded up;
 *   vert_map_out [n_vert] or NULL: the output index of each input vertex's cluster.
 * Triangles: the three indices go through vert_map; a triangle with two equal mapped indices is dropped (degenerate); of the
 * triangles with the same canonical triple (the cyclic rotation that puts the smallest index first, which keeps the winding) the one
 * with the smallest input index stays and the others are dropped (duplicate) -- (A, B, C) and (A, C, B) are different triangles
 * and both stay; survivors are written in input order, mapped but not rotated.
 * Every output vertex lies in the closed box of its cell, up to the f32 rounding of the result; winding is preserved; the result
 * may be non-manifold.
 * Host or device pointers throughout.  No size query: vert_cap = n_vert and tri_cap = n_tri always suffice; short capacities give
 * TL3D_E_CAPACITY with the four counts stored (vertices and triangles out, triangles dropped as degenerate and as duplicate).
 * TL3D_E_INVALID: a null ctx, negative sizes, n_vert >= 2^31, n_tri >= 2^32, cell or origin not finite, cell <= 0, an output that
 * overlaps an input (all decided before any device call); an index >= n_vert, a vertex that is not finite or whose cell index is
 * out of range (two passes of their own in front of every indexed access).  n_vert == 0 or n_tri == 0 is TL3D_OK (n_vert == 0:
 * nothing is read; n_tri == 0: the vertices are clustered all the same). */
int tl3d_mesh_simplify_clusters(tl3d_ctx *ctx, const float *xyz_hd, const uint8_t *rgb_hd, int64_t n_vert,
                                const uint32_t *tri_hd, int64_t n_tri, double cell, const double origin[3],
                                float *out_xyz_hd, uint8_t *out_rgb_hd, int64_t vert_cap, uint32_t *out_tri_hd, int64_t tri_cap,
                                uint32_t *vert_map_out_hd,
                                int64_t *out_n_vert, int64_t *out_n_tri, int64_t *out_n_degenerate, int64_t *out_n_duplicate);

/* tl3d_mesh_simplify_clusters with every cluster's vertex placed by its quadric error instead of at the members' mean (Lindstrom's
 * quadric clustering, Out-of-Core Simplification of Large Polygonal Models, 2000; the area^2-weighted plane quadric added per
 * corner, as Open3D's quadric mode does).  Clusters, their numbering, vert_map, colours, the triangle rules, the
 * validation and the error codes are exactly those of tl3d_mesh_simplify_clusters; only positions differ.  It keeps the creases
 * and corners of piecewise planar surfaces, which the mean rounds off; on smooth curved surfaces it gains nothing.
 * Quadric coordinates: 2^10 steps per cell, h_a = (q_a + 8192) >> 14 (arithmetic shift = floor division: q may be slightly
 * negative or slightly above 2^24); seen from a cell I, a vertex v is p_a = (i(v)_a - I_a) * 1024 + h(v)_a.
 * Contribution: for every input triangle (v0, v1, v2) and every corner k, with I = i(v_k): the corner contributes iff
 * |i(v_j)_a - I_a| <= 3 for all three corners j and all axes a, otherwise it is skipped and counted.  With p_j seen from I:
 * N = (p_1 - p_0) x (p_2 - p_0), d = -(N . p_0), exact integers; N_a N_b (00, 01, 02, 11, 12, 22) go into the sums A_ab and d N_a
 * into the sums b_a of v_k's cluster.  A triangle that names a vertex twice, or has no area, adds zeros.
 * Bounds: |p| <= 4097, |N_a| < 2^27, |d| < 2^41, |N_a N_b| < 2^54, |d N_a| < 2^68; fewer than 2^34 terms, so the sums stay below
 * 2^102 in signed 128 bits: exact, hence independent of the order of the additions.
 * Solve, per cluster, in fp64, every operation rounded once, dbl() as defined for the smoothing below:
 *   1. A00 = A11 = A22 = 0 (no triangle, or only skipped and zero-area ones): the mean rule, the bytes of
 *      tl3d_mesh_simplify_clusters.  Otherwise the cluster counts as placed by its quadric, and
 *   2. T = (dbl(A00) + dbl(A11)) + dbl(A22); M_ab = dbl(A_ab) / T; g_a = dbl(b_a) / T; m_a = (double)S_a / ((double)n * 16384.0);
 *   3. K = M + reg I; r_a = reg * m_a - g_a (Tikhonov regularisation towards the mean: K is symmetric positive definite with
 *      eigenvalues in [reg, 1 + reg], so there is no eigen-decomposition, no rank decision and no square root);
 *   4. K x = r by the adjugate: c00 = K11 K22 - K12 K12, c01 = K02 K12 - K01 K22, c02 = K01 K12 - K02 K11,
 *      c11 = K00 K22 - K02 K02, c12 = K01 K02 - K00 K12, c22 = K00 K11 - K01 K01, det = (K00 c00 + K01 c01) + K02 c02,
 *      x0 = ((c00 r0 + c01 r1) + c02 r2) / det, x1 = ((c01 r0 + c11 r1) + c12 r2) / det, x2 = ((c02 r0 + c12 r1) + c22 r2) / det;
 *      then ONE step of refinement with the same cofactors: p_a = r_a - ((K_a0 x0 + K_a1 x1) + K_a2 x2),
 *      x0 = x0 + ((c00 p0 + c01 p1) + c02 p2) / det, x1 and x2 likewise (on a single plane K has the eigenvalues 1 + reg, reg,
 *      reg, the cofactors and det cancel, and the adjugate alone is off by eps / reg^2; the step brings that back to eps / reg);
 *   5. each x_a is clamped to [0, 1024] (an x_a that is not a number, which takes a reg so small that det underflows, becomes 0);
 *      a cluster with any axis clamped is counted; the output vertex stays in the closed box of its cell;
 *   6. position (float)(o_a + ((double)i_a + x_a / 1024.0) * cell), operations in that order.
 * reg: 0 < reg <= 1, finite; the pipeline passes 2^-10.  It bounds the refined solve's error near eps / reg relative and
 * biases a rank-deficient solve (a plane, a crease) towards the mean by about reg / sigma_min of the mean's offset.
 * The three further counts (clusters placed by their quadric, clusters clamped, corners skipped by the span rule) are stored with
 * the other four, also on TL3D_E_CAPACITY.  TL3D_E_INVALID as for tl3d_mesh_simplify_clusters, and for a reg outside (0, 1] (before
 * any device call).  Scratch: 144 B per input vertex on top of tl3d_mesh_simplify_clusters', only while this call is in use. */
int tl3d_mesh_simplify_quadric(tl3d_ctx *ctx, const float *xyz_hd, const uint8_t *rgb_hd, int64_t n_vert,
                               const uint32_t *tri_hd, int64_t n_tri, double cell, const double origin[3], double reg,
                               float *out_xyz_hd, uint8_t *out_rgb_hd, int64_t vert_cap, uint32_t *out_tri_hd, int64_t tri_cap,
                               uint32_t *vert_map_out_hd,
                               int64_t *out_n_vert, int64_t *out_n_tri, int64_t *out_n_degenerate, int64_t *out_n_duplicate,
                               int64_t *out_n_quadric, int64_t *out_n_clamped, int64_t *out_n_skipped);

/* Taubin smoothing and vertex normals of an indexed triangle mesh: n_vert vertices (xyz f32 [V][3]), n_tri rows of
 * three uint32 indices, any mesh (the calls need no grid).  No reference code: the reference has no mesh (Open3D's
 * filter_smooth_taubin is the model); the rules are ours, chosen so that the result is a function of the mesh alone, bit for bit, in
 * every run, and does not depend on how vertices or triangles are numbered.
 * Fixed point: Q(x) = (int64)rint((double)x * 16777216.0) (units of 2^-24 m; the product is exact, halves to even).  All sums are
 * exact integers (up to 2^76 for positions, 2^123 for normals; exact for any valence below 2^31), hence order-free.
 * dbl(N) of a wide integer N: |N| = hi * 2^64 + lo, both words unsigned; dbl = (double)hi * 18446744073709551616.0 + (double)lo,
 * negated when N < 0.  Every fp64 operation is rounded once.
 * Neighbours: u and v are neighbours iff u != v and some triangle names both; N(v) holds each neighbour once however many
 * triangles share the edge; k = |N(v)| is the valence ((a, a, b) makes a and b neighbours).
 * One step with factor s (Jacobi: every vertex reads the positions from before the step), per axis a:
 *   D_a = sum_{j in N(v)} Q(x_j,a) - k * Q(x_v,a);  x'_a = (float)((double)x_a + s * (dbl(D_a) / ((double)k * 16777216.0))),
 *   operations in that order; k = 0 copies the vertex.
 * One iteration is a step with lambda, then a step with mu.  iterations = 0 copies the input.
 * tl3d_mesh_smooth_taubin: out_xyz [V][3]; valence_out u32 [V] or NULL; *out_n_edges = the unique undirected edges.  Needs
 * 0 < lambda <= 1, -2 <= mu <= 0, 0 <= iterations <= 1000.  A step that gives a coordinate that is not finite or lies beyond 2^20 m
 * sets a flag; the call finishes its steps and returns TL3D_E_INVALID.
 * Face vector of (a, b, c): F = (Q(p_b) - Q(p_a)) x (Q(p_c) - Q(p_a)) in exact integers (units of 2^-48 m^2); the same for the three
 * cyclic rotations, 0 for a triangle that names a vertex twice.
 * tl3d_mesh_vertex_normals: N_v = sum of F over the triangles that name v (area-weighted; it points to t > 0 as the extraction's
 * winding does); n = dbl(N_v) per component, L = sqrt((n_x n_x + n_y n_y) + n_z n_z), out_normal [V][3] = (float)(n_a / L), and
 * (0, 0, 0) when N_v is zero or no triangle names v; *out_n_zero = the number of such vertices.
 * Host or device pointers throughout.  TL3D_E_INVALID: a null ctx or argument, negative sizes, n_vert >= 2^31, n_tri >= 2^32,
 * parameters out of range, an output that overlaps an input (all decided before any device call); an index >= n_vert, a vertex that
 * is not finite or has |x| > 2^20 m (two passes of their own in front of every indexed access).  n_vert == 0 is TL3D_OK and nothing
 * is read; n_tri == 0 is TL3D_OK: positions are copied, normals and valences are zero. */
int tl3d_mesh_smooth_taubin(tl3d_ctx *ctx, const float *xyz_hd, int64_t n_vert, const uint32_t *tri_hd, int64_t n_tri,
                            int iterations, double lambda, double mu, float *out_xyz_hd, uint32_t *valence_out_hd,
                            int64_t *out_n_edges);
int tl3d_mesh_vertex_normals(tl3d_ctx *ctx, const float *xyz_hd, int64_t n_vert, const uint32_t *tri_hd, int64_t n_tri,
                             float *out_normal_hd, int64_t *out_n_zero);

/* The weld of the keyed meshes of a lattice's blocks into one mesh: n_parts meshes as tl3d_extract_mesh_keyed
 * writes them, each with the core [core_lo, core_hi) of its block in LATTICE voxels (the call needs no grid).  No reference code:
 * the reference has no mesh; the result is a function of the input alone, the same bytes in every run.
 * Owner voxel of a key: idx = key / 3, x = idx % Lx, y = (idx / Lx) % Ly, z = idx / (Lx Ly).  Vertex v of part p is KEPT iff its
 * owner voxel lies in the part's core.  The output vertices (xyz, rgb, key) are the kept ones, in part order, then in the part's
 * vertex order: kept vertices that no triangle names stay; the copies that are not kept (halo copies) go, named by a triangle or
 * not.  The output triangles are all triangles of all parts, in part order, then triangle order, neither rotated nor dropped;
 * corner i of a triangle of part p becomes the output index of the kept vertex whose key equals key_p[i], in whichever part it is.
 * *out_n_twice = kept vertices minus distinct kept keys; *out_n_unowned = triangle corners whose key no kept vertex has.  Either
 * non-zero: TL3D_E_INVALID ("a vertex is owned by two block cores" / "a triangle references a vertex no block core owns") with
 * all four counts stored and the output arrays unspecified.
 * Host or device pointers throughout (the part array itself is host memory).  rgb_hd is given in every part or in none (parts
 * without vertices do not count); out_rgb_hd is required with rgb, and neither read nor written (it may be NULL) without;
 * out_key_hd may be NULL.  No size query: vert_cap =
 * the sum of n_vert and tri_cap = the sum of n_tri always suffice; short capacities, or 2^31 kept vertices or more, give
 * TL3D_E_CAPACITY with the vertex and triangle counts stored.
 * TL3D_E_INVALID, decided before any device call: a null argument, n_parts < 0, a negative size or capacity, a part with n_vert >=
 * 2^31 or n_tri >= 2^32, 2^32 triangles or more in all, a lattice dimension <= 0 or a lattice of 2^61 voxels or more, a core with
 * lo < 0, lo > hi or hi > L (an empty core is allowed and owns nothing; cores need not be multiples of 8 and need not tile the
 * lattice), rgb in some parts only, an output that overlaps an input, a null ctx.  From a pass of its own in front of every indexed
 * access: a triangle index >= its part's n_vert, a key outside [0, 3 Lx Ly Lz).  n_parts == 0, or no vertex in any part, is
 * TL3D_OK with empty outputs. */
typedef struct tl3d_mesh_part {
    const float   *xyz_hd;      /* [n_vert][3]                                   */
    const uint8_t *rgb_hd;      /* [n_vert][3], or NULL in EVERY part            */
    const int64_t *key_hd;      /* [n_vert], as tl3d_extract_mesh_keyed writes   */
    int64_t        n_vert;
    const uint32_t *tri_hd;     /* [n_tri][3], indices into THIS part            */
    int64_t        n_tri;
    int64_t        core_lo[3], core_hi[3];   /* the part's core [lo, hi) in LATTICE voxels */
} tl3d_mesh_part;
int tl3d_mesh_weld_keyed(tl3d_ctx *ctx, const tl3d_mesh_part *parts, int n_parts, const int64_t lattice_dims[3],
                         float *out_xyz_hd, uint8_t *out_rgb_hd, int64_t *out_key_hd, int64_t vert_cap,
                         uint32_t *out_tri_hd, int64_t tri_cap,
                         int64_t *out_n_vert, int64_t *out_n_tri, int64_t *out_n_twice, int64_t *out_n_unowned);

/* ray casting of the TSDF channel from one camera: one ray per pixel of the context's camera, pose (R, t)
 * world->camera as tl3d_integrate.  depth [H][W] f32 (0 = no hit), normals [H][W][3] f32 in the camera frame facing the
 * camera ((0,0,0) where undefined), colour [H][W][3] BGR (TSDF-mode extraction colour of the hit voxel, 128 without one).
 * Voxels with weight < max(1, min_weight) are unusable.  z_near <= 0: the context's min_depth; z_far <= 0: its max_depth.
 * Each output may be NULL, host or device memory.  slot >= 0: the depth (and the colour, when the slot has a colour buffer)
 * is also written into that frame slot, which then reads as an uploaded f32 frame (tl3d_build_normals, ICP, fusion).
 * TL3D_E_STATE without a TSDF channel, and on a block (a grid with a voxel offset or a core: blocked ray casting does not
 * exist); TL3D_E_INVALID for a null pose or a slot >= n_slots.  No reference code: the reference has no TSDF. */
int tl3d_raycast(tl3d_ctx *ctx, const double R[9], const double t[3], int min_weight, double z_near, double z_far,
                 int slot, float *depth_out_hd, float *normal_out_hd, uint8_t *bgr_out_hd);

/* Point-to-SDF registration of a frame against the TSDF channel (no reference code: the reference has no
 * TSDF).  The residual of a sampled pixel of `slot` (f32 depth * scale, the context's depth range) is the trilinearly interpolated
 * signed distance at its back-projection under the world->camera pose (R, t), in metres; the analytic gradient of the field plays
 * the part of the normal; a sample is a correspondence when its cell is defined (all 8 voxels with weight >= max(1, min_weight),
 * as tl3d_raycast) and |F| <= min(max_dist / sdf_trunc, 0.98).  J = [p x n, n] for moving the camera-frame point: the same 6x6
 * normal equations as tl3d_icp_*.
 * tl3d_track_evaluate: ONE pass at (R, t), no update; sums laid out as tl3d_icp_evaluate_pairs gives them, bit for bit the same in
 * every run.  tl3d_track_frame: `levels` coarse to fine (iters, stride, max_dist as the gate, damping, eps, eig_rel;
 * estimate_scale must be 0), every iteration on the device, then a final pass at the result; out->T is the world->camera pose as a
 * row-major 4x4, out->scale echoes `scale`; status 2 (fewer than 8 correspondences or a singular system) leaves T at the last good
 * pose.  Both first issue pending TSDF batches and fold the free-space counts, are ordered behind uploads into the slot and block
 * for their result.  TL3D_E_STATE without a TSDF channel, on a block (voxel offset or core), for an empty slot and while an ICP
 * batch is uncollected; TL3D_E_INVALID for a bad slot, stride < 1, max_dist <= 0, n_levels outside 1..TL3D_ICP_MAX_LEVELS, a null pose. */
int tl3d_track_evaluate(tl3d_ctx *ctx, int slot, double scale, const double R[9], const double t[3], int min_weight, int stride,
                        double max_dist, tl3d_icp_eval *out);
int tl3d_track_frame(tl3d_ctx *ctx, int slot, double scale, const double R_init[9], const double t_init[3], int min_weight,
                     const tl3d_icp_params *levels, int n_levels, tl3d_icp_result *out);

/* f1: statistical outlier removal on a point list (Open3D remove_statistical_outlier, D2R:412-415): keep_out[i] = 1 when
 * 0 < mean_i < mu + std_ratio * sigma, with mean_i as tl3d_knn_mean_distance gives it and mu / sigma (Bessel-corrected) taken over
 * the points with mean_i > 0; *out_kept = the number of ones.  Host or device pointers for xyz and keep_out. */
int tl3d_statistical_outlier(tl3d_ctx *ctx, const float *xyz_hd, int64_t n, int nb_neighbors, double std_ratio,
                             double cell_size, uint8_t *keep_out_hd, int64_t *out_kept);

/* per point: mean fp64 distance to its nb_neighbors nearest neighbours (itself included, k clamped to n); the quantity
 * tl3d_statistical_outlier thresholds, from the same stage of the filter (no reference code: Open3D keeps it internal).  Host or
 * device pointers.  The same argument checks: nb_neighbors in [1,64], cell_size > 0, n == 0 is TL3D_OK.  cell_size only sets the
 * search grid (doubled until it has at most 2^27 cells); the result does not depend on it. */
int tl3d_knn_mean_distance(tl3d_ctx *ctx, const float *xyz_hd, int64_t n, int nb_neighbors, double cell_size, double *mean_out_hd);

/* Normals and surface variation of a point list by PCA over each point's k nearest neighbours (no reference
 * code: the reference's cloud carries positions and colours only -- the definition is Open3D's estimate_normals followed by
 * orient_normals_towards_camera_location, and PCL's surface variation).  Host or device pointers for xyz, normal_out [n][3] and
 * curvature_out [n] (may be NULL); viewpoints is a HOST array [m][3] (may be NULL with m = 0); out_degenerate may be NULL; no grid
 * is needed.
 * Neighbourhood of point i: the min(nb_neighbors, n) points that are smallest under the order (d^2, index), d^2 the fp64 sum of
 * squares of the fp64 differences of the f32 coordinates; the point itself is one of them and an exact tie goes to the smaller
 * index (the rule of tl3d_nearest_points).  max_radius > 0 then drops every member with d^2 > max_radius * max_radius (one fp64
 * product; a point exactly on the radius stays); max_radius <= 0: no limit.
 * Covariance, all in fp64, the k' members summed in their (d^2, index) order: e_j = p_j - p_i (exact), m = (sum e_j) / k',
 * C = sum (e_j - m)(e_j - m)^T (two passes, no division: scale does not matter).  That order is why the result is the same bytes
 * for every cell_size and in every run.
 * normal_out[i] = the unit eigenvector of C's smallest eigenvalue l0 (l0 <= l1 <= l2; cyclic Jacobi in fp64, accurate when two
 * eigenvalues are close), rounded to f32 at the end; curvature_out[i] = l0 / (l0 + l1 + l2) as f32, 0 when the sum is 0.
 * Degenerate: fewer than 3 members left, or l2 == 0 (all members coincide, C is exactly 0): normal (0,0,0), curvature 0, counted in
 * *out_degenerate.  A collinear neighbourhood is not degenerate: it gets some unit vector perpendicular to the line.
 * Orientation: with n_viewpoints > 0 point i looks at its nearest viewpoint c (nearest by (d^2, index) in fp64 over all of them);
 * the fp64 normal is negated before rounding when n . (c - p_i) < 0, and left as the unoriented call gives it when that is
 * exactly 0.  Without viewpoints the sign is unspecified, but the same in every run.
 * nb_neighbors in [3, 64]; cell_size > 0 only sets the search grid (doubled until it has at most 2^27 cells) and never changes a
 * result; n == 0 is TL3D_OK.  TL3D_E_INVALID before any device work, with nothing written: a null ctx, xyz or normal_out, n < 0 or
 * n >= 2^31, n_viewpoints < 0 (or > 0 with a null pointer), a non-finite viewpoint, an output that overlaps the input or the other
 * output; and from the device pass in front of the search, with nothing written: a non-finite coordinate.
 * Tests (tests/test_gpu_cloud_normals.py): sin(angle to an fp64 reference) <= 2^-22 + 1024 * 2^-52 * l2 / (l1 - l0) per point,
 * exact answers on lattices with ties, the same bytes for every cell size, for host and device arrays and in every run. */
int tl3d_estimate_normals(tl3d_ctx *ctx, const float *xyz_hd, int64_t n,
                          int nb_neighbors, double max_radius, double cell_size,
                          const double *viewpoints_h, int64_t n_viewpoints,
                          float *normal_out_hd, float *curvature_out_hd, int64_t *out_degenerate);

/* Planar regions of a point list with normals (no reference code: the reference never segments its cloud -- the
 * rules are ours: smoothness-constrained region growing as in PCL's RegionGrowing with a planarity test behind it, the question
 * Open3D's detect_planar_patches answers).  Host or device pointers for xyz [n][3], normal [n][3], curvature [n] (may be NULL),
 * plane_id_out [n] and planes_out [plane_cap] (may be NULL with plane_cap 0); params and out_counts [4] are host memory; no grid
 * is needed.  All arithmetic is fp64 on the f32 inputs converted exactly, plain products and sums in x, y, z order.
 * Eligible point: the squared length of its normal is finite and > 0; with a curvature array and max_curvature > 0 also
 * curvature <= max_curvature (a NaN compares false: not eligible).
 * Link between eligible i != j (symmetric), when all of: d^2 = dx dx + dy dy + dz dz <= radius * radius (one product; a pair exactly
 * on the radius is linked); s = n_i . n_j, |s| unless signed_normals, s >= min_cos; |n_i . (p_j - p_i)| <= max_offset and
 * |n_j . (p_i - p_j)| <= max_offset.
 * Region: a connected component of the link graph over the eligible points; its label is its smallest point index (its seed).  The
 * partition is a function of the point SET; only the numbering follows the input order.
 * Moments of a region with count >= min_points, about its seed: Q(x) = llrint(x * 2^20), e = Q(p) - Q(p_seed); the sums count,
 * sum e (3), sum e_a e_b (6, 128-bit) and sum N with N = llrint(n * 2^20) (3; a normal component beyond +-2^11 is clamped to it)
 * are exact integers, so their order is free and every run gives the same sums.  (sum e and sum N are kept in 64 bits; the call
 * refuses a cloud where sum e might not fit: n * (E * 2^20 + 1) must stay below 2^62, E the largest extent of the points' box in
 * metres -- 2^31 points over 2 km, 2^20 points over 4 000 km.)
 * Plane of a region, one fixed fp64 sequence on those sums: m = sum e / count, C_ab = sum e_a e_b - sum e_a * sum e_b / count;
 * l0 <= l1 <= l2 and the unit eigenvector of l0 by cyclic Jacobi; the normal is negated when normal . sum N < 0 and left as it is
 * when that is 0; centroid = (Q(p_seed) + m) * 2^-20, d = normal . centroid, rms = sqrt(max(l0, 0) / count) * 2^-20.
 * Accepted as a plane: count >= min_points, l2 > 0 and (max_rms <= 0 or rms <= max_rms).  Accepted planes are numbered 0 .. P-1 in
 * ascending label; plane_id_out[i] = the number of i's accepted plane, else -1 (ineligible points, small regions, rejected regions).
 * out_counts = {eligible points, regions, regions with count >= min_points, planes}.  plane_cap < planes: TL3D_E_CAPACITY with the
 * four counts stored and plane_id_out written, but no plane record.  cell_size > 0 only sets the search grid (doubled until it has
 * at most 2^27 cells) and never changes a result; n == 0 is TL3D_OK.  A gently curved surface grows into ONE region, which max_rms
 * then rejects; planes that meet at a crease are kept apart by max_curvature on the crease's blended normals.
 * TL3D_E_INVALID before any device work, with nothing written: a null ctx, xyz, normal, params, plane_id_out or out_counts (or
 * planes_out with plane_cap > 0), n < 0 or n >= 2^31, plane_cap < 0, radius not finite or <= 0, min_cos outside [0, 1] or NaN, a
 * negative or NaN max_offset, min_points < 3, cell_size not > 0, reserved != 0, an output that overlaps an input or the other
 * output; and from the device pass in front of the index, with nothing written: a non-finite coordinate, |x| >= 2^22 m, or
 * n * (E * 2^20 + 1) >= 2^62.
 * Tests (tests/test_gpu_plane_segments.py): plane_id, the counts and every plane's count and seed equal two numpy / scipy
 * formulations exactly on crafted clouds, decision edges one f32 ulp apart and union-find topologies; the same bytes for every cell
 * size, for host and device arrays and in every run; the plane parameters within a derived bar of the exact sums' answer. */
typedef struct tl3d_plane_params {
    double radius, min_cos, max_offset, max_curvature, max_rms;
    int64_t min_points;
    int32_t signed_normals;
    int32_t reserved;
} tl3d_plane_params;
typedef struct tl3d_plane {
    double normal[3];
    double d;
    double centroid[3];
    double rms;
    int64_t count;
    int64_t seed;
} tl3d_plane;
int tl3d_segment_planes(tl3d_ctx *ctx, const float *xyz_hd, const float *normal_hd, const float *curvature_hd, int64_t n,
                        const tl3d_plane_params *params, double cell_size,
                        int32_t *plane_id_out_hd, tl3d_plane *planes_out_hd, int64_t plane_cap, int64_t *out_counts /* [4] */);

/* Exact nearest neighbours from one set to ANOTHER (no reference code: the reference never scores a cloud -- the
 * definition is Open3D's compute_point_cloud_distance).  Per query point q: dist_out[q] = the fp64 distance to the nearest target
 * point (differences of the f32 coordinates, squares and their sum in fp64, one correctly rounded root) and index_out[q] = its index;
 * the winner is the minimum over the pair (d^2, index), so an exact tie goes to the smaller index and nothing depends on the order
 * the search meets the points in.  Host or device pointers throughout; either output may be NULL; no grid is needed.
 * cell_size only sets the search grid over the target's box (doubled until it has at most 2^27 cells) and never changes a result;
 * cell_size <= 0: (V / (4 n_target))^(1/k) with V the product of the box's k non-zero extents (1 for a box without extent).
 * max_dist <= 0: unlimited; otherwise a query with nothing at distance <= max_dist gets +inf and -1.  An empty target gives +inf / -1
 * for every query and TL3D_OK; n_query == 0 is TL3D_OK.  Queries may lie anywhere, far outside the target's box included.
 * TL3D_E_INVALID before any device work: a null ctx, negative sizes, n_target >= 2^31, an output that overlaps an input (or the
 * other output); and from a device pass in front of the search, with nothing written: a non-finite coordinate in either set.
 * Tests (tests/test_gpu_nearest.py): distances within 1e-12 relative of an fp64 brute force and exactly 0 where it is 0, the index
 * the smallest-index minimiser on exact ties, the same bytes for every cell size, for host and device arrays and in every run. */
int tl3d_nearest_points(tl3d_ctx *ctx, const float *query_hd, int64_t n_query,
                        const float *target_hd, int64_t n_target, double cell_size, double max_dist,
                        double *dist_out_hd, int32_t *index_out_hd);

/* The same against an indexed triangle list: dist_out[q] = the fp64 distance from q to the nearest point of the nearest CLOSED
 * triangle (the plane distance where the foot of the perpendicular lies inside, else the minimum over the three closed edges),
 * tri_out[q] = that triangle, the smaller index on an exact tie.  Triangles with collinear or repeated corners are segments or
 * points and measure as such (never NaN).  A triangle is listed in every cell its box overlaps; the cell doubles until that list
 * has at most min(16 n_tri + 2^20, 2^31) entries, so one triangle across the whole box beside thousands of small ones costs memory
 * in proportion to n_tri.  cell_size <= 0: the mean over the triangles of their box's largest extent.  Everything else as
 * tl3d_nearest_points, with n_vert and n_tri < 2^31 and, from the device pass, TL3D_E_INVALID for a triangle index >= n_vert
 * (compared before it is used) and for a non-finite vertex.  Unreferenced vertices only widen the search grid.
 * Tests: within 16 eps_tri x the box diagonal of an fp64 reference held against a long-double second formulation. */
int tl3d_nearest_triangles(tl3d_ctx *ctx, const float *query_hd, int64_t n_query,
                           const float *xyz_hd, int64_t n_vert, const uint32_t *tri_hd, int64_t n_tri,
                           double cell_size, double max_dist, double *dist_out_hd, int32_t *tri_out_hd);

/* Summary of a distance array (host or device): n, the finite entries, their sum, sum of squares and maximum (0 without one), and
 * per threshold t_j (at most 8) the entries <= t_j.  Fixed reduction shape (1024 block partials added in block order): the same
 * input gives the same bytes in every run; the counts and the maximum are exact.  +inf entries (queries beyond max_dist) are no
 * finite entries and lie under no finite threshold.  TL3D_E_INVALID: null ctx / out, n < 0, more than 8 thresholds.
 * The struct is tl3d_distance_stats: C has one name space for typedefs and functions. */
typedef struct tl3d_distance_stats {
    int64_t n;
    int64_t n_finite;
    double  sum;
    double  sum_sq;
    double  max;
    int64_t below[8];
} tl3d_distance_stats;
int tl3d_distance_summary(tl3d_ctx *ctx, const double *dist_hd, int64_t n,
                          const double *thresholds, int n_thresholds, tl3d_distance_stats *out);

/* Queries of the two searches run bucketed by the target grid's cell, so that the lanes of a wave read the same few cells, and
 * scatter their results back by original index (default).  cell_order = 0: in input order.  The results are the same bytes. */
int tl3d_set_nearest_query_order(tl3d_ctx *ctx, int cell_order);

/* ---- registration of two unorganised point clouds: ICP over the cell index, optionally with scale ------
 * One pass at the pose (T, scale), every operation fp64 and rounded once, in this order (tests/cloud_register_reference.py
 * restates it bit for bit).  For every sampled source point p (index i with i % stride == 0; f32 -> fp64):
 *   m = R p, m_x = (R00 px + R01 py) + R02 pz ...;  w = scale * m;  q = w + t              (q is never rounded to f32)
 *   y = the target point minimising (d2, index), d = y - q, d2 = dx dx + dy dy + dz dz      (tl3d_nearest_points' rule: an exact
 *       tie goes to the smaller index); the pair is kept iff sqrt(d2) <= max_dist (max_dist <= 0: unlimited)
 *   point-to-plane (target normals given): n = the normal of y; a correspondence whose normal is exactly (0, 0, 0) is dropped and
 *       counted in n_no_normal; r = (n_x e_x + n_y e_y) + n_z e_z with e = q - y; J = [q x n, n, n . w] (the last with scale only)
 *   point-to-point (normals NULL): three rows per correspondence, n = e_x, e_y, e_z in that order, the same expressions
 *   A += J_i J_j (upper triangle), b += J_i r, e += r r; n_corr counts correspondences, n_src the sampled points.
 * The sums have a fixed shape that depends on n_src alone: they, and the pose of tl3d_cloud_register, are the same bytes in every
 * run, for every cell_size and under either setting of tl3d_set_nearest_query_order.  index_out[i] = the index of y, or -1 where
 * the pair was gated, the target is empty or the point was not sampled.  cell_size as tl3d_nearest_points (the target's grid). */
typedef struct tl3d_cloud_eval {
    double  A[28];              /* upper triangle of the 7 x 7 matrix, row-major; without with_scale row and column 6 are 0 */
    double  b[7];
    double  e;
    int64_t n_corr;
    int64_t n_src;
    int64_t n_no_normal;
} tl3d_cloud_eval;
/* TL3D_E_INVALID before any device work: null ctx / source / target (with points) / T / out, negative sizes, n_tgt or n_src >= 2^31,
 * stride < 1, a non-finite T or scale; from the bounds pass, with nothing written: a non-finite coordinate.  TL3D_E_STATE while an
 * ICP batch is uncollected.  n_src == 0 or n_tgt == 0: zero sums (n_src still counts the sampled points), every index -1. */
int tl3d_cloud_evaluate(tl3d_ctx *ctx, const float *src_hd, int64_t n_src, const float *tgt_hd, int64_t n_tgt,
                        const float *tgt_normals_hd /* NULL: point-to-point */, const double T[16], double scale, int stride,
                        double max_dist, double cell_size, int with_scale, tl3d_cloud_eval *out,
                        int32_t *index_out_hd /* may be NULL, [n_src] */);
/* Gauss-Newton over such passes: per iteration solve (A + damping tr(A)/k I) x = -b under the relative eigenvalue cutoff (k = 6,
 * or 7 with estimate_scale), T <- exp(x) T, scale <- scale exp(x[6]).  A pass with fewer than 6 correspondences or an unsolvable
 * system fails the run (status 2, T the last good pose); |x|_max < eps ends a level (status 1); a level that failed or ended with
 * fewer than 8 correspondences ends the run.  The target's index is built once; every level and iteration is enqueued without a
 * host round trip and the state is read once.  out->T maps source to target and holds the rigid part, out->scale is sigma, n_src
 * the sampled points of the last level.  Empty source or target: status 2, T = T_init.  Refusals as tl3d_cloud_evaluate, and
 * n_levels outside 1..TL3D_ICP_MAX_LEVELS, iters outside [0, 1000], a max_dist that is not positive. */
int tl3d_cloud_register(tl3d_ctx *ctx, const float *src_hd, int64_t n_src, const float *tgt_hd, int64_t n_tgt,
                        const float *tgt_normals_hd, const double T_init[16], double scale_init,
                        const tl3d_icp_params *levels, int n_levels, double cell_size, tl3d_icp_result *out);

/* ---- global registration of two clouds: the front end that finds a start for tl3d_cloud_register ------------
 * Four calls: subsample, FPFH descriptors, nearest-feature correspondences, RANSAC over three-correspondence samples.  Host or
 * device pointers throughout (params, the result and the out_* words are host memory); no grid is needed.  All arithmetic is fp64 on
 * the f32 inputs converted exactly, every operation rounded once, dot products and squared lengths summed in x, y, z order
 * ((a + b) + c); tests/cloud_global_reference.py restates every sequence.  Every result is the same bytes in every run.
 *
 * Voxel subsample.  cell = floor(x / voxel) per axis (fp64 division), a lattice through (0, 0, 0); of every occupied voxel the member
 * with the smallest index is kept.  index_out [n] receives the kept indices ascending (entries behind *out_n are not written),
 * *out_n their number: a subset, so normals and colours follow by indexing.  n == 0 is TL3D_OK with *out_n = 0.
 * TL3D_E_INVALID before any device work: a null ctx, xyz (with n > 0), index_out or out_n, n < 0 or n >= 2^31, a voxel that is not
 * finite and > 0, an output that overlaps the input; from the bounds pass, with nothing written: a non-finite coordinate, or a
 * cell with |cell| >= 2^20 on any axis (the three cells make one 63-bit key). */
int tl3d_cloud_voxel_subsample(tl3d_ctx *ctx, const float *xyz_hd, int64_t n, double voxel, int32_t *index_out_hd, int64_t *out_n);

/* FPFH (Rusu et al. 2009; the pair feature is PCL's and Open3D's).  Neighbourhood N(i): the list tl3d_estimate_normals builds for the
 * same nb_neighbors (clamped to n) and max_radius (<= 0: none) -- the k smallest under (d2, index), then the members with
 * d2 <= max_radius^2 -- less the members with d2 == 0 (the point itself, duplicates) and the members whose normal is exactly (0, 0, 0).
 * Pair feature of (i, j), j in N(i), in list order: d = p_j - p_i, L = sqrt(d2), a1 = (n_i . d) / L, a2 = (n_j . d) / L.  When
 * |a1| < |a2|: (ns, nt, d, f3) = (n_j, n_i, -d, -a2); otherwise (n_i, n_j, d, a1).  v = d x ns; a pair with |v| == 0 is skipped;
 * v /= |v| (three divisions by sqrt(v . v)), w = ns x v, f2 = v . nt, f1 = atan2(w . nt, ns . nt).  Bins: b1 = clamp(floor(11 (f1 + pi)
 * / (2 pi)), 0, 10), b2 = clamp(floor(11 (f2 + 1) / 2), 0, 10), b3 likewise from f3, each product before its division.  Normals are
 * taken as given: they are not renormalised and their SIGN MATTERS (orient them by a rule that moves with the cloud).
 * SPFH of i: the 33 integer counts c_i (b1, 11 + b2, 22 + b3 per counted pair) and the number of counted pairs m_i; the spfh_out row
 * is c_i[0..32], m_i.  A point whose normal is (0, 0, 0) counts nothing.  A point with m_i == 0 has an all-zero FPFH row.  Otherwise
 * S[b] = sum over j in N(i) with m_j > 0, in list order, of (100 c_j[b] / m_j) / d2_ij; each group of 11 bins with a sum > 0 (added in
 * bin order) is multiplied by 100 / sum; F_i[b] = S[b] + 100 c_i[b] / m_i, rounded to f32 once.  Counts are exact and the fp64 sums
 * run in the list's order: the bytes do not depend on cell_size (> 0; it only sets the search grid), fill order or run.
 * nb_neighbors in [4, 64]; n == 0 is TL3D_OK.  TL3D_E_INVALID before any device work: a null ctx, xyz, normals or fpfh_out, n < 0 or
 * n >= 2^31, nb_neighbors or cell_size out of range, a NaN max_radius, outputs that overlap an input or each other; from the bounds
 * pass, with nothing written: a non-finite coordinate.  Normals must be finite. */
int tl3d_cloud_fpfh(tl3d_ctx *ctx, const float *xyz_hd, const float *normals_hd, int64_t n, int nb_neighbors, double max_radius,
                    double cell_size, float *fpfh_out_hd /* [n][33] */, int32_t *spfh_out_hd /* [n][34], may be NULL */);

/* Nearest feature.  For every row of a [n_a][dim] the row of b [n_b][dim] minimising (d2, index): d2 = the fp64 sum over
 * c = 0 .. dim - 1, in that order, of the squared fp64 difference; an exact tie goes to the smaller index.  index_out [n_a] and
 * dist2_out [n_a] (either may be NULL); n_b == 0 gives -1 and +inf; a row none of whose distances is finite (an infinite or
 * NaN feature) gets index 0 and +inf.  Brute force on purpose (33 dimensions defeat a cell grid): the
 * call is refused when n_a * n_b > 2^34 -- a safety condition for a shared device, not a tuning value; subsample first.
 * TL3D_E_INVALID before any device work: a null ctx, a null a or b with rows, negative sizes, n_a or n_b >= 2^31, dim outside
 * [1, 64], n_a * n_b > 2^34, an output that overlaps an input or the other output. */
int tl3d_feature_match(tl3d_ctx *ctx, const float *feat_a_hd, int64_t n_a, const float *feat_b_hd, int64_t n_b, int dim,
                       int32_t *index_out_hd, double *dist2_out_hd);

/* RANSAC over correspondences corr [m][2] = (source index, target index).  Hypothesis h = 0 .. n_hypotheses - 1 draws the three
 * correspondence numbers i_j = mix(seed + 0x9E3779B97F4A7C15 * (3 h + j + 1)) mod m, j = 0, 1, 2, in wrapping u64 arithmetic; mix is
 * the finaliser of MurmurHash3 (x ^= x >> 33; x *= 0xFF51AFD7ED558CCD; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53; x ^= x >> 33).
 * Rejected (count -1) when two draws coincide; when for any of the point pairs (0,1), (1,2), (2,0) the source and target edge lengths
 * ls, lt (sqrt of the squared length) have max == 0 or min(ls, lt) < edge_ratio * max(ls, lt); or when either triad is degenerate.
 * Triad of three points, for source and target alike: x = (p1 - p0) / |p1 - p0|, z = x x (p2 - p0), degenerate unless |z| > 0,
 * z /= |z|, y = z x x.  R_ij = (xt_i xs_j + yt_i ys_j) + zt_i zs_j; t = mt - R ms with the means ((p0 + p1) + p2) / 3.  No SVD.
 * Score: the number of correspondences k with |(R s_k + t) - t_k|^2 <= max_dist * max_dist (one product on the right; a pair exactly
 * on the threshold counts).  Winner: the maximum over (count, -h) -- the most inliers, the smaller h on a tie.
 * status 1: a winner; status 2, T = I, best_h -1: nothing passed (m < 3 included).  count_out [n_hypotheses]
 * (may be NULL): every hypothesis' count, or -1.  The edge-length test assumes ONE scale for both clouds.
 * TL3D_E_INVALID before any device work: null ctx / params / out, null clouds or corr with entries, negative sizes, sizes >= 2^31,
 * n_hypotheses outside [1, 2^24], a max_dist that is not finite and > 0, an edge_ratio outside [0, 1], reserved != 0, a count_out
 * that overlaps an input; from the device passes in front of the draw, with nothing written: a non-finite coordinate, a
 * correspondence that names a point outside its cloud. */
typedef struct tl3d_ransac_params {
    int64_t  n_hypotheses;
    double   max_dist;
    double   edge_ratio;        /* 0.9 is the usual value */
    uint64_t seed;
    int64_t  reserved;
} tl3d_ransac_params;
typedef struct tl3d_ransac_result {
    double  T[16];              /* row-major, maps source to target */
    int64_t best_h;
    int64_t inliers;
    int64_t n_passed;           /* hypotheses that were scored */
    int64_t m;
    int32_t status;
    int32_t reserved;
} tl3d_ransac_result;
int tl3d_cloud_ransac(tl3d_ctx *ctx, const float *src_hd, int64_t n_src, const float *tgt_hd, int64_t n_tgt,
                      const int32_t *corr_hd, int64_t m, const tl3d_ransac_params *params, tl3d_ransac_result *out,
                      int32_t *count_out_hd);

/* measurement */
int tl3d_set_profile(tl3d_ctx *ctx, int count_records, int time_kernels);
/* Noise-robust registration: normal maps built after this call come from the depth averaged over a (2 radius + 1)^2 window
 * -- the HARMONIC mean (mean of 1 / z, which is linear in the pixel coordinates on any plane) over the centre pixel and the
 * pixel pairs (u + du, v + dv), (u - du, v - dv) that are both valid and within depth_jump of the centre (a symmetric set: no
 * average runs across a depth edge, and none is pulled to one side at the edge of a surface) -- with the tangent vectors
 * `radius` pixels to either side; registrations then read that averaged depth as their SOURCE too (tl3d_icp_*: a slot whose
 * normal map was built smoothed).  0 (default) = central differences of the depth image itself.  With 1 mm of depth noise the
 * frame-to-frame chain of config 2 drifts 7 x less at radius 1 (tests/test_gpu_baseline_configs.py). */
int tl3d_set_normal_smoothing(tl3d_ctx *ctx, int radius);

/* tl3d_integrate collects up to 32 frames per update launch (the bricks they see are read and written once for all of them;
 * the grid is the same bit for bit).  on = 0: one frame per launch.  Default: on. */
int tl3d_set_tsdf_pairing(tl3d_ctx *ctx, int on);
/* The TSDF prep keeps what it derives from a frame's depth image alone (depth tiles, their pyramid, one valid pixel: functions
 * of the image, the scale and the depth limits) with the frame's slot, and builds it again only after a new frame went into
 * the slot or when one of those parameters differs: a frame fused a second time (another scan, another block of a blocked
 * grid, tl3d_count_bricks followed by the fusion) skips that pass.  builds: per-frame builds so far; hits: look-ups that
 * found the slot's tiles usable; bytes: device memory the tiles hold (about 0.95 MB per 1080 x 1920 slot, taken on first
 * use).  Any of the three may be null; the pending batch is issued first (look-ups happen then).  With TL3D_TILE_CACHE=0 in the environment when the context is created every look-up
 * is a miss (the tiles are built once per batch, as before the cache existed). */
int tl3d_tile_cache_info(tl3d_ctx *ctx, uint64_t *builds, uint64_t *hits, uint64_t *bytes);
/* Beside the tiles a slot keeps the RESULT of the TSDF prep's brick and sub-brick classification for the last (pose, scale, depth
 * limits, grid geometry) it was fused or counted with: the bricks near a surface with their sub-brick masks and the free-space
 * bricks.  A batch that meets the slot again with exactly that key (compared bit for bit, the pose as the twelve f32 words the
 * kernels get) replays the lists instead of classifying: another scan over resident frames with fixed poses, a fusion after
 * tl3d_grid_reset, tl3d_count_bricks followed by the fusion.  One entry per slot; a new image, a ray cast into the slot or
 * another key replaces it.  The grid is the same bit for bit either way.  classified / replayed: frames that went through the
 * classification kernels / whose entry was replayed; overflowed: of the classified, those whose bricks did not fit the slot's
 * buffer (never replayed); bytes: device memory the entries hold (288 KB per slot by default, taken on first use).  Any of the
 * four may be null; the pending batch is issued first and the call waits for the device.  Environment, read when the context is
 * created: TL3D_CLASS_CACHE=0 every frame is classified; TL3D_CLASS_CACHE_ENTRIES=n bricks per slot buffer (default 49152, 6 B
 * each); TL3D_TILE_CACHE=0 switches this cache off too. */
int tl3d_class_cache_info(tl3d_ctx *ctx, uint64_t *classified, uint64_t *replayed, uint64_t *overflowed, uint64_t *bytes);
/* The first fusion batch that replays a slot's entry (and holds the slot once; at most 8 entries per batch, the others at their
 * next replay) REFINES its sub-brick masks: every sub-brick the
 * entry lists as near a surface is put through the update's own per-voxel test against the 8x8-pixel depth tiles, once, and the
 * ones that test decides for all 64 voxels leave the update's work for good -- all behind every surface: dropped; all in free
 * space in front of every surface: counted as free space.  Later replays of the entry use the refined masks.  A frame that is
 * fused once pays nothing; the grid is the same bit for bit.  Counts of (frame, sub-brick) pairs over the context's life:
 * seen: put through the test; dropped / freed: decided as above; decided: every voxel decided, some one way and some the other
 * (kept: a mask bit cannot say which voxel is which); overflowed: always 0 (reserved for per-voxel masks that did not fit).
 * Any of the five may be null; the pending batch is issued first and the call waits for the device.  Environment, read when the
 * context is created: TL3D_CLASS_REFINE=0 nothing is refined; so with TL3D_CLASS_CACHE=0 or TL3D_TILE_CACHE=0. */
int tl3d_class_refine_info(tl3d_ctx *ctx, uint64_t *seen, uint64_t *dropped, uint64_t *freed, uint64_t *decided, uint64_t *overflowed);
int tl3d_get_stats(tl3d_ctx *ctx, tl3d_stats *out);
int tl3d_reset_stats(tl3d_ctx *ctx);
int tl3d_event_record(tl3d_ctx *ctx, int which /* 0 or 1 */);
int tl3d_event_elapsed_ms(tl3d_ctx *ctx, float *ms);      /* time between event 0 and event 1, blocks */

#ifdef __cplusplus
}
#endif
#endif /* TL3D_H */
