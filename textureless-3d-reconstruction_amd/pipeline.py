"""DepthToReconstructionPipeline: the reference's orchestration (depth_to_reconstruction.py:423-703) with the
SfM pose front end replaced by on-device point-to-plane ICP and the vstack + Open3D merge replaced by on-device
voxel fusion.

Kept from the reference: load_data()'s file rules and messages, cam0 = (I, 0), the pose chain
R_c = R_rel R_prev, t_c = R_rel t_prev + t_rel (D2R:618-620), frames whose registration fails are skipped and
do not extend the pose list (D2R:598-615), subsample_factor / voxel_size semantics, the progress lines
(`Camera i: n points`, `Final reconstruction: ...`), save_reconstruction().
Not kept (out of scope): SIFT / essential-matrix poses; the sparse
triangulation that feeds estimate_scale -- depth is taken as metric (scale = config.depth_scale), which is
what D2R itself falls back to (D2R:555-558).
"""
from __future__ import annotations

from collections import defaultdict
from typing import List, Optional, Tuple

import os
import time

import numpy as np

from . import _cabi as abi
from . import fileio
from .config import ReconstructionConfig
from .dense import DenseReconstructor
from .fusion import FusionContext, GridSpec
from .lattice import (MAX_BLOCK_VOXELS, Block, _make_block, align_grid_to_open3d, layout_from_counts, plan_blocks,  # noqa: F401
                      plan_grid, plan_lattice, split_block, weld_meshes)


def compose(r_rel, t_rel, r_prev, t_prev):
    """D2R:619-620."""
    r_rel = np.asarray(r_rel, np.float64)
    return r_rel @ np.asarray(r_prev, np.float64), r_rel @ np.asarray(t_prev, np.float64).reshape(3, 1) + np.asarray(t_rel, np.float64).reshape(3, 1)


def relative_prior(init_poses, a, b):
    """The 4x4 that takes frame a's camera coordinates to frame b's, from the two absolute priors: R = R_b R_a^T, t = t_b - R t_a."""
    (ra, ta), (rb, tb) = init_poses[a], init_poses[b]
    rr = np.asarray(rb) @ np.asarray(ra).T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rr, (np.asarray(tb).reshape(3) - rr @ np.asarray(ta).reshape(3))
    return T


DENSE_WITHOUT_ASKING = 1 << 30        # bytes: below this a dense grid is allocated (and cleared) faster than its occupancy is counted


def choose_layout(ctx: FusionContext, grid: GridSpec, slots, poses, scales, centroid_subsample, dist=None, log=print) -> GridSpec:
    """Dense or sparse, from what the frames will really touch (tl3d_count_bricks: the fusion's own classification, no records).

    The reference's merge is a hash map over occupied voxels (D2R:404-410): memory follows the surfaces, whatever the extent.
    Here a grid is allocated (and cleared) before the first frame is fused, so its layout is a decision -- taken from a count, not
    from the extent.  Small grids are dense without asking.  With `dist` (reconstruct_sharded) every rank counts its own frames and
    all take the SUM (an upper bound of the union the merge will bring to every rank), so that all ranks choose alike."""
    nbr = grid.nvox // 512
    dense = GridSpec(grid.dims, grid.origin, grid.voxel_size, grid.sdf_trunc, grid.channels, voxel_offset=grid.voxel_offset)
    if dense.device_bytes() <= DENSE_WITHOUT_ASKING:
        return dense
    nt, nc = ctx.count_bricks(grid, slots, poses, scales, centroid_subsample=centroid_subsample) if len(slots) else (0, 0)
    if dist is not None:
        from . import distributed as dd
        nt, nc = dd.allreduce_counts([nt, nc], dist)
    out = layout_from_counts(grid, nt, nc)
    log(f"  Occupancy: {nt} TSDF bricks, {nc} centroid bricks of {nbr}: "
        f"{'sparse' if out.sparse else 'dense'} volume, {out.device_bytes() / 2**30:.2f} GiB (dense: {dense.device_bytes() / 2**30:.2f} GiB)")
    return out


BLOCK_MEMORY_MARGIN = 2 << 30         # device bytes a block leaves free for the fusion, extraction and mesh scratch


def device_free_bytes(device: int) -> int:
    """Free device memory (hipMemGetInfo of the HIP runtime libtl3d.so runs on: no second runtime, no torch context)."""
    import ctypes as C
    lib = abi.load()
    free, total = C.c_size_t(0), C.c_size_t(0)
    if lib.hipSetDevice(int(device)) != 0 or lib.hipMemGetInfo(C.byref(free), C.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(free.value)


class ScaleTracker:
    """The reference's depth-scale bookkeeping (row f3), with the anchor source left to the caller.

    depth_to_reconstruction.py estimates, per view, the median of Z_anchor / depth[pixel] over sparse anchors
    (estimate_scale, D2R:297-326), averages the first two views (D2R:552-554) and then runs
    avg = 0.7 * avg + 0.3 * scale_i (D2R:650); views without enough anchors keep the running value (D2R:645-647).
    In the reference the anchors are triangulated SIFT matches -- the SfM front end that ICP replaces here -- so
    they are an input: any sparse metric source (fiducials, a laser range, an external SLAM map) can provide
    {frame_index: (points3d [n,3], pixels [n,2])}.  Without anchors the depth is taken as metric (D2R:555-558)."""

    def __init__(self, default: float = 1.0):
        self.avg = float(default)
        self.history = []

    def first_pair(self, s0: float, s1: float) -> float:
        self.avg = (s0 + s1) / 2
        self.history = [self.avg, self.avg]
        return self.avg

    def update(self, scale_i=None, weight: float = 0.3) -> float:
        """D2R:650 with weight = 0.3; weight = 1 takes every view's own estimate as it comes."""
        if scale_i is not None:
            self.avg = (1.0 - weight) * self.avg + weight * scale_i
        self.history.append(self.avg)
        return self.avg


def per_frame_scales(depths, anchors, default: float = 1.0, fetch=None):
    """Scale of every frame from sparse anchors, exactly as the reference sequences it.  `fetch(i)` returns frame i's
    depth map when `depths[i]` is not held on the host (streaming)."""
    from .dense import estimate_scale_d2r
    n = len(depths)
    tr = ScaleTracker(default)
    if not anchors:
        return [float(default)] * n

    def depth_of(i):
        return depths[i] if depths[i] is not None else fetch(i)

    def est(i):
        if i not in anchors:
            return None
        p3, p2 = anchors[i]
        if len(p3) < 3:
            print("  Warning: Not enough valid points for scale, using previous")
            return None
        return estimate_scale_d2r(np.asarray(p3), np.asarray(p2), depth_of(i))

    s0, s1 = est(0), est(1) if n > 1 else None
    if s0 is not None and s1 is not None:
        tr.first_pair(s0, s1)
    else:
        print("Warning: Not enough sparse points for scale estimation")
        tr.history = [tr.avg, tr.avg]
    print(f"Average scale: {tr.avg:.6f}")
    for i in range(2, n):
        tr.update(est(i))
    return tr.history[:n]


def check_cloud_options(cfg):
    """config.cloud_planes: what reconstruct() refuses before any work"""
    if not bool(getattr(cfg, "cloud_planes", False)):
        return
    if not bool(getattr(cfg, "cloud_normals", False)):
        raise ValueError("cloud_planes segments the cloud by its normals: it needs cloud_normals = True")
    for name in ("cloud_planes_radius", "cloud_planes_offset", "cloud_planes_max_curvature", "cloud_planes_max_rms"):
        v = float(getattr(cfg, name))
        if not np.isfinite(v) or v < 0.0:
            raise ValueError(f"{name} = {v}: must be finite and not negative (0: the default)")
    angle = float(cfg.cloud_planes_angle_deg)
    if not 0.0 <= angle <= 90.0:                        # (false for NaN)
        raise ValueError(f"cloud_planes_angle_deg = {angle}: must lie in [0, 90]")
    m = cfg.cloud_planes_min_points
    if isinstance(m, bool) or int(m) != m or int(m) < 3:
        raise ValueError(f"cloud_planes_min_points = {m}: must be a whole number, 3 at the least")


def cloud_plane_parameters(cfg, voxel_size=None) -> dict:
    """config.cloud_planes_* as FusionContext.segment_planes takes them, lengths in metres: a length of 0 is 2.5 voxels for the
    radius, 1 voxel for the offset and 0.5 voxel for the rms"""
    voxel = float(cfg.voxel_size if voxel_size is None else voxel_size)
    return dict(radius=float(cfg.cloud_planes_radius) or 2.5 * voxel, max_angle_deg=float(cfg.cloud_planes_angle_deg),
                max_offset=float(cfg.cloud_planes_offset) or voxel, max_curvature=float(cfg.cloud_planes_max_curvature),
                min_points=int(cfg.cloud_planes_min_points), max_rms=float(cfg.cloud_planes_max_rms) or 0.5 * voxel)


def load_alignment_matrix(init):
    """compare_align_init as a finite 4 x 4 float64 matrix: an array, or the path of a .npy or text file holding one."""
    if isinstance(init, (str, os.PathLike)):
        path = os.fspath(init)
        try:
            init = np.load(path) if path.lower().endswith(".npy") else np.loadtxt(path)
        except (OSError, ValueError) as e:
            raise ValueError(f"compare_align_init: cannot read a matrix from {path!r} ({e})") from e
    T = np.asarray(init, dtype=np.float64)
    if T.shape != (4, 4) or not np.all(np.isfinite(T)):
        raise ValueError(f"compare_align_init: a finite 4 x 4 matrix is needed, got shape {T.shape}")
    return np.ascontiguousarray(T)


def check_compare_options(cfg):
    """The configuration's compare_align settings: refused with a message before any work.  Returns the initial matrix (or None)."""
    align = bool(getattr(cfg, "compare_align", False))
    scale = bool(getattr(cfg, "compare_align_scale", False))
    init = getattr(cfg, "compare_align_init", None)
    glob = bool(getattr(cfg, "compare_align_global", False))
    gvoxel = getattr(cfg, "compare_align_global_voxel", None)
    if (scale or init is not None) and not align:
        raise ValueError("compare_align_scale / compare_align_init set how compare_align registers: they need compare_align = True")
    if (glob or gvoxel is not None) and not align:
        raise ValueError("compare_align_global / compare_align_global_voxel set where compare_align starts: they need compare_align = True")
    if gvoxel is not None and not glob:
        raise ValueError("compare_align_global_voxel is the global start's voxel: it needs compare_align_global = True")
    if glob and init is not None:
        raise ValueError("compare_align_global finds the start itself: it cannot be combined with compare_align_init")
    if glob and scale:
        raise ValueError("compare_align_global is rigid only (the RANSAC's edge-length test assumes one scale): it cannot be combined "
                         "with compare_align_scale")
    if gvoxel is not None and not (np.isfinite(float(gvoxel)) and float(gvoxel) > 0):
        raise ValueError(f"compare_align_global_voxel must be finite and positive, got {gvoxel!r}")
    if not align:
        return None
    if not getattr(cfg, "compare_to", None):
        raise ValueError("compare_align registers the result onto the reference scan: it needs compare_to")
    return None if init is None else load_alignment_matrix(init)


def check_depth_filter_options(cfg):
    """config.depth_filter: what reconstruct() refuses before any work (the ranges of tl3d_filter_depth_slots)"""
    if not bool(getattr(cfg, "depth_filter", False)):
        return
    jump = float(cfg.depth_filter_jump)
    if not (np.isfinite(jump) and jump > 0.0):
        raise ValueError(f"depth_filter_jump = {jump}: must be finite and positive")
    ints = {}
    for name in ("depth_filter_radius", "depth_filter_min_support", "depth_filter_min_region"):
        v = getattr(cfg, name)
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} = {v}: must be a whole number")
        ints[name] = int(v)
    r = ints["depth_filter_radius"]
    if not 1 <= r <= 3:
        raise ValueError(f"depth_filter_radius = {r}: must lie in [1, 3]")
    top = (2 * r + 1) ** 2 - 1
    if not 0 <= ints["depth_filter_min_support"] <= top:
        raise ValueError(f"depth_filter_min_support = {ints['depth_filter_min_support']}: must lie in [0, {top}] for radius {r}")
    if ints["depth_filter_min_region"] < 0:
        raise ValueError(f"depth_filter_min_region = {ints['depth_filter_min_region']}: must not be negative")


def depth_filter_parameters(cfg) -> dict:
    """config.depth_filter_* as FusionContext.filter_depth_slots takes them"""
    return dict(jump_rel=float(cfg.depth_filter_jump), radius=int(cfg.depth_filter_radius),
                min_support=int(cfg.depth_filter_min_support), min_region=int(cfg.depth_filter_min_region))


def check_photometric_options(cfg, images=None, estimate_scale=False, sharded=False):
    """config.photometric: what reconstruct() / reconstruct_sharded() refuse before any device work.
    images: the loaded colour images (an entry None = a frame without colour)."""
    if not bool(getattr(cfg, "photometric", False)):
        return
    if sharded:
        raise ValueError("photometric needs a single GPU: the shards register on the ICP lanes, and the joint registration is not wired into them")
    if estimate_scale:
        raise ValueError("photometric does not go with estimate_scale: the joint registration estimates no scale")
    if bool(getattr(cfg, "loop_closure", False)):
        raise ValueError("photometric does not go with loop_closure: the pose graph's edge weights are geometric (a joint-weight graph is a later change)")
    w, g, j = float(cfg.photo_weight), float(cfg.photo_gate), float(cfg.photo_depth_jump)
    if not (np.isfinite(w) and w >= 0.0):
        raise ValueError(f"photo_weight = {w}: must be finite and not negative")
    if not (np.isfinite(g) and g > 0.0):
        raise ValueError(f"photo_gate = {g}: must be finite and positive")
    if not (np.isfinite(j) and j > 0.0):
        raise ValueError(f"photo_depth_jump = {j}: must be finite and positive")
    r = cfg.photo_smooth_radius
    if isinstance(r, bool) or int(r) != r or not 0 <= int(r) <= 7:
        raise ValueError(f"photo_smooth_radius = {r}: must be a whole number in [0, 7]")
    if images is not None and any(im is None for im in images):
        raise ValueError("photometric needs a colour image with every frame")


class DepthToReconstructionPipeline:
    def __init__(self, config: ReconstructionConfig = None):
        self.config = config or ReconstructionConfig()
        self.dense = DenseReconstructor(self.config)
        self.images: List[np.ndarray] = []
        self.image_names: List[str] = []
        self.depths: List[np.ndarray] = []
        self.camera_poses: List[Tuple[np.ndarray, np.ndarray]] = []
        self.frame_index: List[int] = []          # which loaded frame each pose belongs to
        self.chain_poses: List[Tuple[np.ndarray, np.ndarray]] = []   # the poses as registration chained them (config.loop_closure / model_tracking: before the optimisation / the tracking)
        self.icp_log: List[dict] = []
        self.stats: dict = {}
        self.timings: dict = {}                   # wall seconds per stage of the last reconstruct()
        self.grid: Optional[GridSpec] = None      # the fusion volume of the last reconstruct(): the whole lattice (nvox may exceed 2^32)
        self.blocks: List[GridSpec] = []          # the grids it was fused in (one, or the blocks of a lattice beyond one grid)
        self.mesh_normals = None                  # f32 [V,3] of that mesh when config.mesh_normals, else None
        self.mesh = None                          # (xyz f32 [V,3], rgb u8 [V,3], tris u32 [T,3]) of the last reconstruct(), config.extract_mesh
        self.cloud_normals = None                 # f32 [N,3] of the returned points when config.cloud_normals, else None
        self.cloud_curvature = None               # f32 [N] of the returned points when config.cloud_curvature, else None
        self.cloud_plane_ids = None               # i32 [N] of the returned points when config.cloud_planes: a plane's number or -1
        self.cloud_planes = None                  # the planes' records (normal, d, centroid, rms, count, seed) when config.cloud_planes
        self._plane_curvature = None              # the curvature on its way from the normals to the planes, between the two calls only

    # ---- a2 --------------------------------------------------------------------------------------
    def load_data(self, rgb_folder: str, depth_folder: str) -> int:
        self.images, self.depths, self.image_names = fileio.load_data(rgb_folder, depth_folder)
        self._files = None
        return len(self.images)

    def load_data_streaming(self, rgb_folder: str, depth_folder: str) -> int:
        """Same pairing rules and messages as load_data(), but only the file names are kept: reconstruct() then decodes
        on worker threads into pinned buffers and uploads asynchronously (fileio.FramePrefetcher), so host RAM never
        holds the whole sequence (the reference keeps every frame in two lists, D2R:434-437)."""
        from pathlib import Path
        rgb_path, depth_path = Path(rgb_folder), Path(depth_folder)
        files = sorted(f for f in rgb_path.iterdir() if f.suffix.lower() in fileio.IMAGE_SUFFIXES)
        print(f"Found {len(files)} RGB images")
        pairs = []
        for f in files:
            d = fileio.DepthImageLoader.find_matching_depth(f.name, depth_path)
            if d is None:
                print(f"  Warning: No depth found for {f.name}")
                continue
            pairs.append((f, d))
        print(f"Loaded {len(pairs)} image-depth pairs")
        self._files = pairs
        self.image_names = [f.name for f, _ in pairs]
        if pairs:
            first = fileio.read_image_bgr(pairs[0][0])
            self._frame_shape = first.shape[:2]
        self.images, self.depths = [None] * len(pairs), [None] * len(pairs)
        return len(pairs)

    def set_frames(self, images, depths, names=None):
        """Same state load_data() leaves, from arrays already in memory."""
        self.images, self.depths = list(images), list(depths)
        self.image_names = list(names) if names is not None else [f"frame_{i:04d}" for i in range(len(self.images))]
        return len(self.images)

    # ---- poses: ICP replaces detect_and_match / compute_pose ---------------------------------------
    def _register(self, ctx: FusionContext, scales, init_poses=None):
        """Frame-to-frame registration.  Consecutive pairs are independent: they go to the device in batches, every pair of
        a batch through all its levels and iterations inside one launch.  A failed pair drops its frame (reference rule,
        D2R:598-615): the following pair is then re-registered against the last kept frame."""
        n = len(self.depths)
        if not isinstance(scales, (list, tuple)):
            scales = [float(scales)] * n
        level_list = self._icp_levels()
        cfg = self.config
        photo = bool(getattr(cfg, "photometric", False))
        log_start = len(self.icp_log)
        log_keys = ("fitness", "rmse", "n_corr", "iters_run", "status") + (("n_photo", "photo_rmse") if photo else ())
        if photo:
            level_list = [dict(lv, photo_weight=float(cfg.photo_weight), photo_gate=float(cfg.photo_gate)) for lv in level_list]

        def register(pairs, T0s, pair_scales):
            """the one way to the device: the joint registration with config.photometric, else the batched ICP"""
            if photo:
                return ctx.rgbd_register(pairs, level_list, T_init=T0s, scales=pair_scales)
            return ctx.icp_batch(pairs, level_list, T_init=T0s, scales=pair_scales)

        def blocking(src, cur, T0):
            return register([(src, cur)], [T0], [scales[src]])[0]
        poses = [(np.eye(3), np.zeros((3, 1)))]
        index = [0]
        prev = 0
        ctx.build_normals_many(list(range(n)), scales)
        if photo:
            ctx.build_intensity(list(range(n)), int(cfg.photo_smooth_radius), float(cfg.photo_depth_jump))
        T_guess = np.eye(4)

        def prior(a, b_):
            return T_guess if init_poses is None else relative_prior(init_poses, a, b_)

        i = 1
        while i < n:
            # every pair of a batch runs all its levels inside ONE launch (tl3d_icp_batch_*); batches only exist so that the
            # constant-velocity prior of the next one can come from the last pose found (a short first batch gets one early)
            batch = list(range(i, min(n, i + (16 if i == 1 else 128))))
            srcs = [prev if cur == batch[0] else cur - 1 for cur in batch]
            T0s = [prior(src, cur) for src, cur in zip(srcs, batch)]
            results = register(list(zip(srcs, batch)), T0s, [scales[src] for src in srcs])
            for lane, cur in enumerate(batch):
                print(f"\nProcessing image {cur}...")
                res = results[lane]
                src = prev if cur == batch[0] else cur - 1
                if src != prev:                       # the frame this run started from was dropped: redo against `prev`
                    res = blocking(prev, cur, prior(prev, cur))
                self.icp_log.append(dict(frame=cur, against=prev, **{k: res[k] for k in log_keys}))
                if res["status"] == 2 or res["n_corr"] < 8:
                    print(f"  Skipping - registration failed (correspondences: {res['n_corr']})")
                    continue
                T = res["T"]
                r_c, t_c = compose(T[:3, :3], T[:3, 3], *poses[-1])
                poses.append((r_c, t_c))
                index.append(cur)
                print(f"  ICP: fitness {res['fitness']:.3f}, rmse {res['rmse'] * 1e3:.2f} mm, {res['iters_run']} iterations")
                T_guess = T                  # constant-velocity prior for the next batch
                prev = cur
            i = batch[-1] + 1
        if photo:
            kept = [e for e in self.icp_log[log_start:] if e["frame"] in index[1:]]
            self._photo_stats = dict(weight=float(cfg.photo_weight), gate=float(cfg.photo_gate), smooth_radius=int(cfg.photo_smooth_radius),
                                     depth_jump=float(cfg.photo_depth_jump), frames=len(kept), n_photo=int(sum(e["n_photo"] for e in kept)),
                                     mean_photo_rmse=float(np.mean([e["photo_rmse"] for e in kept])) if kept else 0.0)
        return poses, index

    def _close_loops(self, ctx: FusionContext):
        """config.loop_closure: detect revisits from the chain's poses, register them with the chain's own
        ICP, and optimise every pose over the graph of odometry and loop edges (posegraph).  An edge (i, j) is the registration of
        src = kept frame i against tgt = kept frame j; its weight is the 6 x 6 A of the point-to-plane pass at its pose
        (FusionContext.icp_evaluate, final level's stride and gate).  Returns (poses, stats); the poses ARE self.camera_poses when
        nothing was optimised."""
        from . import posegraph as pg
        cfg = self.config
        poses, index = self.camera_poses, self.frame_index
        n = len(poses)
        stats = dict(candidates=0, scored=0, registered=0, accepted=0, pruned=0, iterations=0, cost_before=0.0, cost_after=0.0,
                     max_correction_mm=0.0, max_correction_deg=0.0)
        cands = pg.loop_candidates(poses, cfg.loop_min_gap, cfg.loop_max_dist, cfg.loop_max_angle_deg)
        stats["candidates"] = len(cands)
        if not cands:
            print("Loop closure: no revisit among the chain's poses, nothing to optimise")
            return poses, stats
        print("\n--- Step 1b: Close loops (pose graph over ICP edges) ---")
        if n > pg.MAX_NODES:
            raise ValueError(f"loop_closure: {n} kept frames exceed the {pg.MAX_NODES} nodes the dense pose-graph solve holds")
        T = pg.poses_to_matrices(poses)
        levels = self._icp_levels()
        stride, gate, coarse_gate = levels[-1]["stride"], levels[-1]["max_dist"], levels[0]["max_dist"]
        slot = lambda k: index[k]                            # kept frame k lives in slot index[k]
        scale = lambda k: self.scales[index[k]]
        # 1. the odometry edges: every chain pair at its result
        chain_pairs = [(k, k + 1) for k in range(n - 1)]
        chain_Z = [pg.relative_pose(T[i], T[j]) for i, j in chain_pairs]
        ev = ctx.icp_evaluate([(slot(i), slot(j)) for i, j in chain_pairs], chain_Z, stride, gate, scales=[scale(i) for i, _ in chain_pairs])
        edges = [(i, j, Z, e["A"]) for (i, j), Z, e in zip(chain_pairs, chain_Z, ev)]
        # 2.-4. score every candidate at the chain-relative pose (coarse gate), keep the best few per frame
        rel = [pg.relative_pose(T[i], T[j]) for i, j in cands]
        sc = ctx.icp_evaluate([(slot(i), slot(j)) for i, j in cands], rel, stride, coarse_gate, scales=[scale(i) for i, _ in cands])
        stats["scored"] = len(sc)
        keep = pg.select_candidates(cands, [e["n_corr"] for e in sc], [e["fitness"] for e in sc], cfg.loop_edges_per_frame, cfg.loop_min_fitness)
        stats["registered"] = len(keep)
        loops = []
        if keep:
            # 5. register them from the chain-relative pose, through the chain's levels
            kp = [cands[k] for k in keep]
            res = []
            for i0 in range(0, len(kp), 256):
                part = kp[i0:i0 + 256]
                res += ctx.icp_batch([(slot(i), slot(j)) for i, j in part], levels, T_init=[rel[k] for k in keep[i0:i0 + 256]],
                                     scales=[scale(i) for i, _ in part])
            # 6. their weights at the result; accept by status and fitness there
            ev = ctx.icp_evaluate([(slot(i), slot(j)) for i, j in kp], [r["T"] for r in res], stride, gate, scales=[scale(i) for i, _ in kp])
            for (i, j), r, e in zip(kp, res, ev):
                if r["status"] != 2 and e["fitness"] >= cfg.loop_min_fitness:
                    loops.append((i, j, np.array(r["T"]), e["A"]))
        stats["accepted"] = len(loops)
        if not loops:
            print(f"  Loop closure: {len(cands)} candidates, none accepted, nothing to optimise")
            return poses, stats
        # 7., 8. optimise, drop the closures that keep a large residual, optimise again
        import torch
        device = torch.device("cuda", int(cfg.device)) if torch.cuda.is_available() else "cpu"
        out, info = pg.optimise_and_prune(poses, edges + loops, [False] * len(edges) + [True] * len(loops), cfg.loop_max_residual, device=device)
        mm, deg = pg.largest_correction(poses, out)
        stats.update(pruned=len(info["pruned"]), iterations=info["iterations"], cost_before=info["cost_before"], cost_after=info["cost_after"],
                     max_correction_mm=round(mm, 4), max_correction_deg=round(deg, 5))
        print(f"  Loop closure: {len(cands)} candidates, {len(keep)} registered, {len(loops)} accepted, {len(info['pruned'])} pruned; "
              f"{info['iterations']} iterations, cost {info['cost_before']:.4g} -> {info['cost_after']:.4g}, largest correction {mm:.2f} mm / {deg:.3f} deg")
        return out, stats

    def _track_model(self, ctx: FusionContext):
        """config.model_tracking: register every kept frame against the TSDF fused from the kept frames before
        it (FusionContext.track, point-to-SDF), in order.  Frame 0 is integrated at its pose; frame k starts from the chain's step
        applied to the tracked pose of frame k - 1, M0_k = (M_k M_k-1^-1)(chain) M_k-1(tracked), takes the registration's pose
        unless it failed (status 2) or its fitness is below track_min_fitness (then it keeps M0_k and counts as lost), and is
        integrated there.  The tracking grid is a TSDF-only grid of its own over the frames' bounds at the chain's poses, detached
        again; the fusion that follows starts afresh.  Returns (poses, stats)."""
        cfg = self.config
        index, chain = self.frame_index, self.camera_poses
        scales = [self.scales[fi] for fi in index]
        mn, mx = ctx.frames_bounds(index, chain, scales, subsample=cfg.subsample_factor)
        if not np.all(np.isfinite(mn)):
            raise ValueError("model_tracking: the frames at the chain's poses hold no valid point")
        mn, mx = np.asarray(mn, np.float64) - cfg.track_margin, np.asarray(mx, np.float64) + cfg.track_margin
        voxel = float(cfg.track_voxel_size or cfg.voxel_size)
        while True:                                          # one block that fits: the tracker reads a whole lattice
            lattice = plan_lattice(mn, mx, voxel, cfg.grid_dim, channels=abi.CH_TSDF, trunc_voxels=cfg.sdf_trunc_voxels)
            if lattice.nvox <= MAX_BLOCK_VOXELS:
                layout = choose_layout(ctx, lattice, index, chain, scales, cfg.subsample_factor, log=lambda *a: None)
                if layout.device_bytes() <= device_free_bytes(cfg.device) - BLOCK_MEMORY_MARGIN:
                    break
            voxel *= 2.0
        print(f"\n--- Step 1c: Track frames against the fused model (point-to-SDF, grid {layout.dims} @ {voxel * 1e3:g} mm) ---")
        if cfg.track_levels is None:
            levels = self._icp_levels()
        else:
            common = dict(damping=cfg.icp_damping, eig_rel=cfg.icp_eig_rel, eps=cfg.icp_eps)
            levels = [dict(iters=int(lv[0]), stride=int(lv[1]), max_dist=float(lv[2]), **common) for lv in cfg.track_levels]
        mat = lambda p: np.block([[np.asarray(p[0], np.float64).reshape(3, 3), np.asarray(p[1], np.float64).reshape(3, 1)], [np.zeros((1, 3)), np.ones((1, 1))]])
        M_chain = [mat(p) for p in chain]
        out, fit, rmse, lost, mm, deg = [M_chain[0]], [], [], 0, 0.0, 0.0
        ctx.attach_grid(layout)
        try:
            ctx.integrate(index[0], chain[0], scales[0])
            for k in range(1, len(index)):
                M0 = (M_chain[k] @ np.linalg.inv(M_chain[k - 1])) @ out[-1]
                res = ctx.track(index[k], (M0[:3, :3], M0[:3, 3]), levels, min_weight=cfg.track_min_weight, scale=scales[k])
                M = M0
                if res["status"] != 2 and res["fitness"] >= cfg.track_min_fitness:
                    M = np.array(res["T"])
                    fit.append(res["fitness"])
                    rmse.append(res["rmse"])
                    D = M @ np.linalg.inv(M0)
                    mm = max(mm, 1e3 * float(np.linalg.norm(M0[:3, :3].T @ M0[:3, 3] - M[:3, :3].T @ M[:3, 3])))
                    deg = max(deg, float(np.degrees(np.arccos(np.clip(0.5 * (np.trace(D[:3, :3]) - 1.0), -1.0, 1.0)))))
                else:
                    lost += 1
                out.append(M)
                ctx.integrate(index[k], (M[:3, :3], M[:3, 3]), scales[k])
        finally:
            ctx.detach_grid()
        stats = dict(frames=len(index), tracked=len(index) - 1 - lost, lost=lost, mean_fitness=round(float(np.mean(fit)), 4) if fit else 0.0,
                     mean_rmse_mm=round(1e3 * float(np.mean(rmse)), 4) if rmse else 0.0, max_correction_mm=round(mm, 4),
                     max_correction_deg=round(deg, 5), voxel_size=voxel)
        print(f"  Model tracking: {stats['tracked']} of {len(index) - 1} frames tracked, {lost} lost; mean fitness {stats['mean_fitness']:.3f}, "
              f"mean rmse {stats['mean_rmse_mm']:.2f} mm, largest correction {mm:.2f} mm / {deg:.3f} deg")
        shape = np.shape(chain[0][1])
        return [(M[:3, :3].copy(), M[:3, 3].reshape(shape).copy()) for M in out], stats

    def _icp_levels(self, sim3: bool = False):
        """The levels handed to ctx.icp_batch.  Coarse-to-fine: each level is (iterations, pixel stride, correspondence gate); every
        level starts from the previous level's pose.  A wide first gate takes frame steps of 0.5 m / 30 degrees that the 5 cm gate
        alone loses from 15 cm / 8 degrees on (tools/icp_basin.py); a level that has converged stops after one iteration.
        sim3: a wider level still in front, the scale as 7th unknown, the last abi.ICP_MAX_LEVELS of them."""
        cfg = self.config
        levels = [tuple(l) for l in cfg.icp_coarse] + [(cfg.icp_iters, cfg.icp_stride, cfg.icp_max_dist)]
        common = dict(damping=cfg.icp_damping, eig_rel=cfg.icp_eig_rel, eps=cfg.icp_eps)
        if sim3:
            levels = ([(15, max(2, int(cfg.icp_stride) * 2), 1.0)] + levels)[-abi.ICP_MAX_LEVELS:]
            common["estimate_scale"] = True
        return [dict(iters=int(lv[0]), stride=int(lv[1]), max_dist=float(lv[2]), **common) for lv in levels]

    def _sim3_chain(self, ctx: FusionContext, frames, slot_of, state, init_poses=None, weight: float = 0.3):
        """One stretch of the Sim(3) registration chain: the views `frames` (ascending global indices), one after the other,
        each against the last kept view.  `state` = dict(prev, prev_scale, avg, T_guess) is where the chain stands -- the last kept
        view (resident in slot_of, its normals built with prev_scale), the running scale and the constant-velocity prior -- and
        comes back advanced, so that the next stretch (the next rank, reconstruct_sharded) continues exactly where this one ends.
        Returns {cur: row}; row: T (prev -> cur, the (R_rel, t_rel) the reference chains), against, ok, scale_raw (the
        registration's own estimate), scale (the running value the view is fused with), statistics."""
        level_list = self._icp_levels(sim3=True)
        rows = {}
        prev, avg, T_guess = int(state["prev"]), float(state["avg"]), np.asarray(state["T_guess"], np.float64).reshape(4, 4)
        for cur in frames:
            print(f"\nProcessing image {cur}...")
            T0 = T_guess if init_poses is None else relative_prior(init_poses, cur, prev)
            res = ctx.icp_batch([(slot_of[cur], slot_of[prev])], level_list, T_init=[T0], scales=[avg])[0]
            ok = not (res["status"] == 2 or res["n_corr"] < 8 or not np.isfinite(res["scale"]) or not (1e-3 < res["scale"] < 1e3))
            row = dict(T=np.eye(4), against=prev, ok=ok, scale_raw=float(res["scale"]) if np.isfinite(res["scale"]) else 0.0, scale=avg,
                       **{k: res[k] for k in ("fitness", "rmse", "n_corr", "iters_run", "status")})
            rows[cur] = row
            if not ok:
                print(f"  Skipping - registration failed (correspondences: {res['n_corr']})")
                continue
            avg = (1.0 - weight) * avg + weight * res["scale"]               # D2R:650 with weight = 0.3
            T = res["T"]
            Ti = np.eye(4)
            Ti[:3, :3] = T[:3, :3].T
            Ti[:3, 3] = -T[:3, :3].T @ T[:3, 3]              # prev -> cur = (R_rel, t_rel)
            row["T"], row["scale"] = Ti, avg
            print(f"  ICP: fitness {res['fitness']:.3f}, rmse {res['rmse'] * 1e3:.2f} mm, {res['iters_run']} iterations, scale {res['scale']:.6f} -> {avg:.6f}")
            ctx.build_normals(slot_of[cur], scale=avg)
            T_guess = T
            prev = cur
            state.update(prev=prev, prev_scale=avg)
        state.update(avg=avg, T_guess=T_guess)
        return rows

    def _register_with_scale(self, ctx: FusionContext, scale0: float, init_poses=None, weight: float = 0.3):
        """Registration of RELATIVE depth maps (row f3): every view's metric scale is the 7th unknown of its registration
        against the previous kept view (Sim(3) point-to-plane ICP, tl3d_icp_params.estimate_scale), which replaces the
        reference's median of Z_triangulated / depth over SIFT points (D2R:297-326, DER:659-697).  View 0 fixes the gauge
        (scale0 = config.depth_scale, or the anchors' estimate); the running scale follows the reference's rule
        avg = (1 - w) avg + w scale_i (D2R:650, w = 0.3; config.scale_update_weight = 1 trusts every view's own estimate).
        The source of a run is the NEW view (unknown scale), the target the previous one (scale known, normals built with
        it), so the run returns cur -> prev; its inverse is the (R_rel, t_rel) the reference chains (D2R:618-620).
        Sequential by nature: a view's target needs that view's scale.  (Both views of a run read window-averaged depth when
        config.icp_smooth_radius > 0: the target through its normal map, the source through the averaged map its own normals were
        built from -- a view is a source BEFORE its scale is known, so its map is built with the running value first and rebuilt
        with its own scale once that is known; the averaged depth itself does not depend on the scale.)"""
        n = len(self.depths)
        ctx.build_normals_many(list(range(n)), [float(scale0)] * n)       # every view's averaged depth (what a SOURCE reads); normals are rebuilt per view below
        state = dict(prev=0, prev_scale=float(scale0), avg=float(scale0), T_guess=np.eye(4))
        rows = self._sim3_chain(ctx, list(range(1, n)), {g: g for g in range(n)}, state, init_poses, weight)
        return self._sim3_finish(rows, n, scale0)

    def _sim3_finish(self, rows, n, scale0):
        """(poses, kept frame indices, per-frame scales) from the rows of every view 1 .. n-1: cam0 = (I, 0), then
        R = R_rel R_prev, t = R_rel t_prev + t_rel over the kept views (D2R:618-620)."""
        poses, index, scales = [(np.eye(3), np.zeros((3, 1)))], [0], [float(scale0)] * n
        for cur in range(1, n):
            row = rows[cur]
            self.icp_log.append(dict(frame=cur, against=row["against"], scale=row["scale_raw"],
                                     **{k: row[k] for k in ("fitness", "rmse", "n_corr", "iters_run", "status")}))
            if not row["ok"]:
                continue
            scales[cur] = row["scale"]
            r_c, t_c = compose(row["T"][:3, :3], row["T"][:3, 3], *poses[-1])
            poses.append((r_c, t_c))
            index.append(cur)
        return poses, index, scales

    # ---- reconstruct ---------------------------------------------------------------------------------
    def reconstruct(self, grid: Optional[GridSpec] = None, init_poses=None, poses=None, anchors=None, estimate_scale: bool = False):
        """(points, colors, camera_poses) like D2R:479-671.

        grid: fix the fusion volume (else planned from the data with Open3D's voxel origin).
        init_poses: optional per-frame pose priors for ICP; poses: skip registration and fuse with these poses.
        anchors: {frame: (points3d, pixels)} sparse metric anchors -> per-frame depth scale by the reference's rule
        (ScaleTracker); default: config.depth_scale for every frame (metric depth).
        estimate_scale: relative depth with no anchors -- every view's scale is estimated by its registration (Sim(3) ICP,
        _register_with_scale); view 0 keeps config.depth_scale (or its anchors' estimate).
        """
        self.mesh = None
        self.mesh_normals = None
        self.cloud_normals = self.cloud_curvature = self.cloud_plane_ids = self.cloud_planes = self._plane_curvature = None
        cfg = self.config
        self._check_mesh_filter_config()
        self._check_mesh_weld_config()
        self._check_cloud_normals_config()
        check_compare_options(cfg)
        check_depth_filter_options(cfg)
        self._photo_stats = None
        if poses is None:                                                       # with poses given nothing is registered: the option is ignored
            check_photometric_options(cfg, None if getattr(self, "_files", None) is not None else self.images, estimate_scale)
        loop = bool(getattr(cfg, "loop_closure", False)) and poses is None      # with poses given nothing is registered: the option is ignored
        if loop and estimate_scale:
            raise ValueError("loop_closure does not go with estimate_scale: the pose graph's edges carry no scale")
        track = bool(getattr(cfg, "model_tracking", False)) and poses is None   # ... and so is this one
        if track and estimate_scale:
            raise ValueError("model_tracking does not go with estimate_scale: tracking against the model estimates no scale")
        if len(self.images) < 2:
            print("Need at least 2 images")
            return None, None, None
        print("\n" + "=" * 70)
        print("DEPTH-ENHANCED RECONSTRUCTION PIPELINE (MI355X: ICP + voxel fusion)")
        print("=" * 70)
        streaming = getattr(self, "_files", None) is not None
        h, w = self._frame_shape if streaming else self.depths[0].shape
        n = len(self.depths)
        scale = float(cfg.depth_scale)
        if not anchors:
            print(f"Using depth scale = {scale} (depth assumed metric, as D2R:555-558)")
        # one context: every frame is uploaded once and stays resident in HBM through registration, bounding and fusion
        # (288 GB holds ~19 000 frames of 1080x1920 depth+colour); the grid is attached once the scene bounds are known
        clock, marks = time.perf_counter, [("start", time.perf_counter())]
        ctx = FusionContext(w, h, cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.min_depth, cfg.max_depth, n_slots=n, grid=None,
                            device=cfg.device)
        ctx.set_normal_smoothing(int(getattr(cfg, "icp_smooth_radius", 0)))
        try:
            if streaming:
                pre = fileio.FramePrefetcher(ctx, [f for f, _ in self._files], [d for _, d in self._files])
                try:
                    for _i, _slot in pre:
                        pass
                finally:
                    # where a file-fed run's time goes: decode (summed over the worker threads) against the wall time of the stage
                    self.decode_stats = dict(workers=pre.workers, decode_thread_seconds=round(pre.decode_s, 3),
                                             decode_ms_per_frame_and_thread=round(1e3 * pre.decode_s / max(1, n), 2))
                    pre.close()
            else:
                for i in range(n):
                    if self.depths[i].shape != (h, w):
                        raise ValueError(f"frame {i} is {self.depths[i].shape}, expected {(h, w)}")
                    ctx.upload(i, self.depths[i], self.images[i])
            # depth maps may be GPU tensors (depth estimated in this process): the scale rule then reads them back per frame
            host_depths = [d if isinstance(d, np.ndarray) else None for d in self.depths]
            self.scales = per_frame_scales(host_depths, anchors, default=scale, fetch=ctx.download_depth)
            marks.append(("upload", clock()))
            depth_filter_stats = None
            if getattr(cfg, "depth_filter", False):
                depth_filter_stats = self._filter_depth_frames(ctx, n)
                marks.append(("depth_filter", clock()))
            if poses is not None:
                self.camera_poses, self.frame_index = list(poses), list(range(len(poses)))
            else:
                if estimate_scale:
                    print("\n--- Step 1: Register frames (Sim(3) point-to-plane ICP: pose and depth scale, frame to frame) ---")
                    self.camera_poses, self.frame_index, self.scales = self._register_with_scale(
                        ctx, self.scales[0], init_poses, weight=float(getattr(cfg, "scale_update_weight", 0.3)))
                else:
                    print("\n--- Step 1: Register frames (point-to-plane ICP, frame to frame) ---")
                    self.camera_poses, self.frame_index = self._register(ctx, self.scales, init_poses)
            marks.append(("register", clock()))
            if len(self.camera_poses) < 2:
                print("Pose estimation failed")
                return None, None, None
            self.chain_poses = list(self.camera_poses)
            loop_stats = None
            if loop:
                self.camera_poses, loop_stats = self._close_loops(ctx)
                marks.append(("loop_closure", clock()))
            track_stats = None
            if track:
                self.camera_poses, track_stats = self._track_model(ctx)
                marks.append(("track", clock()))
            given = grid is not None
            if given:
                blocks = [Block(grid, (0, 0, 0), tuple(grid.dims))]          # the caller's grid: one block, its layout taken as given
            else:
                print("\n--- Step 2: Bound the scene ---")
                # extent of the union of the frames' clouds, on the device
                mn, mx = ctx.frames_bounds(self.frame_index, self.camera_poses, [self.scales[fi] for fi in self.frame_index],
                                           subsample=cfg.subsample_factor)
                if not np.all(np.isfinite(mn)):
                    print("Reconstruction failed")
                    return None, None, None
                # the whole lattice, never shaved; more than one grid's worth of voxels is fused block by block
                grid = plan_lattice(mn, mx, cfg.voxel_size, cfg.grid_dim, trunc_voxels=cfg.sdf_trunc_voxels)
                blocks = plan_blocks(grid, MAX_BLOCK_VOXELS)
            xyz, rgb = self._fuse_blocks(ctx, grid, blocks, marks, layout_given=given)
            if depth_filter_stats is not None:
                self.stats["depth_filter"] = depth_filter_stats
            if loop_stats is not None:
                self.stats["loop_closure"] = loop_stats
            if track_stats is not None:
                self.stats["model_tracking"] = track_stats
            if self._photo_stats is not None:
                self.stats["photometric"] = self._photo_stats
        finally:
            ctx.close()
        return xyz.astype(np.float64), rgb, self.camera_poses

    def _filter_depth_frames(self, ctx: FusionContext, n: int) -> dict:
        """config.depth_filter: flying pixels and small regions of all n resident frames set to 0, in one call, in front of everything
        that reads a frame.  Returns what goes into stats["depth_filter"]: the totals of the four counts, the
        frames and the parameters."""
        prm = depth_filter_parameters(self.config)
        counts = ctx.filter_depth_slots(list(range(n)), **prm)
        tot = counts.sum(axis=0)
        out = dict(frames=int(n), valid=int(tot[0]), removed_flying=int(tot[1]), regions=int(tot[2]), removed_regions=int(tot[3]), **prm)
        print(f"  Depth filter: {out['removed_flying']} flying pixels and {out['removed_regions']} pixels of small regions "
              f"removed from {out['valid']} valid pixels of {n} frames")
        return out

    def _compare(self, ctx: FusionContext, xyz):
        """config.compare_to: the fused cloud against the reference scan's points (metrics.compare_clouds; a = the fused cloud, so
        precision is its accuracy and recall its completeness), and under "mesh" the reference against the final mesh
        (metrics.compare_cloud_to_mesh) when there is one.  Reads the results only: nothing the run computes changes."""
        from . import metrics
        cfg = self.config
        ref = fileio.read_ply_points(cfg.compare_to)
        thr = tuple(float(t) for t in (cfg.compare_thresholds or ()))
        cloud = np.ascontiguousarray(xyz, dtype=np.float32)
        mesh_xyz = self.mesh[0] if self.mesh is not None else None
        alignment = None
        if getattr(cfg, "compare_align", False):
            # the scan's normals stay unoriented (the sign of a normal does not reach a point-to-plane row); the cloud and the mesh's
            # vertices are moved on the host, in copies: what the run computed and writes stays in its own frame
            init = check_compare_options(cfg)
            normals = ctx.estimate_normals(ref)
            kw = {}
            if getattr(cfg, "compare_align_global", False):
                # the start from anywhere; when no sample passes T is the identity: the plain local start
                init = "global"
                kw["global_kw"] = dict(voxel=float(cfg.compare_align_global_voxel or 5.0 * cfg.voxel_size))
            res, cloud = metrics.align_clouds(ctx, cloud, ref, normals, T_init=init, estimate_scale=bool(cfg.compare_align_scale), **kw)
            alignment = dict(T=res["T"].tolist(), scale=res["scale"], fitness=res["fitness"], rmse=res["rmse"], n_corr=res["n_corr"],
                             iters_run=res["iters_run"], status=res["status"])
            if "global" in res:
                g = res["global"]
                alignment["global"] = dict(T=g["T"].tolist(), inliers=g["inliers"], n_corr=g["n_corr"], n_passed=g["n_passed"],
                                           hypotheses=g["hypotheses"], voxel=g["voxel"], mutual=g["mutual"])
            if mesh_xyz is not None:
                mesh_xyz = metrics.move_points(mesh_xyz, res["T"], res["scale"])
        out = metrics.compare_clouds(ctx, cloud, ref, thresholds=thr, max_dist=cfg.compare_max_dist)
        out["reference"], out["reference_points"] = str(cfg.compare_to), len(ref)
        if self.mesh is not None:
            out["mesh"] = metrics.compare_cloud_to_mesh(ctx, ref, mesh_xyz, self.mesh[2], thresholds=thr, max_dist=cfg.compare_max_dist)
        if alignment is not None:
            out["alignment"] = alignment
            print("  " + metrics.format_alignment(alignment))
        print("  " + metrics.format_line(out))
        return out

    def _extract_points(self, ctx: FusionContext):
        cfg = self.config
        return ctx.extract(abi.EXTRACT_CENTROID, min_count=1, min_weight=cfg.tsdf_min_weight, max_abs_tsdf=cfg.tsdf_max_abs)

    def _clean_cloud(self, ctx: FusionContext, clouds, voxel_size):
        """The extracted clouds [(xyz, rgb)] as one, through the statistical outlier filter (D2R:413-415, once over the whole cloud;
        DER's merge has none, DER:615-645).  Returns xyz, rgb and the two counts of `stats`."""
        cfg = self.config
        xyz, rgb = clouds[0] if len(clouds) == 1 else [np.concatenate(c) for c in zip(*clouds)]
        n_vox = len(xyz)
        if n_vox > 0 and cfg.outlier_filter:
            keep = ctx.statistical_outlier(xyz, cfg.outlier_nb_neighbors, cfg.outlier_std_ratio, cell_size=2.0 * voxel_size)
            xyz, rgb = xyz[keep], rgb[keep]
        return xyz, rgb, dict(voxels=n_vox, after_outlier_filter=len(xyz))

    def _estimate_cloud_normals(self, ctx: FusionContext, xyz, voxel_size) -> float:
        """config.cloud_normals: normals (and curvature) of the cleaned cloud, every normal turned towards the nearest kept camera's
        centre -R^T t; once over the whole cloud, so a blocked run shows no seam.  Leaves cloud_normals /
        cloud_curvature (rows match xyz) and stats["cloud_normals"]; returns the seconds it took."""
        cfg = self.config
        t0 = time.perf_counter()
        k, radius = int(cfg.cloud_normals_neighbors), float(cfg.cloud_normals_radius)
        centres = np.array([-np.asarray(R, np.float64).T @ np.asarray(t, np.float64).reshape(3) for R, t in self.camera_poses],
                           np.float64).reshape(-1, 3)
        planes = bool(getattr(cfg, "cloud_planes", False))         # the segmentation wants the curvature, asked for or not
        out = ctx.estimate_normals(xyz, k, max_radius=radius, viewpoints=centres, cell_size=2.0 * voxel_size,
                                   curvature=bool(cfg.cloud_curvature) or planes)
        self.cloud_normals, curvature = out if (cfg.cloud_curvature or planes) else (out, None)
        self.cloud_curvature = curvature if cfg.cloud_curvature else None
        self.stats["cloud_normals"] = dict(neighbors=k, radius=radius, viewpoints=len(centres), degenerate=ctx.last_normals_degenerate)
        print(f"  Cloud normals: {len(xyz)} points, {k} neighbours, {len(centres)} viewpoints, {ctx.last_normals_degenerate} degenerate")
        self._plane_curvature = curvature if planes else None
        return time.perf_counter() - t0

    def _segment_cloud_planes(self, ctx: FusionContext, xyz, voxel_size) -> float:
        """config.cloud_planes: the planar regions of the cleaned cloud from its normals and curvature; once
        over the whole cloud, right behind _estimate_cloud_normals.  Leaves cloud_plane_ids (rows match xyz), cloud_planes and
        stats["cloud_planes"]; returns the seconds it took."""
        t0 = time.perf_counter()
        prm = cloud_plane_parameters(self.config, voxel_size)
        ids, planes, counts = ctx.segment_planes(xyz, self.cloud_normals, self._plane_curvature, **prm)
        self._plane_curvature = None
        self.cloud_plane_ids, self.cloud_planes = ids, planes
        largest = np.argsort(-planes["count"], kind="stable")[:10]
        self.stats["cloud_planes"] = dict(**counts, **prm, largest=[dict(count=int(planes["count"][k]), rms=float(planes["rms"][k])) for k in largest])
        print(f"  Cloud planes: {counts['planes']} planes hold {int((ids >= 0).sum())} of {len(xyz)} points "
              f"({counts['eligible']} eligible, {counts['regions']} regions, {counts['candidates']} of {prm['min_points']} points or more)")
        return time.perf_counter() - t0

    def _fuse_blocks(self, ctx: FusionContext, lattice: GridSpec, blocks: List[Block], marks=None, layout_given: bool = False):
        """The fusion of reconstruct(), for a lattice planned as one block as for many.  Per block, in the one context whose frames
        stay resident: the block's layout (from its own brick count), attach its grid, set its core, fuse every kept frame (the cull
        drops the frames that miss the block), extract the core's points (and its keyed mesh), detach.  Then once: the statistical
        outlier filter over the whole cloud, the blocks' meshes welded by their keys, `stats`, `timings`.  The blocks'
        cores tile the lattice and their halos carry the neighbours' voxels bit for bit: the points and the mesh are the single
        lattice's.  A plan of ONE block is the lattice grid itself: no core and no keys (its mesh is returned as extracted, nothing
        to weld), and it stays attached, because the ray caster (config.render_dir) reads an attached grid without a core.
        Returns (xyz f32, rgb)."""
        cfg, clock = self.config, time.perf_counter
        marks = marks or [("start", clock())]
        one = len(blocks) == 1
        if cfg.render_dir and not one:
            raise ValueError(f"render_dir: the scene's lattice {lattice.dims} ({lattice.nvox} voxels) is fused in {len(blocks)} "
                             "blocks, and ray casting across blocks does not exist (raise --voxel-size)")
        scales = [self.scales[fi] for fi in self.frame_index]
        # wall time per stage, summed over the blocks (host clock; a stage ends where the host has its result); the bounding and
        # planning since the last mark count as allocation
        stage = defaultdict(float, bound_and_allocate=clock() - marks[-1][1])
        if not one:
            print(f"  Lattice {lattice.dims} @ {lattice.voxel_size * 1e3:g} mm, origin {np.round(lattice.origin, 4)}: {lattice.nvox} voxels "
                  f"in {len(blocks)} blocks")
            print("\n--- Step 3: Fuse depth frames block by block (TSDF + voxel centroids) ---")
        todo, done, clouds, mesh_parts = list(reversed(blocks)), [], [], []
        core_points = valid_points = 0
        sums = dict(bricks_tsdf=0, bricks_centroid=0, pool_refused=0)
        while todo:
            b = todo.pop()
            t0 = clock()
            # dense or sparse: from the bricks these frames will really touch, not from the extent
            layout = b.grid if layout_given else choose_layout(ctx, b.grid, self.frame_index, self.camera_poses, scales, cfg.subsample_factor)
            if one:         # (a single grid that does not fit fails in attach_grid: splitting it instead would change behaviour)
                print(f"  Grid {layout.dims} @ {layout.voxel_size * 1e3:g} mm, origin {np.round(layout.origin, 4)}")
                print("\n--- Step 3: Fuse depth frames (TSDF + voxel centroids) ---")
            else:
                need = layout.device_bytes()
                if cfg.extract_mesh and layout.channels & abi.CH_TSDF:
                    need += (layout.pool_tsdf or layout.nvox // 512) * 2048          # the mesh's vertex-id scratch: 4 B per TSDF record
                if need > device_free_bytes(cfg.device) - BLOCK_MEMORY_MARGIN:
                    print(f"  Block at {b.grid.voxel_offset}: {need / 2**30:.2f} GiB does not fit, split in two")
                    todo.extend(reversed(split_block(lattice, b)))
                    continue
            ctx.attach_grid(layout)
            if not one:
                ctx.set_block_core(lattice.dims, b.lo, b.hi)
            ctx.reset_stats()
            t1 = clock()
            # TSDF + centroids of every kept frame, in order
            ctx.fuse_frames(self.frame_index, self.camera_poses, scales, centroid_subsample=cfg.subsample_factor)
            st = ctx.stats()
            t2 = clock()
            clouds.append(self._extract_points(ctx))
            t3 = clock()
            if cfg.extract_mesh:
                off = np.asarray(b.grid.voxel_offset, np.int64)
                mesh = ctx.extract_mesh(min_weight=cfg.tsdf_min_weight, keys=not one)
                mesh_parts.append(tuple(mesh) + (off + np.asarray(b.lo), off + np.asarray(b.hi)))
                stage["mesh"] += clock() - t3
            t4 = clock()
            if not one:
                ctx.detach_grid()
            core_points += int(st["centroid_points"])
            if not done:                                 # every block sees every kept frame's samples: in its core or elsewhere
                valid_points = int(st["centroid_points"]) + int(st["centroid_dropped"])
            sums["bricks_tsdf"] += int(st["pool_slots_tsdf"])
            sums["bricks_centroid"] += int(st["pool_slots_centroid"])
            sums["pool_refused"] += int(st["pool_refused"])
            done.append(layout)
            stage["bound_and_allocate"] += (t1 - t0) + (clock() - t4)
            stage["fuse"] += t2 - t1
            stage["extract_and_filter"] += t3 - t2
            if not one:
                print(f"  Block {len(done)} at {layout.voxel_offset}, grid {layout.dims} ({'sparse' if layout.sparse else 'dense'}, "
                      f"{layout.device_bytes() / 2**30:.2f} GiB): {len(clouds[-1][0])} voxels")
        self.blocks, self.grid = done, (done[0] if one else lattice)
        for fi in self.frame_index:
            print(f"Camera {fi}: fused")
        print("\n--- Step 4: Extract and clean point cloud ---")
        t0 = clock()
        xyz, rgb, counts = self._clean_cloud(ctx, clouds, lattice.voxel_size)
        stage["extract_and_filter"] += clock() - t0
        self.stats = dict(points_accumulated=core_points, points_dropped=valid_points - core_points, **counts,
                          sparse=any(g.sparse for g in done), **sums, blocks=len(done))
        if cfg.cloud_normals:
            stage["cloud_normals"] = self._estimate_cloud_normals(ctx, xyz, lattice.voxel_size)
        if getattr(cfg, "cloud_planes", False):
            stage["cloud_planes"] = self._segment_cloud_planes(ctx, xyz, lattice.voxel_size)
        if one and done[0].sparse:
            print(f"  Sparse volume: {sums['bricks_tsdf']} TSDF bricks and {sums['bricks_centroid']} centroid bricks hold records "
                  f"(of {done[0].nvox // 512}); {done[0].device_bytes() / 2**30:.2f} GiB")
        if sums["pool_refused"]:
            print(f"  Warning: {sums['pool_refused']} bricks found the record pool full and are missing from the result"
                  + (" (raise --grid, the memory budget of the volume)" if one else ""))
        if cfg.extract_mesh:
            t0 = clock()
            if one or not self._mesh_weld_on_device():
                vx, vr, vt = mesh_parts[0][:3] if one else weld_meshes(mesh_parts, lattice.dims)[:3]
            else:                                        # (the last block is detached: its grid's memory is free for the table)
                vx, vr, vt = ctx.weld_meshes(mesh_parts, lattice.dims)[:3]
                self.stats["mesh_weld"] = dict(parts=len(mesh_parts), vertices_in=sum(len(m[0]) for m in mesh_parts), vertices=len(vx),
                                               triangles=len(vt))
                stage["mesh_weld"] = clock() - t0
            print(f"  Mesh: {len(vx)} vertices, {len(vt)} triangles" + ("" if one else f" (welded from {len(done)} blocks)"))
            stage["mesh"] += clock() - t0
            if self._mesh_filter_on():                   # on the WELDED mesh: a surface that crosses a block seam is counted whole
                t0 = clock()
                vx, vr, vt = self._filter_mesh(ctx, (vx, vr, vt))
                stage["mesh_filter"] = clock() - t0
            if self._mesh_simplify_on():                 # after the filter: specks are judged at full resolution
                t0 = clock()
                vx, vr, vt = self._simplify_mesh(ctx, (vx, vr, vt))
                stage["mesh_simplify"] = clock() - t0
            if self._mesh_smooth_on():                   # after both: it moves what they left, and changes no index
                t0 = clock()
                vx = self._smooth_mesh(ctx, (vx, vr, vt))[0]
                stage["mesh_smooth"] = clock() - t0
            if cfg.mesh_normals:                         # last: from the final positions
                t0 = clock()
                self.mesh_normals = ctx.mesh_normals(vx, vt)
                stage["mesh_normals"] = clock() - t0
            self.mesh = (vx, vr, vt)
            self.stats["mesh_vertices"] = len(vx)
            self.stats["mesh_triangles"] = len(vt)
        if cfg.render_dir:
            t0 = clock()
            self._render_views(ctx)
            stage["render"] = clock() - t0
        if cfg.compare_to:
            t0 = clock()
            self.stats["compare"] = self._compare(ctx, xyz)
            stage["compare"] = clock() - t0
        self.timings = {name + "_s": round(t1 - t0, 4) for (name, t1), (_, t0) in zip(marks[1:], marks[:-1])}
        self.timings.update({k + "_s": round(v, 4) for k, v in stage.items()})
        if not one:
            self.timings["blocks_s"] = round(clock() - marks[-1][1], 4)          # the whole blocked fusion
        print(f"\nFinal reconstruction: {len(xyz)} points, {len(self.camera_poses)} cameras")
        return xyz, rgb

    # ---- multi-GPU: frames shard across ranks, one exchange step at merge time -------------
    def _register_pairs(self, ctx: FusionContext, pairs, slot_of, scales, init_poses=None, T_guess=None):
        """Independent registrations (src, cur) -> result dict, every pair through the coarse-to-fine levels inside one
        launch per batch.  slot_of maps a global frame index to its resident slot."""
        out = {}

        def prior(a, b_):
            if init_poses is None:
                return np.eye(4) if T_guess is None else T_guess
            return relative_prior(init_poses, a, b_)

        level_list = self._icp_levels()
        for i0 in range(0, len(pairs), 256):
            batch = pairs[i0:i0 + 256]
            results = ctx.icp_batch([(slot_of[a], slot_of[b_]) for a, b_ in batch], level_list, T_init=[prior(a, b_) for a, b_ in batch],
                                    scales=[scales[a] for a, _ in batch])
            for (a, b_), res in zip(batch, results):
                out[b_] = dict(res, against=a)
        return out

    def reconstruct_sharded(self, dist, grid: Optional[GridSpec] = None, init_poses=None, poses=None, anchors=None, estimate_scale: bool = False):
        """reconstruct() over the ranks of an initialised torch.distributed group, one process per GPU:

          1. rank r uploads its contiguous frame range [lo, hi) plus the one-frame halo lo - 1 and registers every pair whose
             later frame it owns (the pair that crosses a shard boundary belongs to the later rank), on its ICP lanes;
          2. the relative transforms are exchanged (a few hundred bytes) and every rank chains the same global poses with
             the same fp64 products as D2R:618-620; a frame whose registration failed is dropped and its successor is
             re-registered against the last kept frame by the successor's owner (the reference's skip rule, D2R:598-615);
          3. scene bounds: per-rank min / max, MIN / MAX all-reduce -> every rank plans the same grid;
          4. rank r fuses its own frames into its private grid;
          5. ONE sum all-reduce of the integer grids (RCCL over xGMI with the nccl backend) -> every rank holds the merged
             grid, bit-identical to a single-GPU run GIVEN THE SAME POSES (pairs are registered independently here, from
             identity or init_poses; reconstruct() seeds later batches with a constant-velocity prior, so the two can converge
             to poses that differ in the last bits); rank 0 extracts, filters and returns the cloud (other ranks return
             (None, None, poses)).
        estimate_scale (relative depth, no anchors: reconstruct()'s Sim(3) registration): a view's target needs that view's scale,
        so the chain is sequential -- the ranks take turns, each continues it over its own views from the state the previous rank
        hands over (last kept view and its scale, running scale, motion prior: 19 doubles), and the poses, the scales and the
        cloud are those of the single-process run bit for bit; fusion and merge stay parallel.
        Every frame must be loaded on every rank's host (load_data); only the rank's own range goes to its GPU."""
        from . import distributed as dd
        if getattr(self.config, "loop_closure", False) and poses is None:
            raise ValueError("loop_closure needs a single GPU: every kept frame must be resident where the revisits are registered")
        if getattr(self.config, "model_tracking", False) and poses is None:
            raise ValueError("model_tracking needs a single GPU: every kept frame is registered against one model, in order")
        if getattr(self.config, "depth_filter", False):
            raise ValueError("depth_filter needs a single GPU: the shards upload their frames in several places, and the filter is not wired into them")
        if poses is None:
            check_photometric_options(self.config, sharded=True)
        self._check_mesh_filter_config()
        self._check_cloud_normals_config()
        check_compare_options(self.config)
        world, rank = dist.get_world_size(), dist.get_rank()
        self.mesh = None
        self.mesh_normals = None
        self.cloud_normals = self.cloud_curvature = self.cloud_plane_ids = self.cloud_planes = self._plane_curvature = None
        if len(self.images) < 2:
            print("Need at least 2 images")
            return None, None, None
        if getattr(self, "_files", None) is not None:
            raise ValueError("reconstruct_sharded needs load_data(): frames decoded on the host of every rank")
        cfg = self.config
        n = len(self.depths)
        h, w = self.depths[0].shape
        lo, hi = dd.shard_range(n, world, rank)
        first = max(0, lo - 1) if hi > lo else lo                  # halo frame in front of the range
        resident = list(range(first, hi))
        slot_of = {g: k for k, g in enumerate(resident)}
        say = print if rank == 0 else (lambda *a, **k: None)
        say("\n" + "=" * 70)
        say(f"DEPTH-ENHANCED RECONSTRUCTION PIPELINE (MI355X x{world}: ICP + voxel fusion, frames sharded by rank)")
        say("=" * 70)
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO() if rank else None) if rank else contextlib.nullcontext():
            self.scales = per_frame_scales(self.depths, anchors, default=float(cfg.depth_scale))
        spare = len(resident)                                       # one more slot for out-of-range sources of repairs
        ctx = FusionContext(w, h, cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.min_depth, cfg.max_depth, n_slots=len(resident) + 1, grid=None,
                            device=cfg.device)
        ctx.set_normal_smoothing(int(getattr(cfg, "icp_smooth_radius", 0)))
        try:
            for g in resident:
                ctx.upload(slot_of[g], self.depths[g], self.images[g])
            if poses is not None:
                self.camera_poses, self.frame_index = list(poses), list(range(len(poses)))
            elif estimate_scale:
                say("\n--- Step 1: Register frames (Sim(3) point-to-plane ICP: pose and depth scale; the ranks take turns along the chain) ---")
                scale0 = float(self.scales[0])
                weight = float(getattr(cfg, "scale_update_weight", 0.3))
                for g in resident:
                    ctx.build_normals(slot_of[g], scale=scale0)           # every view's averaged depth (what a SOURCE reads)
                state = dict(prev=0, prev_scale=scale0, avg=scale0, T_guess=np.eye(4))
                rows = {}
                for turn in range(world):
                    mine_now = list(range(max(lo, 1), hi)) if turn == rank else []
                    if mine_now:
                        slots = dict(slot_of)
                        if state["prev"] not in slots:                    # the last kept view lives on another rank's GPU: bring it here
                            ctx.upload(spare, self.depths[state["prev"]], self.images[state["prev"]])
                            slots[state["prev"]] = spare
                        ctx.build_normals(slots[state["prev"]], scale=state["prev_scale"])     # the target's normals, with ITS scale
                        with contextlib.redirect_stdout(io.StringIO()) if rank else contextlib.nullcontext():
                            rows = self._sim3_chain(ctx, mine_now, slots, state, init_poses, weight)
                    state = dd.handover_sim3_state(state, turn, dist)
                table = dd.exchange_sim3_rows(rows, n, dist)
                self.camera_poses, self.frame_index, self.scales = self._sim3_finish(table, n, scale0)
            else:
                say("\n--- Step 1: Register frames (point-to-plane ICP, frame to frame, pairs sharded by rank) ---")
                for g in resident:
                    ctx.build_normals(slot_of[g], scale=self.scales[g])
                own = [(a, b_) for a, b_ in dd.pairs_for_rank(n, world, rank)]
                local = self._register_pairs(ctx, own, slot_of, self.scales, init_poses)
                table = dd.exchange_registrations(local, n, dist)             # every rank: {cur: T, against, ok, statistics}
                # the reference's skip rule: a failed frame is dropped and its successor is re-registered against the last
                # kept frame -- by the successor's owner, one exchange per repair (failures are rare); every rank takes the
                # same decisions from the same table
                for _ in range(n):
                    kept, redo = dd.resolve_chain(table, n)
                    if redo is None:
                        break
                    want, cur = redo
                    fixed = {}
                    if lo <= cur < hi:
                        src_slot = slot_of
                        if want not in slot_of:                               # the source frame lives on another rank's GPU: bring it here
                            ctx.upload(spare, self.depths[want], self.images[want])
                            src_slot = {**slot_of, want: spare}
                        fixed = self._register_pairs(ctx, [(want, cur)], src_slot, self.scales, init_poses)
                    dd.exchange_registrations(fixed, n, dist, into=table)
                self.camera_poses, self.frame_index, self.icp_log = dd.chain_from_table(table, n)
                for e in self.icp_log:
                    say(f"\nProcessing image {e['frame']}...")
                    if e["dropped"]:
                        say(f"  Skipping - registration failed (correspondences: {e['n_corr']})")
                    else:
                        say(f"  ICP: fitness {e['fitness']:.3f}, rmse {e['rmse'] * 1e3:.2f} mm, {e['iters_run']} iterations")
            if len(self.camera_poses) < 2:
                say("Pose estimation failed")
                return None, None, None
            pose_of = dict(zip(self.frame_index, self.camera_poses))
            mine = [g for g in range(lo, hi) if g in pose_of]
            if grid is None:
                say("\n--- Step 2: Bound the scene ---")
                mn, mx = np.full(3, np.inf), np.full(3, -np.inf)
                if mine:
                    mn, mx = ctx.frames_bounds([slot_of[g] for g in mine], [pose_of[g] for g in mine], [self.scales[g] for g in mine],
                                               subsample=cfg.subsample_factor)
                mn, mx = dd.allreduce_bounds(mn, mx, dist)
                if not np.all(np.isfinite(mn)):
                    say("Reconstruction failed")
                    return None, None, None
                grid, clipped = plan_grid(mn, mx, cfg.voxel_size, cfg.grid_dim, trunc_voxels=cfg.sdf_trunc_voxels)
                if clipped:
                    say(f"  Warning: scene extent {np.round(mx - mn, 3)} m at {cfg.voxel_size} m voxels exceeds the budget of "
                        f"{cfg.grid_dim}^3 voxels; the grid {grid.dims} is centred on the scene and points outside it are dropped "
                        "(raise --grid or --voxel-size)")
                grid = choose_layout(ctx, grid, [slot_of[g] for g in mine], [pose_of[g] for g in mine], [self.scales[g] for g in mine],
                                     cfg.subsample_factor, dist=dist if world > 1 else None, log=say)
            say(f"  Grid {grid.dims} @ {grid.voxel_size * 1e3:g} mm, origin {np.round(grid.origin, 4)}")
            self.grid = grid
            ctx.attach_grid(grid)
            say(f"\n--- Step 3: Fuse depth frames (TSDF + voxel centroids), {len(mine)} of {len(pose_of)} on this rank ---")
            for g in mine:
                if grid.channels & abi.CH_TSDF:
                    ctx.integrate(slot_of[g], pose_of[g], scale=self.scales[g])
                ctx.accumulate_centroid(slot_of[g], pose_of[g], scale=self.scales[g], subsample=cfg.subsample_factor)
            say("\n--- Step 4: Merge the per-GPU grids (integer sum all-reduce) ---")
            info = dd.merge_context_grids(ctx, dist)
            if info:
                say(f"  {info['bricks_sent']} of {info['bricks_total']} bricks travelled ({info['bytes'] / 1e6:.1f} MB per rank and direction)")
            st = ctx.stats()
            tot = dd.allreduce_counts([st["centroid_points"], st["centroid_dropped"]], dist)
            xyz = rgb = None
            if rank == 0:
                say("\n--- Step 5: Extract and clean point cloud ---")
                xyz, rgb, counts = self._clean_cloud(ctx, [self._extract_points(ctx)], grid.voxel_size)
                self.stats = dict(points_accumulated=tot[0], points_dropped=tot[1], **counts)
                if cfg.cloud_normals:
                    self.timings["cloud_normals_s"] = round(self._estimate_cloud_normals(ctx, xyz, grid.voxel_size), 4)
                if getattr(cfg, "cloud_planes", False):
                    self.timings["cloud_planes_s"] = round(self._segment_cloud_planes(ctx, xyz, grid.voxel_size), 4)
                if cfg.extract_mesh:
                    t0 = time.perf_counter()
                    self.mesh = self._extract_mesh(ctx)
                    self.timings["mesh_s"] = round(time.perf_counter() - t0, 4)
                    if self._mesh_filter_on():
                        t0 = time.perf_counter()
                        self.mesh = self._filter_mesh(ctx, self.mesh)
                        self.stats["mesh_vertices"], self.stats["mesh_triangles"] = len(self.mesh[0]), len(self.mesh[2])
                        self.timings["mesh_filter_s"] = round(time.perf_counter() - t0, 4)
                    if self._mesh_simplify_on():
                        t0 = time.perf_counter()
                        self.mesh = self._simplify_mesh(ctx, self.mesh)
                        self.stats["mesh_vertices"], self.stats["mesh_triangles"] = len(self.mesh[0]), len(self.mesh[2])
                        self.timings["mesh_simplify_s"] = round(time.perf_counter() - t0, 4)
                    if self._mesh_smooth_on():
                        t0 = time.perf_counter()
                        self.mesh = self._smooth_mesh(ctx, self.mesh)
                        self.timings["mesh_smooth_s"] = round(time.perf_counter() - t0, 4)
                    if cfg.mesh_normals:
                        t0 = time.perf_counter()
                        self.mesh_normals = ctx.mesh_normals(self.mesh[0], self.mesh[2])
                        self.timings["mesh_normals_s"] = round(time.perf_counter() - t0, 4)
                if cfg.compare_to:
                    t0 = time.perf_counter()
                    self.stats["compare"] = self._compare(ctx, xyz)
                    self.timings["compare_s"] = round(time.perf_counter() - t0, 4)
                say(f"\nFinal reconstruction: {len(xyz)} points, {len(self.camera_poses)} cameras")
                xyz = xyz.astype(np.float64)
        finally:
            ctx.close()
        return xyz, rgb, self.camera_poses

    def export_frame_clouds(self, out_dir, subsample: int = 1, min_depth=None, max_depth=None):
        """Per-frame camera-space clouds like depth_processor.py writes them (DP:371-422 back-projection, DP:923-934 file):
        `<out_dir>/pointclouds/<image stem>.ply`, one per loaded frame.  Returns the number of files written."""
        from pathlib import Path
        cfg = self.config
        out = Path(out_dir) / "pointclouds"
        out.mkdir(parents=True, exist_ok=True)
        if not self.depths:
            return 0
        h, w = self.depths[0].shape
        n_written = 0
        with FusionContext(w, h, cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.min_depth if min_depth is None else min_depth,
                           cfg.max_depth if max_depth is None else max_depth, n_slots=1, grid=None, device=cfg.device) as ctx:
            for name, d, img in zip(self.image_names, self.depths, self.images):
                ctx.upload(0, d, img)
                pts, col = ctx.backproject(0, pose=None, scale=float(cfg.depth_scale), subsample=int(subsample))
                if len(pts) == 0:
                    continue                                         # DP:929-931: nothing to save
                fileio.write_ply_binary(out / f"{Path(name).stem}.ply", pts.astype(np.float64), col)
                n_written += 1
        return n_written

    def _extract_mesh(self, ctx: FusionContext):
        """marching-cubes mesh of the fused TSDF (gate: config.tsdf_min_weight); stats gain its size"""
        xyz, rgb, tris = ctx.extract_mesh(min_weight=self.config.tsdf_min_weight)
        self.stats["mesh_vertices"] = len(xyz)
        self.stats["mesh_triangles"] = len(tris)
        print(f"  Mesh: {len(xyz)} vertices, {len(tris)} triangles")
        return xyz, rgb, tris

    def _mesh_filter_on(self) -> bool:
        cfg = self.config
        return int(getattr(cfg, "mesh_min_component_triangles", 0)) > 0 or bool(getattr(cfg, "mesh_largest_component", False))

    def _check_mesh_filter_config(self):
        if self._mesh_filter_on() and not self.config.extract_mesh:
            raise ValueError("mesh_min_component_triangles / mesh_largest_component filter the mesh: they need extract_mesh = True")
        cell = float(getattr(self.config, "mesh_simplify_cell", 0.0))
        if not np.isfinite(cell) or cell < 0.0:
            raise ValueError(f"mesh_simplify_cell = {cell}: must be a finite size in metres, or 0 for none")
        if cell > 0.0 and not self.config.extract_mesh:
            raise ValueError("mesh_simplify_cell simplifies the mesh: it needs extract_mesh = True")
        placement = getattr(self.config, "mesh_simplify_placement", "mean")
        if placement not in ("mean", "quadric"):
            raise ValueError(f"mesh_simplify_placement = {placement!r}: must be 'mean' or 'quadric'")
        if placement == "quadric" and not cell > 0.0:
            raise ValueError("mesh_simplify_placement = 'quadric' places the simplified mesh's vertices: it needs mesh_simplify_cell > 0")

        it = getattr(self.config, "mesh_smooth_iterations", 0)
        lam, mu = float(getattr(self.config, "mesh_smooth_lambda", 0.5)), float(getattr(self.config, "mesh_smooth_mu", -0.53))
        if isinstance(it, bool) or int(it) != it or not 0 <= int(it) <= 1000:
            raise ValueError(f"mesh_smooth_iterations = {it}: must be a whole number in [0, 1000]")
        if not 0.0 < lam <= 1.0:                         # (false for NaN)
            raise ValueError(f"mesh_smooth_lambda = {lam}: must lie in (0, 1]")
        if not -2.0 <= mu <= 0.0:
            raise ValueError(f"mesh_smooth_mu = {mu}: must lie in [-2, 0]")
        if (int(it) > 0 or bool(getattr(self.config, "mesh_normals", False))) and not self.config.extract_mesh:
            raise ValueError("mesh_smooth_iterations / mesh_normals work on the mesh: they need extract_mesh = True")

    def _check_cloud_normals_config(self):
        cfg = self.config
        check_cloud_options(cfg)
        on = bool(getattr(cfg, "cloud_normals", False))
        if bool(getattr(cfg, "cloud_curvature", False)) and not on:
            raise ValueError("cloud_curvature comes out of the normal estimation: it needs cloud_normals = True")
        if on:
            k, radius = cfg.cloud_normals_neighbors, float(cfg.cloud_normals_radius)
            if isinstance(k, bool) or int(k) != k or not 3 <= int(k) <= 64:
                raise ValueError(f"cloud_normals_neighbors = {k}: must be a whole number in [3, 64]")
            if not np.isfinite(radius) or radius < 0.0:
                raise ValueError(f"cloud_normals_radius = {radius}: must be a finite distance in metres, or 0 for no limit")

    def _check_mesh_weld_config(self):
        mode = getattr(self.config, "mesh_weld", "host")
        if mode not in ("host", "device"):
            raise ValueError(f"mesh_weld = {mode!r}: must be 'host' or 'device'")
        if mode == "device" and not self.config.extract_mesh:
            raise ValueError("mesh_weld = 'device' welds the blocks' meshes: it needs extract_mesh = True")

    def _mesh_weld_on_device(self) -> bool:
        """config.mesh_weld == "device": the blocks' meshes are welded by FusionContext.weld_meshes, not
        by lattice.weld_meshes on the host -- the same bytes.  Only a run of more than one block welds anything."""
        return getattr(self.config, "mesh_weld", "host") == "device"

    def _mesh_smooth_on(self) -> bool:
        return int(getattr(self.config, "mesh_smooth_iterations", 0)) > 0

    def _smooth_mesh(self, ctx: FusionContext, mesh):
        """The mesh with its positions smoothed by config.mesh_smooth_iterations Taubin iterations (FusionContext.smooth_mesh,
        DESIGN.md section 4.2.3); colours and triangles are passed through.  stats["mesh_smooth"] says what ran."""
        cfg = self.config
        it, lam, mu = int(cfg.mesh_smooth_iterations), float(cfg.mesh_smooth_lambda), float(cfg.mesh_smooth_mu)
        xyz, info = ctx.smooth_mesh(mesh[0], mesh[2], it, lam=lam, mu=mu)
        self.stats["mesh_smooth"] = dict(iterations=it, mu=mu, edges=info["edges"], max_valence=info["max_valence"], **{"lambda": lam})
        print(f"  Mesh smooth: {it} iterations (lambda {lam:g}, mu {mu:g}) over {info['edges']} edges, largest valence {info['max_valence']}")
        return xyz, mesh[1], mesh[2]

    def _mesh_simplify_on(self) -> bool:
        return float(getattr(self.config, "mesh_simplify_cell", 0.0)) > 0.0

    def _simplify_mesh(self, ctx: FusionContext, mesh):
        """The mesh with the vertices of every cell of config.mesh_simplify_cell merged (FusionContext.simplify_mesh, DESIGN.md
        section 4.2.2).  The cell lattice goes through (0, 0, 0), so the result does not depend on where grids or blocks were
        placed; stats["mesh_simplify"] says what was merged and dropped.  config.mesh_simplify_placement = "quadric" puts every
        merged vertex where its triangles' planes meet instead of at the mean (reg = 2^-10), and adds the placement and its three
        counts to the stats."""
        cell = float(self.config.mesh_simplify_cell)
        placement = getattr(self.config, "mesh_simplify_placement", "mean")
        xyz, rgb, tris, info = ctx.simplify_mesh(*mesh, cell=cell, origin=(0.0, 0.0, 0.0), placement=placement)
        info.pop("vert_map")
        self.stats["mesh_simplify"] = dict(info, cell=cell, **({"placement": placement} if placement != "mean" else {}))
        quadric = (f"; quadric placement: {info['quadric_placed']} vertices, {info['clamped']} clamped, {info['corners_skipped']} corners "
                   f"skipped" if placement == "quadric" else "")
        print(f"  Mesh simplify: cell {cell:g} m, {info['vertices_in']} -> {info['clusters']} vertices, {info['triangles_in']} -> {len(tris)} "
              f"triangles ({info['degenerate_dropped']} degenerate, {info['duplicates_dropped']} duplicate){quadric}")
        return xyz, rgb, tris

    def _filter_mesh(self, ctx: FusionContext, mesh):
        """The mesh without its small connected components (config.mesh_min_component_triangles, mesh_largest_component;
        FusionContext.filter_mesh); stats["mesh_components"] says what was found and what went."""
        cfg = self.config
        xyz, rgb, tris, info = ctx.filter_mesh(*mesh, min_triangles=int(getattr(cfg, "mesh_min_component_triangles", 0)),
                                               largest_only=bool(getattr(cfg, "mesh_largest_component", False)))
        info.pop("keep_vert")
        self.stats["mesh_components"] = info
        print(f"  Mesh filter: {info['components_kept']} of {info['components']} components kept, {info['vertices_dropped']} vertices and "
              f"{info['triangles_dropped']} triangles dropped")
        return xyz, rgb, tris

    def _render_views(self, ctx: FusionContext):
        """The fused model rendered at every kept camera (FusionContext.raycast, gate config.tsdf_min_weight) into
        config.render_dir: <stem>_model_depth.npy / .png (fileio.save_depth_like_processor) and <stem>_model_color.png (RGB).
        stats gain render_views and render_residual_mm: per camera the median of |z_model - z_frame * scale| over the pixels
        valid in both, in millimetres (None when no pixel is)."""
        from pathlib import Path
        from PIL import Image
        out = Path(self.config.render_dir)
        out.mkdir(parents=True, exist_ok=True)
        residual = []
        for fi, pose in zip(self.frame_index, self.camera_poses):
            depth, _, bgr = ctx.raycast(pose, min_weight=self.config.tsdf_min_weight)
            stem = Path(self.image_names[fi]).stem
            fileio.save_depth_like_processor(depth, out, f"{stem}_model")
            Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(str(out / f"{stem}_model_color.png"))
            z = ctx.download_depth(fi).astype(np.float64) * float(self.scales[fi])
            both = (depth > 0) & np.isfinite(z) & (z > 0)
            residual.append(round(float(np.median(np.abs(depth[both] - z[both]))) * 1e3, 4) if both.any() else None)
        self.stats["render_views"] = len(residual)
        self.stats["render_residual_mm"] = residual
        print(f"  Rendered the model at {len(residual)} cameras into {out}")

    def save_mesh(self, path: str, ascii: bool = False):
        """Writes the mesh of the last reconstruct() (config.extract_mesh) as PLY (fileio.write_ply_mesh)."""
        if self.mesh is None:
            raise ValueError("no mesh: run reconstruct() with config.extract_mesh = True")
        fileio.write_ply_mesh(path, *self.mesh, ascii=ascii, normals=self.mesh_normals)
        print(f"Saved mesh to {path}")

    def save_reconstruction(self, points, colors, output_path: str, ascii: bool = False, normals=None, curvature=None, planes=None):
        fileio.save_reconstruction(points, colors, output_path, ascii=ascii, normals=normals, curvature=curvature, planes=planes)
