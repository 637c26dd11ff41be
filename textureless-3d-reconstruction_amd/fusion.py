"""FusionContext: one GPU's device-resident pipeline state (frame slots + grids) behind the C-ABI.

This is the object the reference-shaped classes in dense.py / pipeline.py drive.  It owns no numerics:
every method is one call into libtl3d.so.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _cabi as abi


@dataclass
class GridSpec:
    dims: Tuple[int, int, int]
    origin: Tuple[float, float, float]
    voxel_size: float = 0.005          # depth_to_reconstruction.py:64
    sdf_trunc: float = 0.02            # 4 voxels at the reference voxel size
    channels: int = abi.CH_TSDF | abi.CH_CENTROID
    # SPARSE grid: the channel keeps records for at most this many 8^3 bricks (4 KB / 16 KB each), handed out on first touch
    # through a brick table; 0 = dense.  dims may then describe a volume far larger than memory (what the reference's hash-map
    # merge gives for free, D2R:404-410).
    pool_tsdf: int = 0
    pool_centroid: int = 0
    # the grid is a BLOCK of a larger voxel lattice that starts at `origin`: index of its voxel (0, 0, 0) in that lattice (multiples of 8;
    # both channels, a TSDF grid within 2^23 voxels of the lattice origin -- tl3d.h: tl3d_config.voxel_offset)
    voxel_offset: Tuple[int, int, int] = (0, 0, 0)

    @property
    def sparse(self) -> bool:
        return bool(self.pool_tsdf or self.pool_centroid)

    def device_bytes(self) -> int:
        """HBM the grid takes: record pools + brick tables + free-space counters."""
        nbr = self.nvox // 512
        t = (min(self.pool_tsdf, nbr) if self.pool_tsdf else nbr) * 4096 if self.channels & abi.CH_TSDF else 0
        c = (min(self.pool_centroid, nbr) if self.pool_centroid else nbr) * 16384 if self.channels & abi.CH_CENTROID else 0
        return t + c + 12 * nbr

    @property
    def nvox(self) -> int:
        return int(self.dims[0]) * int(self.dims[1]) * int(self.dims[2])

    @staticmethod
    def cube(n: int, voxel_size: float, centre=(0.0, 0.0, 0.0), sdf_trunc: Optional[float] = None,
             channels: int = abi.CH_TSDF | abi.CH_CENTROID) -> "GridSpec":
        half = 0.5 * n * voxel_size
        return GridSpec((n, n, n), tuple(float(c) - half for c in centre), voxel_size,
                        4.0 * voxel_size if sdf_trunc is None else sdf_trunc, channels)


class PinnedArray:
    """A numpy array in page-locked host memory (tl3d_pinned_alloc): the source of asynchronous uploads."""

    def __init__(self, shape, dtype):
        self.lib = abi.load()
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        abi.check(self.lib.tl3d_pinned_alloc(self.nbytes, C.byref(p)))
        self._p = p
        buf = (C.c_char * self.nbytes).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def free(self):
        if self._p is not None:
            self.array = None
            self.lib.tl3d_pinned_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedCache:
    """Page-locked staging buffers kept between uses.  Locking and unlocking host memory costs ~1.5 ms per 10 MB each way (measured:
    a ring of 32 x 18.6 MB staging buffers 51 ms to set up, 74 ms to tear down -- a third of a 384-frame file-fed run), so the frame
    prefetcher takes its buffers from here and hands them back; at most `limit_bytes` stay cached, the rest is freed at once, and
    everything is freed when the interpreter exits.  Thread-safe (the decode workers take buffers side by side)."""
    limit_bytes = 1 << 30
    _free = {}
    _cached = 0
    _lock = None

    @classmethod
    def _lk(cls):
        if cls._lock is None:
            import atexit
            import threading
            cls._lock = threading.Lock()
            atexit.register(cls.clear)
        return cls._lock

    @classmethod
    def take(cls, shape, dtype) -> PinnedArray:
        key = (tuple(int(x) for x in shape), np.dtype(dtype).str)
        with cls._lk():
            lst = cls._free.get(key)
            if lst:
                pa = lst.pop()
                cls._cached -= pa.nbytes
                return pa
        return PinnedArray(shape, dtype)

    @classmethod
    def give(cls, pa: PinnedArray):
        if pa is None or pa._p is None:
            return
        key = (tuple(pa.array.shape), pa.array.dtype.str)
        with cls._lk():
            if cls._cached + pa.nbytes <= cls.limit_bytes:
                cls._free.setdefault(key, []).append(pa)
                cls._cached += pa.nbytes
                return
        pa.free()

    @classmethod
    def clear(cls):
        with cls._lk():
            lists, cls._free, cls._cached = list(cls._free.values()), {}, 0
        for lst in lists:
            for pa in lst:
                try:
                    pa.free()
                except Exception:
                    pass


def release_cached_memory():
    """Return what the library keeps between contexts to the system: the device frame slabs of destroyed contexts
    (tl3d_release_cached_memory) and the page-locked staging buffers of closed prefetchers (PinnedCache)."""
    PinnedCache.clear()
    abi.check(abi.load().tl3d_release_cached_memory())


# numpy images of tl3d_icp_pair / tl3d_icp_result (include/tl3d.h; sizes checked against the ctypes structures at import)
_ICP_PAIR_DT = np.dtype([("slot_src", "<i4"), ("slot_tgt", "<i4"), ("scale_src", "<f8"), ("T_init", "<f8", (16,))])
_ICP_RESULT_DT = np.dtype([("T", "<f8", (16,)), ("fitness", "<f8"), ("rmse", "<f8"), ("n_corr", "<i8"), ("n_src", "<i8"),
                           ("iters_run", "<i4"), ("status", "<i4"), ("scale", "<f8")])
_ICP_EVAL_DT = np.dtype([("A", "<f8", (21,)), ("b", "<f8", (6,)), ("e", "<f8"), ("n_corr", "<i8"), ("n_src", "<i8")])
assert _ICP_PAIR_DT.itemsize == C.sizeof(abi.IcpPair) and _ICP_RESULT_DT.itemsize == C.sizeof(abi.IcpResult)
assert _ICP_EVAL_DT.itemsize == C.sizeof(abi.IcpEval)
_RGBD_EVAL_DT = np.dtype([("geo", _ICP_EVAL_DT), ("A_p", "<f8", (21,)), ("b_p", "<f8", (6,)), ("e_p", "<f8"), ("n_photo", "<i8"),
                          ("n_qualified", "<i8")])
_RGBD_INFO_DT = np.dtype([("photo_rmse", "<f8"), ("n_photo", "<i8"), ("n_qualified", "<i8")])
assert _RGBD_EVAL_DT.itemsize == C.sizeof(abi.RgbdEval) and _RGBD_INFO_DT.itemsize == C.sizeof(abi.RgbdInfo)
_TRIU6 = np.triu_indices(6)


# ---- marshalling shared by the methods below (each said once) ------------------------------------------------------------
def _grid_config(grid: GridSpec, cfg=None):
    """`cfg` (default: a fresh abi.Config) with the grid fields of tl3d_config filled from a GridSpec."""
    if cfg is None:
        cfg = abi.Config()
        cfg.abi_version = abi.ABI_VERSION
    cfg.channels = int(grid.channels)
    cfg.nx, cfg.ny, cfg.nz = (int(d) for d in grid.dims)
    cfg.origin = (C.c_double * 3)(*[float(o) for o in grid.origin])
    cfg.voxel_size, cfg.sdf_trunc = float(grid.voxel_size), float(grid.sdf_trunc)
    cfg.pool_bricks_tsdf, cfg.pool_bricks_centroid = int(grid.pool_tsdf), int(grid.pool_centroid)
    cfg.voxel_offset = (C.c_int64 * 3)(*[int(o) for o in grid.voxel_offset])
    return cfg


def _frame_arrays(slots, poses, scales):
    """(slots int32 [n], R float64 [n,3,3], t float64 [n,3], scales float64 [n]) of many frames; poses: one (R, t) per frame."""
    sl = np.ascontiguousarray(slots, np.int32)
    R = np.ascontiguousarray(np.stack([np.asarray(p[0], np.float64).reshape(3, 3) for p in poses]))
    t = np.ascontiguousarray(np.stack([np.asarray(p[1], np.float64).reshape(3) for p in poses]))
    sc = np.ascontiguousarray(np.ones(len(slots)) if scales is None else np.asarray(scales, np.float64))
    return sl, R, t, sc


def _icp_params(kw) -> "abi.IcpParams":
    """tl3d_icp_params from a level dict (the keywords of icp(), with its defaults)."""
    return abi.IcpParams(int(kw.get("iters", 10)), int(kw.get("stride", 4)), float(kw.get("max_dist", 0.05)),
                         float(kw.get("damping", 1e-6)), float(kw.get("eps", 1e-9)), float(kw.get("eig_rel", 1e-4)),
                         1 if kw.get("estimate_scale", False) else 0, 0)


def _icp_levels(levels):
    lv = (abi.IcpParams * max(1, len(levels)))()
    for i, kw in enumerate(levels):
        lv[i] = _icp_params(kw)
    return lv


def _icp_result_dicts(res, n: int = 1) -> list:
    """The first n of tl3d_icp_result records (a numpy record array, or one ctypes structure) as the dicts icp() returns."""
    if not isinstance(res, np.ndarray):
        res = np.frombuffer(res, _ICP_RESULT_DT)
    T = res["T"].reshape(-1, 4, 4)
    fit, rmse, nc, ns, it, st, sc = (res[k].tolist() for k in ("fitness", "rmse", "n_corr", "n_src", "iters_run", "status", "scale"))
    return [dict(T=T[i], fitness=fit[i], rmse=rmse[i], n_corr=nc[i], n_src=ns[i], iters_run=it[i], status=st[i], scale=sc[i])
            for i in range(n)]


def _pair_records(pairs, T_init, scales):
    """The request as one numpy record array laid out like tl3d_icp_pair (a Python loop over ctypes fields costs ~10 us per pair:
    as much as the registration of a pair inside a large batch).  T_init: one 4x4 per pair, None entries = identity."""
    n = len(pairs)
    arr = np.zeros(n, _ICP_PAIR_DT)
    pr = np.asarray(pairs, np.int64).reshape(n, 2)
    arr["slot_src"], arr["slot_tgt"] = pr[:, 0], pr[:, 1]
    arr["scale_src"] = 1.0 if scales is None else np.asarray(scales, np.float64)
    arr["T_init"] = np.eye(4).ravel()
    if T_init is not None:
        for i, T0 in enumerate(T_init):
            if T0 is not None:
                arr["T_init"][i] = np.asarray(T0, np.float64).reshape(16)
    return arr


def _eval_dicts(res, n: int = 1) -> list:
    """The first n of tl3d_icp_eval records (a numpy record array, or one ctypes structure) as the dicts icp_evaluate() returns:
    the packed upper triangle unfolded into the symmetric 6 x 6 A, and the statistics derived from the sums."""
    if not isinstance(res, np.ndarray):
        res = np.frombuffer(res, _ICP_EVAL_DT)
    A = np.zeros((n, 6, 6))
    A[:, _TRIU6[0], _TRIU6[1]] = res["A"][:n]
    A[:, _TRIU6[1], _TRIU6[0]] = res["A"][:n]
    out = []
    for i in range(n):
        nc, ns, e = int(res["n_corr"][i]), int(res["n_src"][i]), float(res["e"][i])
        out.append(dict(A=A[i], b=res["b"][i].copy(), e=e, n_corr=nc, n_src=ns, fitness=nc / ns if ns > 0 else 0.0,
                        rmse=float(np.sqrt(e / nc)) if nc > 0 else 0.0))
    return out


class FusionContext:
    def __init__(self, width: int, height: int, fx: float, fy: float, cx: float, cy: float,
                 min_depth: float = 0.1, max_depth: float = 50.0, n_slots: int = 2,
                 grid: Optional[GridSpec] = None, device: int = 0, ext_tsdf=None, ext_centroid=None, stream=None):
        self._h = None
        lib = abi.load()
        if abi.device_count() <= 0:
            raise RuntimeError("libtl3d: no HIP device visible; the MI355X path has no CPU fallback")
        cfg = abi.Config()
        cfg.abi_version = abi.ABI_VERSION
        cfg.width, cfg.height = int(width), int(height)
        cfg.fx, cfg.fy, cfg.cx, cfg.cy = float(fx), float(fy), float(cx), float(cy)
        cfg.min_depth, cfg.max_depth = float(min_depth), float(max_depth)
        cfg.n_slots = int(n_slots)
        if grid is not None:
            _grid_config(grid, cfg)
        cfg.ext_tsdf = abi.ptr(ext_tsdf)
        cfg.ext_centroid = abi.ptr(ext_centroid)
        cfg.stream = abi.ptr(stream)
        self._keep = (ext_tsdf, ext_centroid)
        h = C.c_void_p()
        abi.check(lib.tl3d_create(C.byref(cfg), int(device), C.byref(h)))
        self._h, self._lib = h, lib
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self.grid = grid
        self.device = int(device)
        self.n_slots = int(n_slots)
        self.last_normals_degenerate = 0           # degenerate neighbourhoods of the last estimate_normals()

    # ---- lifetime --------------------------------------------------------------------------
    def close(self):
        if self._h is not None:
            self._lib.tl3d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        abi.check(self._lib.tl3d_sync(self._h))

    def stream_ptr(self) -> int:
        """The hipStream_t the context enqueues on, as an integer (torch.cuda.ExternalStream takes it)."""
        p = C.c_void_p()
        abi.check(self._lib.tl3d_get_stream(self._h, C.byref(p)))
        return int(p.value or 0)

    # ---- frames ----------------------------------------------------------------------------
    def upload(self, slot: int, depth, bgr=None):
        """depth: float32 [H,W] metres / relative units, or uint16 [H,W] millimetres (16-bit PNG, D2R:85-90)."""
        if isinstance(depth, np.ndarray):
            if depth.dtype == np.uint16:
                kind = abi.DEPTH_U16_MM
            else:
                depth = np.ascontiguousarray(depth, dtype=np.float32)
                kind = abi.DEPTH_F32_M
            depth = np.ascontiguousarray(depth)
            assert depth.shape == (self.height, self.width), f"depth {depth.shape} != {(self.height, self.width)}"
        else:                                   # torch tensor (host or device)
            import torch
            kind = abi.DEPTH_U16_MM if depth.dtype in (torch.uint16, torch.int16) else abi.DEPTH_F32_M
            assert tuple(depth.shape) == (self.height, self.width)
        if bgr is not None:
            if isinstance(bgr, np.ndarray):
                bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
            assert tuple(bgr.shape) == (self.height, self.width, 3), f"colour {tuple(bgr.shape)}"
        abi.check(self._lib.tl3d_upload_frame(self._h, int(slot), abi.ptr(depth), kind, abi.ptr(bgr)))

    def upload_async(self, slot: int, depth, bgr=None):
        """Enqueue the copies and return; `depth` / `bgr` (ideally pinned, see pinned_array) must stay untouched until
        slot_wait(slot).  Device work that reads the slot is ordered after the copy automatically."""
        kind = abi.DEPTH_U16_MM if depth.dtype == np.uint16 else abi.DEPTH_F32_M
        assert depth.flags["C_CONTIGUOUS"] and depth.shape == (self.height, self.width)
        assert bgr is None or (bgr.flags["C_CONTIGUOUS"] and bgr.shape == (self.height, self.width, 3) and bgr.dtype == np.uint8)
        abi.check(self._lib.tl3d_upload_frame_async(self._h, int(slot), abi.ptr(depth), kind, abi.ptr(bgr)))

    def slot_wait(self, slot: int):
        abi.check(self._lib.tl3d_slot_wait(self._h, int(slot)))

    def attach_grid(self, grid: "GridSpec", ext_tsdf=None, ext_centroid=None):
        """Give a grid-less context its fusion grid (frames stay resident across registration and fusion)."""
        cfg = _grid_config(grid)
        cfg.ext_tsdf, cfg.ext_centroid = abi.ptr(ext_tsdf), abi.ptr(ext_centroid)
        abi.check(self._lib.tl3d_attach_grid(self._h, C.byref(cfg)))
        self._keep = (ext_tsdf, ext_centroid)
        self.grid = grid

    def detach_grid(self):
        """Free the grid (channels, brick tables, grid-sized scratch); frames, normal maps and ICP state stay, and attach_grid
        works again (tl3d.h: tl3d_detach_grid)."""
        abi.check(self._lib.tl3d_detach_grid(self._h))
        self._keep = (None, None)
        self.grid = None

    def set_block_core(self, lattice_dims=None, lo=None, hi=None):
        """The attached grid is one block of a lattice of `lattice_dims` voxels; extraction, the mesh and the centroid statistics
        keep to the core [lo, hi) (grid-local voxels, multiples of 8).  No arguments: no core (tl3d.h: tl3d_set_block_core)."""
        if lattice_dims is None:
            abi.check(self._lib.tl3d_set_block_core(self._h, None, None, None))
            return
        ld = np.ascontiguousarray([int(x) for x in lattice_dims], np.int64)
        lo_ = np.ascontiguousarray([int(x) for x in lo], np.int32)
        hi_ = np.ascontiguousarray([int(x) for x in hi], np.int32)
        abi.check(self._lib.tl3d_set_block_core(self._h, abi.ptr(ld), abi.ptr(lo_), abi.ptr(hi_)))

    def download_depth(self, slot: int) -> np.ndarray:
        out = np.empty((self.height, self.width), np.float32)
        abi.check(self._lib.tl3d_download_depth(self._h, int(slot), abi.ptr(out)))
        return out

    # ---- depth-frame filter (needs no grid) ---------------------------
    DEPTH_FILTER_COUNTS = ("valid", "removed_flying", "regions", "removed_regions")

    @staticmethod
    def _depth_filter_params(jump_rel, radius, min_support, min_region) -> "abi.DepthFilterParams":
        return abi.DepthFilterParams(jump_rel=float(jump_rel), radius=int(radius), min_support=int(min_support),
                                     min_region=int(min_region), reserved=0)

    def filter_depth(self, depth, jump_rel=0.05, radius=1, min_support=4, min_region=0, out=None):
        """(filtered, counts): one depth image [H,W] (numpy or torch, host or device; float32, or uint16 millimetres) with its
        flying pixels and small regions set to 0; every other pixel, an invalid one too, keeps its bits.  A valid pixel (finite,
        > 0) is linked to a valid neighbour when |d_q - d_p| <= jump_rel * min(d_p, d_q) in f32; it goes when fewer than
        min_support pixels of its (2 radius + 1)^2 window are linked to it, and then when its 4-connected region of linked
        survivors has fewer than min_region pixels (0 or 1: no such stage).  counts = dict(valid, removed_flying, regions,
        removed_regions).  out: an array like depth to write into (depth itself filters in place); default a new one."""
        if isinstance(depth, np.ndarray):
            if depth.dtype != np.uint16:
                depth = np.ascontiguousarray(depth, dtype=np.float32)
            depth = np.ascontiguousarray(depth)
            kind = abi.DEPTH_U16_MM if depth.dtype == np.uint16 else abi.DEPTH_F32_M
            if out is None:
                out = np.empty_like(depth)
        else:
            import torch
            kind = abi.DEPTH_U16_MM if depth.dtype in (torch.uint16, torch.int16) else abi.DEPTH_F32_M
            if kind == abi.DEPTH_F32_M and depth.dtype != torch.float32:
                depth = depth.to(torch.float32)
            depth = depth.contiguous()
            if out is None:
                out = torch.empty_like(depth)
        assert tuple(depth.shape) == (self.height, self.width), f"depth {tuple(depth.shape)} != {(self.height, self.width)}"
        def item(a):
            return a.itemsize if isinstance(a, np.ndarray) else a.element_size()
        assert tuple(out.shape) == tuple(depth.shape) and item(out) == item(depth), "out must match depth in shape and element size"
        prm = self._depth_filter_params(jump_rel, radius, min_support, min_region)
        cnt = (C.c_int64 * 4)()
        abi.check(self._lib.tl3d_filter_depth(self._h, abi.ptr(depth), kind, C.byref(prm), abi.ptr(out), cnt))
        return out, dict(zip(self.DEPTH_FILTER_COUNTS, (int(c) for c in cnt)))

    def filter_depth_slots(self, slots, jump_rel=0.05, radius=1, min_support=4, min_region=0, counts=True):
        """Filters the resident frames `slots` in place by the rule of filter_depth (a uint16 frame on its millimetres), each as a
        new upload of its slot: normal maps and everything cached from the old image are void.  Returns the counts as int64 [n, 4]
        (valid, removed_flying, regions, removed_regions per slot), or None with counts=False (the call then does not wait)."""
        sl = np.ascontiguousarray([int(s) for s in slots], np.int32)
        prm = self._depth_filter_params(jump_rel, radius, min_support, min_region)
        cnt = np.zeros((len(sl), 4), np.int64) if counts else None
        abi.check(self._lib.tl3d_filter_depth_slots(self._h, len(sl), abi.ptr(sl) if len(sl) else None, C.byref(prm), abi.ptr(cnt)))
        return cnt

    # ---- a4/a5 -----------------------------------------------------------------------------
    @staticmethod
    def _pose_args(pose, flags):
        if pose is None:
            return abi.d9(np.eye(3)), abi.d3(np.zeros(3)), flags | abi.F_NO_POSE
        r, t = pose
        return abi.d9(r), abi.d3(t), flags

    def _depth_range(self, min_depth, max_depth):
        return (self.min_depth if min_depth is None else float(min_depth), self.max_depth if max_depth is None else float(max_depth))

    def backproject(self, slot: int, pose=None, scale=1.0, subsample: int = 1, min_depth=None, max_depth=None,
                    scale_f64: bool = False):
        r, t, flags = self._pose_args(pose, abi.F_SCALE_F64 if scale_f64 else 0)
        mn, mx = self._depth_range(min_depth, max_depth)
        cap = -(-self.height // subsample) * -(-self.width // subsample)
        xyz = np.empty((cap, 3), np.float32)
        rgb = np.empty((cap, 3), np.uint8)
        n = C.c_int64(0)
        abi.check(self._lib.tl3d_backproject(self._h, int(slot), abi.ptr(r), abi.ptr(t), float(scale), flags,
                                             int(subsample), mn, mx, abi.ptr(xyz), abi.ptr(rgb), cap, C.byref(n)))
        return xyz[:n.value], rgb[:n.value]

    def backproject_device(self, slot: int, out_xyz, out_rgb, out_n, pose=None, scale=1.0, subsample: int = 1,
                           min_depth=None, max_depth=None, scale_f64: bool = False, cap=None):
        """Asynchronous, device-only form: out_xyz (float32 [cap,3]), out_rgb (uint8 [cap,3]) and out_n (int64 [1]) are
        device tensors (anything with data_ptr()); nothing is read back, the call returns once its kernel is enqueued."""
        r, t, flags = self._pose_args(pose, abi.F_SCALE_F64 if scale_f64 else 0)
        mn, mx = self._depth_range(min_depth, max_depth)
        cap = int(out_xyz.shape[0]) if cap is None else int(cap)
        abi.check(self._lib.tl3d_backproject_device(self._h, int(slot), abi.ptr(r), abi.ptr(t), float(scale), flags, int(subsample),
                                                    mn, mx, abi.ptr(out_xyz), abi.ptr(out_rgb), cap, abi.ptr(out_n)))

    def frame_bounds(self, slot: int, pose=None, scale=1.0, subsample: int = 1, min_depth=None, max_depth=None, scale_f64: bool = False):
        """(min[3], max[3]) of the points backproject() would return, computed on the device (+-inf when there are none)."""
        r, t, flags = self._pose_args(pose, abi.F_SCALE_F64 if scale_f64 else 0)
        mn_d, mx_d = self._depth_range(min_depth, max_depth)
        lo, hi = np.zeros(3), np.zeros(3)
        abi.check(self._lib.tl3d_frame_bounds(self._h, int(slot), abi.ptr(r), abi.ptr(t), float(scale), flags, int(subsample), mn_d, mx_d,
                                              abi.ptr(lo), abi.ptr(hi), None))
        return lo, hi

    def frames_bounds(self, slots, poses, scales=None, subsample: int = 1, min_depth=None, max_depth=None):
        """(min[3], max[3]) over the clouds of many frames (poses: one (R, t) per frame), one read-back per 16 frames."""
        n = len(slots)
        sl, R, t, sc = _frame_arrays(slots, poses, scales)
        mn_d, mx_d = self._depth_range(min_depth, max_depth)
        lo, hi = np.zeros(3), np.zeros(3)
        abi.check(self._lib.tl3d_frames_bounds(self._h, n, abi.ptr(sl), abi.ptr(R), abi.ptr(t), abi.ptr(sc), 0, int(subsample), mn_d, mx_d,
                                               abi.ptr(lo), abi.ptr(hi)))
        return lo, hi

    def count_bricks(self, grid: "GridSpec", slots, poses, scales=None, centroid_subsample: int = 1, min_depth=None, max_depth=None):
        """(TSDF bricks, centroid bricks) a fusion of these frames into `grid` would give records to -- geometry only, nothing is
        allocated or written: what a sparse grid's pools must hold (tl3d.h: tl3d_count_bricks)."""
        n = len(slots)
        cfg = _grid_config(grid)                 # (the pool sizes are not read: the count is what sizes them)
        sl, R, t, sc = _frame_arrays(slots, poses, scales)
        mn_d, mx_d = self._depth_range(min_depth, max_depth)
        nt, nc = C.c_int64(0), C.c_int64(0)
        abi.check(self._lib.tl3d_count_bricks(self._h, C.byref(cfg), n, abi.ptr(sl), abi.ptr(R), abi.ptr(t), abi.ptr(sc), int(centroid_subsample),
                                              mn_d, mx_d, C.byref(nt), C.byref(nc)))
        return int(nt.value), int(nc.value)

    def tile_cache_info(self):
        """(builds, hits, bytes) of the per-slot TSDF tile cache (tl3d.h: tl3d_tile_cache_info)."""
        b, h, m = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        abi.check(self._lib.tl3d_tile_cache_info(self._h, C.byref(b), C.byref(h), C.byref(m)))
        return int(b.value), int(h.value), int(m.value)

    def class_cache_info(self):
        """(classified, replayed, overflowed, bytes) of the per-slot TSDF classification cache, counts per frame (tl3d.h: tl3d_class_cache_info)."""
        c, r, o, m = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        abi.check(self._lib.tl3d_class_cache_info(self._h, C.byref(c), C.byref(r), C.byref(o), C.byref(m)))
        return int(c.value), int(r.value), int(o.value), int(m.value)

    def class_refine_info(self):
        """(seen, dropped, freed, decided, overflowed): (frame, sub-brick) pairs the refinement of replayed classification entries
        tested and what it decided for them (tl3d.h: tl3d_class_refine_info)."""
        v = [C.c_uint64(0) for _ in range(5)]
        abi.check(self._lib.tl3d_class_refine_info(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    # ---- fusion ----------------------------------------------------------------------------
    def accumulate_centroid(self, slot: int, pose=None, scale=1.0, subsample: int = 1, min_depth=None, max_depth=None,
                            scale_f64: bool = False):
        r, t, flags = self._pose_args(pose, abi.F_SCALE_F64 if scale_f64 else 0)
        mn, mx = self._depth_range(min_depth, max_depth)
        abi.check(self._lib.tl3d_accumulate_centroid(self._h, int(slot), abi.ptr(r), abi.ptr(t), float(scale), flags,
                                                     int(subsample), mn, mx))

    def accumulate_points(self, xyz, rgb):
        if isinstance(xyz, np.ndarray):
            xyz = np.ascontiguousarray(xyz, dtype=np.float32)
            rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        n = int(xyz.shape[0])
        abi.check(self._lib.tl3d_accumulate_points(self._h, abi.ptr(xyz), abi.ptr(rgb), n))

    def points_bounds(self, xyz):
        if isinstance(xyz, np.ndarray):
            xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        mn, mx = np.zeros(3), np.zeros(3)
        abi.check(self._lib.tl3d_points_bounds(self._h, abi.ptr(xyz), int(xyz.shape[0]), abi.ptr(mn), abi.ptr(mx)))
        return mn, mx

    def integrate(self, slot: int, pose, scale=1.0):
        r, t = pose
        abi.check(self._lib.tl3d_integrate(self._h, int(slot), abi.ptr(abi.d9(r)), abi.ptr(abi.d3(t)), float(scale)))

    def fuse_frames(self, slots, poses, scales=None, centroid_subsample: int = 0, min_depth=None, max_depth=None):
        """integrate() (and accumulate_centroid() when centroid_subsample >= 1) of many frames in one call, in order."""
        n = len(slots)
        if n == 0:
            return
        sl, R, t, sc = _frame_arrays(slots, poses, scales)
        mn_d, mx_d = self._depth_range(min_depth, max_depth)
        abi.check(self._lib.tl3d_fuse_frames(self._h, n, abi.ptr(sl), abi.ptr(R), abi.ptr(t), abi.ptr(sc), 0, int(centroid_subsample), mn_d, mx_d))

    def fuse_frames_packed(self, slots_i32, R_f64, t_f64, scales_f64=None, centroid_subsample: int = 0):
        """fuse_frames() on arrays the caller has already packed (int32 [n], float64 [n,9], float64 [n,3], float64 [n]): a
        long-running loop pays the packing once."""
        n = int(slots_i32.shape[0])
        if n == 0:
            return
        sc = scales_f64 if scales_f64 is not None else np.ones(n)
        abi.check(self._lib.tl3d_fuse_frames(self._h, n, abi.ptr(slots_i32), abi.ptr(R_f64), abi.ptr(t_f64), abi.ptr(sc), 0,
                                             int(centroid_subsample), self.min_depth, self.max_depth))

    # ---- ICP -------------------------------------------------------------------------------
    def build_normals_many(self, slots, scales=None, depth_jump=0.05):
        n = len(slots)
        if n == 0:
            return
        sl = np.ascontiguousarray(slots, np.int32)
        sc = None if scales is None else np.ascontiguousarray(np.asarray(scales, np.float64))
        abi.check(self._lib.tl3d_build_normals_many(self._h, n, abi.ptr(sl), None if sc is None else abi.ptr(sc), float(depth_jump)))

    def set_normal_smoothing(self, radius: int):
        """Normal maps built from now on use the window-averaged depth (radius 1 = 3 x 3), and registrations read it as their
        source depth: robust to depth noise (tl3d.h: tl3d_set_normal_smoothing); 0 = off."""
        abi.check(self._lib.tl3d_set_normal_smoothing(self._h, int(radius)))

    def build_normals(self, slot: int, scale=1.0, depth_jump=0.05):
        abi.check(self._lib.tl3d_build_normals(self._h, int(slot), float(scale), float(depth_jump)))

    def download_normals(self, slot: int, out=None) -> np.ndarray:
        """The slot's normal map as a row-major [H][W][4] image (nx, ny, nz, depth); out: a host array or a device tensor of that
        shape to fill instead (the library keeps the map in phase-major rows and converts on the way out)."""
        if out is None:
            out = np.empty((self.height, self.width, 4), np.float32)
        abi.check(self._lib.tl3d_download_normals(self._h, int(slot), abi.ptr(out)))
        return out

    def icp(self, slot_src: int, slot_tgt: int, T_init=None, iters=10, stride=4, max_dist=0.05, damping=1e-6,
            eps=1e-9, scale_src=1.0, eig_rel=1e-4, estimate_scale=False):
        """Point-to-plane ICP; returns T (src camera -> tgt camera) and statistics.  With src = previous frame and
        tgt = current frame, (T[:3,:3], T[:3,3]) is (R_rel, t_rel) of depth_to_reconstruction.py:618-620."""
        T0 = np.ascontiguousarray(np.eye(4) if T_init is None else np.asarray(T_init, np.float64).reshape(4, 4))
        prm = _icp_params(dict(iters=iters, stride=stride, max_dist=max_dist, damping=damping, eps=eps, eig_rel=eig_rel, estimate_scale=estimate_scale))
        res = abi.IcpResult()
        abi.check(self._lib.tl3d_icp_p2plane(self._h, int(slot_src), float(scale_src), int(slot_tgt), abi.ptr(T0),
                                             C.byref(prm), C.byref(res)))
        return _icp_result_dicts(res)[0]

    def icp_enqueue(self, lane: int, slot_src: int, slot_tgt: int, T_init=None, iters=10, stride=4, max_dist=0.05,
                    damping=1e-6, eps=1e-9, scale_src=1.0, eig_rel=1e-4, estimate_scale=False):
        """Asynchronous form: up to abi.ICP_LANES independent registrations in flight (one per lane)."""
        T0 = np.ascontiguousarray(np.eye(4) if T_init is None else np.asarray(T_init, np.float64).reshape(4, 4))
        prm = _icp_params(dict(iters=iters, stride=stride, max_dist=max_dist, damping=damping, eps=eps, eig_rel=eig_rel, estimate_scale=estimate_scale))
        abi.check(self._lib.tl3d_icp_enqueue(self._h, int(lane), int(slot_src), float(scale_src), int(slot_tgt), abi.ptr(T0),
                                             C.byref(prm)))

    def icp_collect(self, lane: int):
        res = abi.IcpResult()
        abi.check(self._lib.tl3d_icp_collect(self._h, int(lane), C.byref(res)))
        return _icp_result_dicts(res)[0]

    def icp_batch_enqueue(self, pairs, levels, T_init=None, scales=None):
        """Register every (slot_src, slot_tgt) of `pairs` through all of `levels` in ONE launch (asynchronous).

        levels: sequence of dicts with the keyword arguments of icp() (iters, stride, max_dist, damping, eps, eig_rel),
        coarse to fine.  T_init: one 4x4 per pair (default identity); scales: metric scale of each pair's source depth."""
        n = len(pairs)
        arr = _pair_records(pairs, T_init, scales)
        lv = _icp_levels(levels)
        abi.check(self._lib.tl3d_icp_batch_enqueue(self._h, arr.ctypes.data_as(C.POINTER(abi.IcpPair)), n, lv, len(levels)))
        self._icp_batch_n = n

    def icp_batch_collect(self):
        n = getattr(self, "_icp_batch_n", 0)
        res = np.zeros(max(1, n), _ICP_RESULT_DT)
        abi.check(self._lib.tl3d_icp_batch_collect(self._h, res.ctypes.data_as(C.POINTER(abi.IcpResult)), n))
        self._icp_batch_n = 0
        return _icp_result_dicts(res, n)

    def icp_batch(self, pairs, levels, T_init=None, scales=None):
        self.icp_batch_enqueue(pairs, levels, T_init, scales)
        return self.icp_batch_collect()

    def icp_evaluate(self, pairs, T, stride=2, max_dist=0.05, scales=None):
        """One point-to-plane pass for every (slot_src, slot_tgt) of `pairs` at the pose T[i] (src camera -> tgt camera), no update
        (tl3d_icp_evaluate_pairs).  Returns one dict per pair: A (6 x 6, sum J J^T with J = [p x n, n]: the weight of the pair as an
        edge of a pose graph), b (sum J r), e (sum r^2), n_corr, n_src, fitness = n_corr / n_src, rmse = sqrt(e / n_corr).
        T: one 4x4 per pair (None entries = identity); scales: metric scale of each pair's source depth."""
        n = len(pairs)
        arr = _pair_records(pairs, T, scales)
        res = np.zeros(max(1, n), _ICP_EVAL_DT)
        abi.check(self._lib.tl3d_icp_evaluate_pairs(self._h, arr.ctypes.data_as(C.POINTER(abi.IcpPair)), n, int(stride), float(max_dist),
                                                    res.ctypes.data_as(C.POINTER(abi.IcpEval))))
        return _eval_dicts(res, n)

    # ---- joint point-to-plane + photometric registration -------------
    def build_intensity(self, slots, radius=1, depth_jump=0.05):
        """The intensity maps of `slots` (one slot or a sequence), from each slot's colour image and depth
        (tl3d_build_intensity_many): what rgbd_evaluate / rgbd_register read on both sides of a pair."""
        sl = np.ascontiguousarray(np.atleast_1d(np.asarray(slots, np.int32)))
        abi.check(self._lib.tl3d_build_intensity_many(self._h, len(sl), abi.ptr(sl), int(radius), float(depth_jump)))

    def download_intensity(self, slot: int, out=None) -> np.ndarray:
        """The slot's intensity map as a row-major [H][W][4] image (S, Sx, Sy, flag); out: a host array or a device tensor to fill."""
        if out is None:
            out = np.empty((self.height, self.width, 4), np.float32)
        abi.check(self._lib.tl3d_download_intensity(self._h, int(slot), abi.ptr(out)))
        return out

    def rgbd_evaluate(self, pairs, T, stride=2, max_dist=0.05, photo_gate=0.2, scales=None):
        """One pass of the geometric AND the photometric system for every (slot_src, slot_tgt) of `pairs` at the pose T[i], no update
        (tl3d_rgbd_evaluate_pairs).  One dict per pair: icp_evaluate's keys for the geometric system (A, b, e, n_corr, n_src,
        fitness, rmse) plus A_p (6 x 6), b_p, e_p, n_photo, n_qualified and photo_rmse = sqrt(e_p / n_photo)."""
        n = len(pairs)
        arr = _pair_records(pairs, T, scales)
        res = np.zeros(max(1, n), _RGBD_EVAL_DT)
        abi.check(self._lib.tl3d_rgbd_evaluate_pairs(self._h, arr.ctypes.data_as(C.POINTER(abi.IcpPair)), n, int(stride), float(max_dist),
                                                     float(photo_gate), res.ctypes.data_as(C.POINTER(abi.RgbdEval))))
        out = _eval_dicts(np.ascontiguousarray(res["geo"]), n)
        for i, d in enumerate(out):
            A_p = np.zeros((6, 6))
            A_p[_TRIU6] = res["A_p"][i]
            A_p = A_p + np.triu(A_p, 1).T
            n_photo, e_p = int(res["n_photo"][i]), float(res["e_p"][i])
            d.update(A_p=A_p, b_p=res["b_p"][i].copy(), e_p=e_p, n_photo=n_photo, n_qualified=int(res["n_qualified"][i]),
                     photo_rmse=float(np.sqrt(e_p / n_photo)) if n_photo > 0 else 0.0)
        return out

    def rgbd_register(self, pairs, levels, T_init=None, scales=None):
        """Register every (slot_src, slot_tgt) of `pairs` through `levels`, coarse to fine, with the photometric term beside the
        point-to-plane one (tl3d_rgbd_register_pairs; blocks).  levels: dicts with icp()'s keywords (estimate_scale is refused) plus
        photo_weight (default 0.1) and photo_gate (default 0.2).  One dict per pair like icp_batch's, plus photo_rmse, n_photo and
        n_qualified of the final pass."""
        n = len(pairs)
        arr = _pair_records(pairs, T_init, scales)
        lv = (abi.RgbdLevel * max(1, len(levels)))()
        for i, kw in enumerate(levels):
            lv[i] = abi.RgbdLevel(_icp_params(kw), float(kw.get("photo_weight", 0.1)), float(kw.get("photo_gate", 0.2)))
        res = np.zeros(max(1, n), _ICP_RESULT_DT)
        info = np.zeros(max(1, n), _RGBD_INFO_DT)
        abi.check(self._lib.tl3d_rgbd_register_pairs(self._h, arr.ctypes.data_as(C.POINTER(abi.IcpPair)), n, lv, len(levels),
                                                     res.ctypes.data_as(C.POINTER(abi.IcpResult)), info.ctypes.data_as(C.POINTER(abi.RgbdInfo))))
        out = _icp_result_dicts(res, n)
        for i, d in enumerate(out):
            d.update(photo_rmse=float(info["photo_rmse"][i]), n_photo=int(info["n_photo"][i]), n_qualified=int(info["n_qualified"][i]))
        return out

    def track_evaluate(self, slot: int, pose, stride=2, max_dist=0.05, min_weight: int = 1, scale=1.0):
        """One point-to-SDF pass of the frame in `slot` against the TSDF channel at pose = (R, t) (world->camera, as integrate), no
        update (tl3d_track_evaluate).  A dict like icp_evaluate's: A (6 x 6, sum J J^T, J = [p x n, n] with n the
        field's gradient in the camera frame), b (sum J r), e (sum r^2, r in metres), n_corr, n_src, fitness, rmse."""
        r, t = abi.d9(pose[0]), abi.d3(pose[1])
        res = abi.IcpEval()
        abi.check(self._lib.tl3d_track_evaluate(self._h, int(slot), float(scale), abi.ptr(r), abi.ptr(t), int(min_weight), int(stride),
                                                float(max_dist), C.byref(res)))
        return _eval_dicts(res)[0]

    def track(self, slot: int, pose_init, levels, min_weight: int = 1, scale=1.0):
        """Register the frame in `slot` against the TSDF channel, starting at pose_init = (R, t) (world->camera), through `levels`
        coarse to fine (dicts with icp()'s keywords: iters, stride, max_dist -- the gate on the signed distance --, damping, eps,
        eig_rel), all on the device (tl3d_track_frame).  A dict like icp()'s, T being the world->camera pose, plus pose = (R, t);
        status 2 (fewer than 8 correspondences or a singular system) leaves the last good pose."""
        r, t = abi.d9(pose_init[0]), abi.d3(pose_init[1])
        lv = _icp_levels(levels)
        res = abi.IcpResult()
        abi.check(self._lib.tl3d_track_frame(self._h, int(slot), float(scale), abi.ptr(r), abi.ptr(t), int(min_weight), lv, len(levels),
                                             C.byref(res)))
        out = _icp_result_dicts(res)[0]
        return dict(out, pose=(out["T"][:3, :3].copy(), out["T"][:3, 3].copy()))

    # ---- grids -----------------------------------------------------------------------------
    def reset(self):
        abi.check(self._lib.tl3d_grid_reset(self._h))

    def grid_ptr(self, channel: int):
        p, nb = C.c_void_p(), C.c_size_t()
        abi.check(self._lib.tl3d_grid_device_ptr(self._h, int(channel), C.byref(p), C.byref(nb)))
        return p.value, nb.value

    def _channel_bytes(self, channel: int) -> int:
        return self.grid.nvox * (8 if channel == abi.CH_TSDF else 32)

    def download_grid(self, channel: int) -> np.ndarray:
        """The channel as a dense array in record order (a sparse grid is gathered through its brick table: the same image)."""
        nb = self._channel_bytes(channel)
        if channel == abi.CH_TSDF:
            out = np.empty((nb // 8, 2), np.int32)
        else:
            out = np.empty((nb // 32, 4), np.uint64)
        abi.check(self._lib.tl3d_grid_download(self._h, int(channel), abi.ptr(out), nb))
        return out

    def upload_grid(self, channel: int, arr):
        nb = self._channel_bytes(channel)
        if isinstance(arr, np.ndarray):
            arr = np.ascontiguousarray(arr)
            assert arr.nbytes == nb
        abi.check(self._lib.tl3d_grid_upload(self._h, int(channel), abi.ptr(arr), nb))

    def add_grid(self, channel: int, arr):
        nb = self._channel_bytes(channel)
        if isinstance(arr, np.ndarray):
            arr = np.ascontiguousarray(arr)
            assert arr.nbytes == nb
        abi.check(self._lib.tl3d_grid_add(self._h, int(channel), abi.ptr(arr), nb))

    # ---- sparse merge helpers (device tensors: anything with data_ptr()) ---------------------------------------------
    @property
    def n_bricks(self) -> int:
        return self.grid.nvox // 512

    def touched_bricks(self, map_dev, channels: int = 0):
        """map_dev[b] |= 1 (uint8, one per brick, device memory, zeroed by the caller) for every brick that holds anything.
        With abi.CH_FREE in `channels` (and in the channel of pack_bricks / unpack_bricks) pending free-space counts stay pending
        and mark nothing: they travel on their own, as grid_tensor(abi.CH_FREE).  With abi.CH_SUB the unit is a 4x4x4 sub-brick:
        the map has 8 bytes per brick, the lists of pack_bricks / unpack_bricks hold brick * 8 + sub-brick, rows are 64 records."""
        abi.check(self._lib.tl3d_grid_touched_bricks(self._h, int(channels), abi.ptr(map_dev), int(map_dev.shape[0])))

    def pack_bricks(self, channel: int, bricks_dev, packed_dev):
        abi.check(self._lib.tl3d_grid_pack_bricks(self._h, int(channel), abi.ptr(bricks_dev), int(bricks_dev.shape[0]), abi.ptr(packed_dev)))

    def unpack_bricks(self, channel: int, bricks_dev, packed_dev):
        abi.check(self._lib.tl3d_grid_unpack_bricks(self._h, int(channel), abi.ptr(bricks_dev), int(bricks_dev.shape[0]), abi.ptr(packed_dev)))

    def max_weight(self) -> int:
        """Largest number of observations any TSDF voxel holds (int32 headroom: _cabi.TSDF_MAX_WEIGHT)."""
        w = C.c_int64(0)
        abi.check(self._lib.tl3d_grid_max_weight(self._h, C.byref(w)))
        return int(w.value)

    # ---- multi-GPU merge through the library's own RCCL binding (hosts without torch.distributed) -------------------
    @staticmethod
    def rccl_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        abi.check(abi.load().tl3d_rccl_unique_id(buf))
        return bytes(buf)

    def rccl_init(self, world: int, rank: int, unique_id: bytes):
        assert len(unique_id) == 128
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        abi.check(self._lib.tl3d_rccl_init(self._h, int(world), int(rank), buf))

    def allreduce_grid(self, channels: int = 0):
        abi.check(self._lib.tl3d_allreduce_grid(self._h, int(channels)))

    def grid_tensor(self, channel: int):
        """Zero-copy torch view of a grid channel (for torch.distributed all_reduce over RCCL)."""
        import torch
        p, nb = self.grid_ptr(channel)
        dt, item, typestr = (torch.int32, 4, "<i4") if channel in (abi.CH_TSDF, abi.CH_FREE) else (torch.int64, 8, "<i8")

        class _Iface:
            __cuda_array_interface__ = {"shape": (nb // item,), "typestr": typestr, "data": (p, False), "version": 2}
        t = torch.as_tensor(_Iface(), device=torch.device("cuda", self.device))
        assert t.data_ptr() == p and t.dtype == dt
        return t

    def extract(self, mode: int = abi.EXTRACT_CENTROID, min_count: int = 1, min_weight: int = 0,
                max_abs_tsdf: float = 1.0):
        n = C.c_int64(0)
        abi.check(self._lib.tl3d_extract(self._h, int(mode), int(min_count), int(min_weight), float(max_abs_tsdf),
                                         None, None, 0, C.byref(n)))
        xyz = np.empty((n.value, 3), np.float32)
        rgb = np.empty((n.value, 3), np.uint8)
        if n.value:
            abi.check(self._lib.tl3d_extract(self._h, int(mode), int(min_count), int(min_weight), float(max_abs_tsdf),
                                             abi.ptr(xyz), abi.ptr(rgb), n.value, C.byref(n)))
        return xyz, rgb

    def extract_mesh(self, min_weight: int = 0, keys: bool = False):
        """Marching-cubes mesh of the TSDF channel: (xyz f32 [V,3], rgb u8 [V,3], tris u32 [T,3]).  The
        vertices are the zero crossings of the usable voxel edges in record order; every triangle is wound so that
        (v1 - v0) x (v2 - v0) points to t > 0 (towards the cameras).  keys=True: a fourth array, int64 [V], 3 * (lattice index of the
        vertex's owner voxel) + axis, which names a vertex across the blocks of a lattice (tl3d.h: tl3d_extract_mesh_keyed)."""
        nv, nt = C.c_int64(0), C.c_int64(0)
        abi.check(self._lib.tl3d_extract_mesh(self._h, int(min_weight), None, None, 0, None, 0, C.byref(nv), C.byref(nt)))
        xyz = np.empty((nv.value, 3), np.float32)
        rgb = np.empty((nv.value, 3), np.uint8)
        tris = np.empty((nt.value, 3), np.uint32)
        key = np.empty(nv.value, np.int64)
        if nv.value:
            if keys:
                abi.check(self._lib.tl3d_extract_mesh_keyed(self._h, int(min_weight), abi.ptr(xyz), abi.ptr(rgb), nv.value, abi.ptr(tris),
                                                            nt.value, abi.ptr(key), C.byref(nv), C.byref(nt)))
            else:
                abi.check(self._lib.tl3d_extract_mesh(self._h, int(min_weight), abi.ptr(xyz), abi.ptr(rgb), nv.value, abi.ptr(tris),
                                                      nt.value, C.byref(nv), C.byref(nt)))
        return (xyz, rgb, tris, key) if keys else (xyz, rgb, tris)

    @staticmethod
    def _mesh_arrays(xyz, rgb, tris):
        """The caller's mesh as the library wants it, and a factory for outputs of the same kind: numpy arrays stay on the host,
        torch tensors (indices as int32 bit patterns, torch having little uint32 support) stay where they are."""
        if hasattr(tris, "data_ptr"):
            import torch
            dev = tris.device
            names = {np.float32: torch.float32, np.uint8: torch.uint8, np.uint32: torch.int32}
            tris = tris.reshape(-1, 3).contiguous()
            assert tris.dtype in (torch.int32, torch.uint32), "triangle indices must be 32-bit"
            if xyz is not None:
                xyz = xyz.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
            if rgb is not None:
                rgb = rgb.to(device=dev, dtype=torch.uint8).reshape(-1, 3).contiguous()

            def empty(shape, dtype):
                return torch.empty(shape, dtype=names[dtype], device=dev)
        else:
            tris = np.ascontiguousarray(tris, dtype=np.uint32).reshape(-1, 3)
            if xyz is not None:
                xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
            if rgb is not None:
                rgb = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1, 3)
            empty = np.empty
        return xyz, rgb, tris, empty

    def mesh_components(self, tris, n_vert: int):
        """Connected components of an indexed triangle list over n_vert vertices (needs no grid):
        (labels u32 [n_vert], tri_counts u32 [n_vert], n_components).  Two vertices are connected when one triangle names both;
        labels[v] is the smallest vertex index of v's component; tri_counts holds a component's triangle count at index = label
        and 0 elsewhere.  numpy in, numpy out; a torch device tensor of int32 indices in, int32 device tensors out."""
        _, _, tris, empty = self._mesh_arrays(None, None, tris)
        n_vert = int(n_vert)
        labels, counts = empty((max(n_vert, 0),), np.uint32), empty((max(n_vert, 0),), np.uint32)
        n = C.c_int64(0)
        abi.check(self._lib.tl3d_mesh_components(self._h, abi.ptr(tris) if len(tris) else None, len(tris), n_vert,
                                                 abi.ptr(labels) if n_vert > 0 else None, abi.ptr(counts) if n_vert > 0 else None, C.byref(n)))
        return labels, counts, n.value

    def filter_mesh(self, xyz, rgb, tris, min_triangles: int = 0, largest_only: bool = False):
        """Drop the small connected components of a mesh (needs no grid): keeps the components with at
        least min_triangles triangles (<= 0: all of them, the identity; from 1 upward the vertices no triangle uses go), or with
        largest_only the one with the most triangles (if it passes min_triangles too).  Survivors keep their order.  rgb may be
        None.  Returns (xyz, rgb, tris, info); info: components, components_kept, vertices_dropped, triangles_dropped and
        keep_vert (bool [V] over the input vertices)."""
        xyz, rgb, tris, empty = self._mesh_arrays(xyz, rgb, tris)
        nv, nt = len(xyz), len(tris)
        oxyz, otri = empty((nv, 3), np.float32), empty((nt, 3), np.uint32)
        orgb = empty((nv, 3), np.uint8) if rgb is not None else None
        keep = empty((nv,), np.uint8)
        kv, kt, nc, nk = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)

        def p(a):
            return abi.ptr(a) if a is not None and len(a) else None
        abi.check(self._lib.tl3d_mesh_filter_components(self._h, p(xyz), p(rgb), nv, p(tris), nt, int(min_triangles), 1 if largest_only else 0,
                                                        p(oxyz), p(orgb), nv, p(otri), nt, p(keep), C.byref(kv), C.byref(kt), C.byref(nc),
                                                        C.byref(nk)))
        info = dict(components=nc.value, components_kept=nk.value, vertices_dropped=nv - kv.value, triangles_dropped=nt - kt.value,
                    keep_vert=keep.astype(bool) if isinstance(keep, np.ndarray) else keep.bool())
        return oxyz[:kv.value], (orgb[:kv.value] if orgb is not None else None), otri[:kt.value], info

    def simplify_mesh(self, xyz, rgb, tris, cell: float, origin=None, placement: str = "mean", reg: float = 2.0 ** -10):
        """Vertex-clustering simplification of a mesh (needs no grid): the vertices of one cell of
        size `cell` (metres, on a lattice through `origin`, default (0, 0, 0)) become one vertex at their mean position and
        colour, numbered in the order of each cell's first vertex; triangles are mapped, the ones that collapse and the repeats
        of an earlier triangle go, the rest keep their order and winding.  Every cell becomes a vertex, also one no surviving
        triangle names (filter_mesh(min_triangles=1) drops those).  Same bytes in every run.  rgb may be None.  Returns
        (xyz, rgb, tris, info); info: clusters, vertices_in, triangles_in, degenerate_dropped, duplicates_dropped and
        vert_map (u32 [V]: the output vertex of every input vertex).
        placement="quadric" (tl3d_mesh_simplify_quadric) changes only the positions: a merged vertex goes where the planes of the
        triangles around its cell meet (Lindstrom's quadric clustering, regularised towards the mean by `reg` in (0, 1]), clamped
        to its cell.  That keeps creases and corners of piecewise planar meshes; on smooth surfaces it gains nothing.  info then
        also has quadric_placed (clusters with a quadric; the others sit at the mean), clamped and corners_skipped (triangle
        corners whose triangle spans more than 3 cells)."""
        if placement not in ("mean", "quadric"):
            raise ValueError(f"placement = {placement!r}: must be 'mean' or 'quadric'")
        xyz, rgb, tris, empty = self._mesh_arrays(xyz, rgb, tris)
        nv, nt = len(xyz), len(tris)
        oxyz, otri = empty((nv, 3), np.float32), empty((nt, 3), np.uint32)
        orgb = empty((nv, 3), np.uint8) if rgb is not None else None
        vmap = empty((nv,), np.uint32)
        o = None if origin is None else (C.c_double * 3)(*[float(v) for v in origin])
        kv, kt, ng, nd = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)

        def p(a):
            return abi.ptr(a) if a is not None and len(a) else None
        if placement == "quadric":
            nq, nc, ns = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            abi.check(self._lib.tl3d_mesh_simplify_quadric(self._h, p(xyz), p(rgb), nv, p(tris), nt, float(cell), o, float(reg), p(oxyz),
                                                           p(orgb), nv, p(otri), nt, p(vmap), C.byref(kv), C.byref(kt), C.byref(ng),
                                                           C.byref(nd), C.byref(nq), C.byref(nc), C.byref(ns)))
        else:
            abi.check(self._lib.tl3d_mesh_simplify_clusters(self._h, p(xyz), p(rgb), nv, p(tris), nt, float(cell), o, p(oxyz), p(orgb), nv,
                                                            p(otri), nt, p(vmap), C.byref(kv), C.byref(kt), C.byref(ng), C.byref(nd)))
        info = dict(clusters=kv.value, vertices_in=nv, triangles_in=nt, degenerate_dropped=ng.value, duplicates_dropped=nd.value,
                    vert_map=vmap)
        if placement == "quadric":
            info.update(quadric_placed=nq.value, clamped=nc.value, corners_skipped=ns.value)
        return oxyz[:kv.value], (orgb[:kv.value] if orgb is not None else None), otri[:kt.value], info

    def smooth_mesh(self, xyz, tris, iterations: int, lam: float = 0.5, mu: float = -0.53):
        """Taubin lambda|mu smoothing of a mesh's positions (needs no grid): `iterations` times a Laplacian
        step with `lam` and an inflating step with `mu` over the unique neighbours of every vertex, in exact integer sums, so the
        result does not depend on the numbering and is the same bytes in every run.  Triangles and colours are not touched.
        Returns (xyz, info); info: edges (unique undirected), valence (u32 [V]) and max_valence."""
        xyz, _, tris, empty = self._mesh_arrays(xyz, None, tris)
        nv, nt = len(xyz), len(tris)
        oxyz, val = empty((nv, 3), np.float32), empty((nv,), np.uint32)
        ne = C.c_int64(0)

        def p(a):
            return abi.ptr(a) if len(a) else None
        abi.check(self._lib.tl3d_mesh_smooth_taubin(self._h, p(xyz), nv, p(tris), nt, int(iterations), float(lam), float(mu), p(oxyz),
                                                    p(val), C.byref(ne)))
        return oxyz, dict(edges=ne.value, valence=val, max_valence=int(val.max()) if nv else 0)

    def mesh_normals(self, xyz, tris):
        """Area-weighted unit vertex normals of a mesh (needs no grid): f32 [V,3], the normalised exact
        integer sum of the face vectors of the triangles that name each vertex, pointing where the extraction's winding points;
        (0, 0, 0) for a vertex without one."""
        xyz, _, tris, empty = self._mesh_arrays(xyz, None, tris)
        nv, nt = len(xyz), len(tris)
        out = empty((nv, 3), np.float32)
        nz = C.c_int64(0)
        abi.check(self._lib.tl3d_mesh_vertex_normals(self._h, abi.ptr(xyz) if nv else None, nv, abi.ptr(tris) if nt else None, nt,
                                                     abi.ptr(out) if nv else None, C.byref(nz)))
        return out

    def weld_meshes(self, parts, lattice_dims):
        """One mesh from the keyed meshes of the blocks of a lattice, welded on the device (needs no grid):
        what lattice.weld_meshes computes on the host, byte for byte.  parts: [(xyz, rgb, tris, keys, core_lo, core_hi)] with the
        core in LATTICE voxels; every vertex whose owner voxel lies in its part's core is kept, in part order, and every triangle
        corner becomes the output index of the kept vertex with the corner's key.  rgb may be None, in every part or in none.  All
        parts numpy arrays (numpy out), or all torch device tensors (indices int32, keys int64; device tensors out).  Raises
        abi.Tl3dError when a vertex is owned by two cores or a triangle names a vertex no core owns.
        Returns (xyz, rgb, tris, keys)."""
        parts = list(parts)
        kinds = {hasattr(p[2], "data_ptr") for p in parts}
        if len(kinds) > 1:
            raise TypeError("weld_meshes: the parts must be all numpy arrays or all torch tensors")
        on_device = kinds == {True}
        rgbs = {p[1] is None for p in parts}
        if len(rgbs) > 1:
            raise ValueError("weld_meshes: rgb is given in every part or in none")
        has_rgb = rgbs != {True}                         # (no part at all: an empty colour array, as the host weld returns)
        arr = (abi.MeshPart * max(1, len(parts)))()
        hold = []
        for m, (xyz, rgb, tris, keys, lo, hi) in zip(arr, parts):
            xyz, rgb, tris, _ = self._mesh_arrays(xyz, rgb, tris)
            if on_device:
                import torch
                keys = keys.to(device=tris.device, dtype=torch.int64).reshape(-1).contiguous()
            else:
                keys = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
            if len(keys) != len(xyz) or (rgb is not None and len(rgb) != len(xyz)):
                raise ValueError(f"weld_meshes: a part has {len(xyz)} vertices, {len(keys)} keys"
                                 + ("" if rgb is None else f" and {len(rgb)} colours"))
            hold.append((xyz, rgb, tris, keys))
            m.n_vert, m.n_tri = len(xyz), len(tris)
            m.xyz_hd = abi.ptr(xyz).value if len(xyz) else None
            m.rgb_hd = abi.ptr(rgb).value if rgb is not None and len(rgb) else None
            m.key_hd = abi.ptr(keys).value if len(keys) else None
            m.tri_hd = abi.ptr(tris).value if len(tris) else None
            for a in range(3):
                m.core_lo[a], m.core_hi[a] = int(lo[a]), int(hi[a])
        nv, nt = sum(len(h[0]) for h in hold), sum(len(h[2]) for h in hold)
        if on_device:
            import torch
            dev = hold[0][2].device
            oxyz, otri = torch.empty((nv, 3), dtype=torch.float32, device=dev), torch.empty((nt, 3), dtype=torch.int32, device=dev)
            orgb = torch.empty((nv, 3), dtype=torch.uint8, device=dev) if has_rgb else None
            okey = torch.empty((nv,), dtype=torch.int64, device=dev)
        else:
            oxyz, otri = np.empty((nv, 3), np.float32), np.empty((nt, 3), np.uint32)
            orgb = np.empty((nv, 3), np.uint8) if has_rgb else None
            okey = np.empty((nv,), np.int64)
        dims = (C.c_int64 * 3)(*[int(d) for d in lattice_dims])

        def p(a):
            return abi.ptr(a) if a is not None and len(a) else None
        kv, kt, tw, un = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        abi.check(self._lib.tl3d_mesh_weld_keyed(self._h, arr, len(parts), dims, p(oxyz), p(orgb), p(okey), nv, p(otri), nt,
                                                 C.byref(kv), C.byref(kt), C.byref(tw), C.byref(un)))
        return oxyz[:kv.value], (orgb[:kv.value] if orgb is not None else None), otri[:kt.value], okey[:kv.value]

    def raycast(self, pose, min_weight: int = 0, z_near=None, z_far=None, slot=None, out=None):
        """Ray-cast the TSDF channel from the camera at pose = (R, t) (world->camera, as integrate):
        (depth f32 [H,W] with 0 = no hit, normals f32 [H,W,3] in the camera frame, bgr u8 [H,W,3]).  z_near / z_far default to
        the context's depth range.  slot: also write the view into that frame slot (an f32 frame with colour for
        build_normals, icp and fusion).  out: (depth, normals, bgr) host arrays or device tensors to fill (entries may be None)
        instead of new arrays; they are returned."""
        r, t = abi.d9(pose[0]), abi.d3(pose[1])
        if out is None:
            out = (np.empty((self.height, self.width), np.float32), np.empty((self.height, self.width, 3), np.float32),
                   np.empty((self.height, self.width, 3), np.uint8))
        for a, shape in zip(out, ((self.height, self.width), (self.height, self.width, 3), (self.height, self.width, 3))):
            assert a is None or tuple(a.shape) == shape, f"output {tuple(a.shape)} != {shape}"
        abi.check(self._lib.tl3d_raycast(self._h, abi.ptr(r), abi.ptr(t), int(min_weight),
                                         float(z_near) if z_near is not None else 0.0, float(z_far) if z_far is not None else 0.0,
                                         -1 if slot is None else int(slot), abi.ptr(out[0]), abi.ptr(out[1]), abi.ptr(out[2])))
        return tuple(out)

    def statistical_outlier(self, xyz, nb_neighbors=20, std_ratio=2.0, cell_size=None):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        keep = np.zeros(len(xyz), np.uint8)
        kept = C.c_int64(0)
        cell = float(cell_size if cell_size is not None else (self.grid.voxel_size * 2 if self.grid else 0.01))
        abi.check(self._lib.tl3d_statistical_outlier(self._h, abi.ptr(xyz), len(xyz), int(nb_neighbors), float(std_ratio),
                                                     cell, abi.ptr(keep), C.byref(kept)))
        return keep.astype(bool)

    def knn_mean_distance(self, xyz, nb_neighbors=20, cell_size=None):
        """float64 [n]: per point the mean distance to its nb_neighbors nearest neighbours, itself included (k clamped to n) --
        what statistical_outlier thresholds.  cell_size sets the search grid only; the result does not depend on it."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        mean = np.zeros(len(xyz), np.float64)
        cell = float(cell_size if cell_size is not None else (self.grid.voxel_size * 2 if self.grid else 0.01))
        abi.check(self._lib.tl3d_knn_mean_distance(self._h, abi.ptr(xyz), len(xyz), int(nb_neighbors), cell, abi.ptr(mean)))
        return mean

    def estimate_normals(self, xyz, nb_neighbors=30, max_radius=0.0, viewpoints=None, cell_size=None, curvature=False):
        """normals float32 [n,3], or (normals, curvature float32 [n]) with curvature=True: per point the unit eigenvector of the
        smallest eigenvalue of the covariance of its nb_neighbors nearest neighbours (itself included, k clamped to n, an exact tie
        to the smaller index; max_radius > 0 drops neighbours beyond it), and the surface variation l0 / (l0 + l1 + l2) (DESIGN.md
        section 4.5).  viewpoints [m,3]: every normal is turned towards the viewpoint nearest its point; without them the sign is
        arbitrary but fixed.  Points with fewer than 3 neighbours left, or whose neighbours all coincide, get (0,0,0) and 0;
        last_normals_degenerate counts them.  cell_size sets the search grid only; the result does not depend on it.
        numpy in, numpy out; a torch device tensor in, device tensors out."""
        xyz = self._points(xyz)
        n = len(xyz)
        if hasattr(xyz, "data_ptr"):
            import torch
            normals = torch.empty((n, 3), dtype=torch.float32, device=xyz.device)
            curv = torch.empty((n,), dtype=torch.float32, device=xyz.device) if curvature else None
        else:
            normals = np.empty((n, 3), np.float32)
            curv = np.empty((n,), np.float32) if curvature else None
        vp = None
        if viewpoints is not None:
            vp = np.ascontiguousarray(viewpoints, dtype=np.float64).reshape(-1, 3)
        cell = float(cell_size if cell_size is not None else (self.grid.voxel_size * 2 if self.grid else 0.01))
        deg = C.c_int64(0)
        self.last_normals_degenerate = 0
        if n:
            abi.check(self._lib.tl3d_estimate_normals(self._h, abi.ptr(xyz), n, int(nb_neighbors), float(max_radius), cell,
                                                      abi.ptr(vp) if vp is not None and len(vp) else None, len(vp) if vp is not None else 0,
                                                      abi.ptr(normals), abi.ptr(curv) if curvature else None, C.byref(deg)))
        self.last_normals_degenerate = int(deg.value)
        return (normals, curv) if curvature else normals

    def segment_planes(self, xyz, normals, curvature=None, radius=None, max_angle_deg=10.0, max_offset=None, max_curvature=0.0,
                       min_points=200, max_rms=0.0, signed_normals=True, cell_size=None):
        """(plane_id int32 [n], planes, counts): the planar regions of a cloud with normals.  Points with a
        usable normal (and, with a curvature array and max_curvature > 0, curvature <= max_curvature) are linked when they lie
        within radius, their normals within max_angle_deg (of parallel or anti-parallel with signed_normals=False) and each within
        max_offset of the other's tangent plane; a connected region of at least min_points points whose fitted plane has
        rms <= max_rms (max_rms <= 0: any) is a plane.  plane_id is the number of a point's plane or -1; planes is a numpy record
        array (normal, d, centroid, rms, count, seed) in ascending seed; counts = dict(eligible, regions, candidates, planes).
        radius / max_offset default to 2.5 / 1 voxel of the attached grid (0.025 / 0.01 m without one).  cell_size sets the search
        grid only (default: radius); the result does not depend on it.  numpy in, numpy plane_id out; torch device tensors in, a
        device plane_id out."""
        xyz, normals = self._points(xyz), self._points(normals)
        n = len(xyz)
        assert len(normals) == n, f"{len(normals)} normals for {n} points"
        voxel = self.grid.voxel_size if self.grid else 0.01
        radius = float(radius) if radius is not None else 2.5 * voxel
        max_offset = float(max_offset) if max_offset is not None else voxel
        if hasattr(xyz, "data_ptr"):
            import torch
            plane_id = torch.empty((n,), dtype=torch.int32, device=xyz.device)
            if curvature is not None:
                curvature = curvature.to(dtype=torch.float32).reshape(-1).contiguous()
        else:
            plane_id = np.empty((n,), np.int32)
            if curvature is not None:
                curvature = np.ascontiguousarray(curvature, dtype=np.float32).reshape(-1)
        assert curvature is None or len(curvature) == n, f"{len(curvature)} curvatures for {n} points"
        prm = abi.PlaneParams(radius=radius, min_cos=math.cos(math.radians(float(max_angle_deg))), max_offset=max_offset,
                              max_curvature=float(max_curvature), max_rms=float(max_rms), min_points=int(min_points),
                              signed_normals=1 if signed_normals else 0, reserved=0)
        cell = float(cell_size) if cell_size is not None else radius
        cnt = (C.c_int64 * 4)()
        cap = n // max(int(min_points), 1)                      # every candidate has min_points points of its own
        planes = np.zeros((cap,), abi.PLANE_DTYPE)
        abi.check(self._lib.tl3d_segment_planes(self._h, abi.ptr(xyz), abi.ptr(normals), abi.ptr(curvature), n, C.byref(prm), cell,
                                                abi.ptr(plane_id), abi.ptr(planes) if cap else None, cap, cnt))
        counts = dict(eligible=int(cnt[0]), regions=int(cnt[1]), candidates=int(cnt[2]), planes=int(cnt[3]))
        return plane_id, planes[:counts["planes"]].copy(), counts

    # ---- distances between sets (none of it needs a grid) -----------
    @staticmethod
    def _points(a):
        """A point list as the library wants it: numpy -> float32 [n,3] on the host, a torch tensor stays where it is."""
        if hasattr(a, "data_ptr"):
            import torch
            return a.to(dtype=torch.float32).reshape(-1, 3).contiguous()
        return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)

    @staticmethod
    def _nearest_outputs(query):
        if hasattr(query, "data_ptr"):
            import torch
            return (torch.empty(len(query), dtype=torch.float64, device=query.device),
                    torch.empty(len(query), dtype=torch.int32, device=query.device))
        return np.empty(len(query), np.float64), np.empty(len(query), np.int32)

    def nearest_points(self, query, target, max_dist=None, cell_size=None):
        """(dist float64 [n], index int32 [n]): for every query point the exact fp64 distance to its nearest target point and that
        point's index (the smallest index on an exact tie).  max_dist: a query with nothing within it gets +inf / -1 (so does every
        query of an empty target).  cell_size sets the search grid only (default: from the target's box and count); the result does
        not depend on it.  numpy in, numpy out; torch device tensors in, device tensors out."""
        query, target = self._points(query), self._points(target)
        dist, index = self._nearest_outputs(query)

        def p(a):
            return abi.ptr(a) if len(a) else None
        abi.check(self._lib.tl3d_nearest_points(self._h, p(query), len(query), p(target), len(target),
                                                float(cell_size) if cell_size is not None else 0.0,
                                                float(max_dist) if max_dist is not None else 0.0, p(dist), p(index)))
        return dist, index

    def nearest_triangles(self, query, xyz, tris, max_dist=None, cell_size=None):
        """(dist float64 [n], tri int32 [n]): for every query point the exact fp64 distance to the nearest point of the closed
        triangles of the mesh (xyz, tris) and the triangle it lies on (the smallest index on an exact tie); degenerate triangles
        measure as the segments or points they are.  max_dist, cell_size (default: the mean triangle box) and array kinds as
        nearest_points."""
        query = self._points(query)
        xyz, _, tris, _ = self._mesh_arrays(xyz, None, tris)
        dist, index = self._nearest_outputs(query)

        def p(a):
            return abi.ptr(a) if len(a) else None
        abi.check(self._lib.tl3d_nearest_triangles(self._h, p(query), len(query), p(xyz), len(xyz), p(tris), len(tris),
                                                   float(cell_size) if cell_size is not None else 0.0,
                                                   float(max_dist) if max_dist is not None else 0.0, p(dist), p(index)))
        return dist, index

    def distance_summary(self, dist, thresholds=()):
        """Summary of a float64 distance array (numpy or device tensor), reduced in a fixed shape on the GPU (the same bytes in every
        run): n, within (the finite entries), sum, sum_sq and max over those, mean and rms (nan without a finite entry), and below:
        per threshold (at most 8) the number of entries <= it."""
        if hasattr(dist, "data_ptr"):
            import torch
            dist = dist.to(dtype=torch.float64).reshape(-1).contiguous()
        else:
            dist = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
        thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        out = abi.DistanceStats()
        abi.check(self._lib.tl3d_distance_summary(self._h, abi.ptr(dist) if len(dist) else None, len(dist),
                                                  abi.ptr(thr) if len(thr) else None, len(thr), C.byref(out)))
        m = out.n_finite
        return dict(n=out.n, within=m, sum=out.sum, sum_sq=out.sum_sq, max=out.max,
                    mean=out.sum / m if m else float("nan"), rms=(out.sum_sq / m) ** 0.5 if m else float("nan"),
                    below=[int(out.below[j]) for j in range(len(thr))])

    def set_nearest_query_order(self, cell_order: bool):
        """nearest_points / nearest_triangles run their queries bucketed by cell (default) or, off, in input order: same bytes."""
        abi.check(self._lib.tl3d_set_nearest_query_order(self._h, 1 if cell_order else 0))

    # ---- registration of two point clouds (needs no grid) -------------
    #: register_clouds' default levels: the frame ICP's gate schedule, every 4th source point, then all
    CLOUD_LEVELS = (dict(iters=10, stride=4, max_dist=0.20), dict(iters=15, stride=1, max_dist=0.05))

    def _cloud_arrays(self, source, target, target_normals):
        source, target = self._points(source), self._points(target)
        if target_normals is not None:
            target_normals = self._points(target_normals)
            assert len(target_normals) == len(target), f"{len(target_normals)} normals for {len(target)} target points"
        return source, target, target_normals

    def cloud_evaluate(self, source, target, target_normals=None, T=None, scale=1.0, stride=1, max_dist=0.05, with_scale=False,
                       cell_size=None, indices=False):
        """One pass of the cloud registration at the pose (T, scale), no update (tl3d_cloud_evaluate): every `stride`-th source point
        p goes to q = scale * R p + t, meets its nearest target point y (the smaller index on a tie; kept within max_dist, None or
        <= 0: unlimited) and gives the point-to-plane row of y's normal, or without normals the three point-to-point rows.  A dict:
        A (7 x 7, sum J J^T with J = [q x n, n, n . w]; row and column 6 are zero without with_scale), b, e, n_corr, n_src,
        n_no_normal (correspondences dropped for a (0, 0, 0) normal), fitness, rmse; with indices=True also index (int32 per source
        point, -1: gated or not sampled; a device tensor for device input)."""
        source, target, target_normals = self._cloud_arrays(source, target, target_normals)
        T0 = np.ascontiguousarray(np.eye(4) if T is None else np.asarray(T, np.float64).reshape(4, 4))
        index = self._nearest_outputs(source)[1] if indices else None

        def p(a):
            return abi.ptr(a) if a is not None and len(a) else None
        res = abi.CloudEval()
        abi.check(self._lib.tl3d_cloud_evaluate(self._h, p(source), len(source), p(target), len(target),
                                                p(target_normals) if len(target) else None, abi.ptr(T0), float(scale), int(stride),
                                                float(max_dist) if max_dist is not None else 0.0,
                                                float(cell_size) if cell_size is not None else 0.0, 1 if with_scale else 0,
                                                C.byref(res), p(index)))
        A = np.zeros((7, 7))
        A[np.triu_indices(7)] = np.frombuffer(res, np.float64, 28)
        A = A + np.triu(A, 1).T
        out = dict(A=A, b=np.array(res.b[:]), e=res.e, n_corr=res.n_corr, n_src=res.n_src, n_no_normal=res.n_no_normal,
                   fitness=res.n_corr / res.n_src if res.n_src else 0.0, rmse=(res.e / res.n_corr) ** 0.5 if res.n_corr else 0.0,
                   raw=bytes(res))
        if indices:
            out["index"] = index
        return out

    def register_clouds(self, source, target, target_normals=None, T_init=None, scale_init=1.0, levels=None, estimate_scale=False,
                        cell_size=None):
        """Register one unorganised cloud onto another (tl3d_cloud_register): ICP over the target's cell index, point-to-plane with
        target_normals (unoriented ones are fine) and point-to-point without, through `levels` coarse to fine (dicts with icp()'s
        keywords; stride counts source points; default CLOUD_LEVELS), all on the device.  estimate_scale makes the scale a 7th
        unknown in every level that does not say otherwise -- it needs a closed or bounded scene: open geometry observes the scale
        weakly.  The dict icp() returns: T maps source to target (rigid part), scale is sigma: x_target = scale * R x + t.  A local
        method: the clouds must start within a gate of each other (T_init)."""
        source, target, target_normals = self._cloud_arrays(source, target, target_normals)
        T0 = np.ascontiguousarray(np.eye(4) if T_init is None else np.asarray(T_init, np.float64).reshape(4, 4))
        levels = [dict(lv) for lv in (self.CLOUD_LEVELS if levels is None else levels)]
        for lv in levels:
            lv.setdefault("stride", 1)
            lv.setdefault("estimate_scale", bool(estimate_scale))
        lv = _icp_levels(levels)

        def p(a):
            return abi.ptr(a) if a is not None and len(a) else None
        res = abi.IcpResult()
        abi.check(self._lib.tl3d_cloud_register(self._h, p(source), len(source), p(target), len(target),
                                                p(target_normals) if len(target) else None, abi.ptr(T0), float(scale_init), lv, len(levels),
                                                float(cell_size) if cell_size is not None else 0.0, C.byref(res)))
        return _icp_result_dicts(res)[0]

    # ---- global registration: a start for register_clouds from anywhere (needs no grid) ----
    @staticmethod
    def _like(a, shape, dtype):
        """An uninitialised output beside a: a device tensor for a device tensor, else a numpy array (dtype: a numpy type)."""
        if hasattr(a, "data_ptr"):
            import torch
            return torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=a.device)
        return np.empty(shape, dtype)

    def voxel_subsample(self, xyz, voxel):
        """int32 [kept], ascending: of every occupied voxel of the lattice through (0, 0, 0) (cell = floor(x / voxel)) the index of
        the member with the smallest index (tl3d_cloud_voxel_subsample).  A subset: xyz[index], normals[index], ... follow by
        indexing.  numpy in, numpy out; a device tensor in, a device tensor out."""
        xyz = self._points(xyz)
        n = len(xyz)
        index = self._like(xyz, (n,), np.int32)
        kept = C.c_int64(0)
        abi.check(self._lib.tl3d_cloud_voxel_subsample(self._h, abi.ptr(xyz) if n else None, n, float(voxel), abi.ptr(index),
                                                       C.byref(kept)))
        return index[:kept.value]

    def compute_fpfh(self, xyz, normals, nb_neighbors=48, max_radius=0.0, cell_size=None, spfh=False):
        """FPFH descriptors float32 [n,33] (tl3d_cloud_fpfh), or (fpfh, spfh int32 [n,34]: the 33 pair counts and their number) with
        spfh=True.  The neighbourhood is estimate_normals' list for the same nb_neighbors (4..64) and max_radius, less the point itself,
        duplicates and members with a (0,0,0) normal.  The normals are taken as given and their SIGN MATTERS: orient them by a rule
        that moves with the cloud (metrics.global_align_clouds uses the cloud's centroid as the viewpoint).  cell_size sets the
        search grid only; the result does not depend on it.  numpy in, numpy out; device tensors in, device tensors out."""
        xyz, normals = self._points(xyz), self._points(normals)
        n = len(xyz)
        assert len(normals) == n, f"{len(normals)} normals for {n} points"
        fpfh = self._like(xyz, (n, 33), np.float32)
        counts = self._like(xyz, (n, 34), np.int32) if spfh else None
        cell = float(cell_size) if cell_size is not None else (float(max_radius) / 2 if max_radius and max_radius > 0 else
                                                                (self.grid.voxel_size * 2 if self.grid else 0.01))
        if n:
            abi.check(self._lib.tl3d_cloud_fpfh(self._h, abi.ptr(xyz), abi.ptr(normals), n, int(nb_neighbors), float(max_radius), cell,
                                                abi.ptr(fpfh), abi.ptr(counts)))
        return (fpfh, counts) if spfh else fpfh

    def match_features(self, feat_a, feat_b, dist2=False):
        """int32 [n_a]: for every row of feat_a the row of feat_b with the smallest squared distance (fp64 sum over the columns in
        order; an exact tie goes to the smaller index; -1 for an empty feat_b), or (index, dist2 float64 [n_a]) with dist2=True
        (tl3d_feature_match).  Brute force: refused when n_a * n_b > 2^34 -- subsample first.  At most 64 columns."""
        def rows(a):
            if hasattr(a, "data_ptr"):
                import torch
                return a.to(dtype=torch.float32).contiguous()
            return np.ascontiguousarray(a, dtype=np.float32)
        feat_a, feat_b = rows(feat_a), rows(feat_b)
        assert feat_a.ndim == 2 and feat_b.ndim == 2 and feat_a.shape[1] == feat_b.shape[1], "features must be [n, dim] with one dim"
        na, nb, dim = feat_a.shape[0], feat_b.shape[0], feat_a.shape[1]
        index = self._like(feat_a, (na,), np.int32)
        d2 = self._like(feat_a, (na,), np.float64) if dist2 else None
        abi.check(self._lib.tl3d_feature_match(self._h, abi.ptr(feat_a) if na else None, na, abi.ptr(feat_b) if nb else None, nb, int(dim),
                                               abi.ptr(index) if na else None, abi.ptr(d2) if dist2 and na else None))
        return (index, d2) if dist2 else index

    def ransac_register(self, source, target, corr, hypotheses=100_000, max_dist=0.05, edge_ratio=0.9, seed=0, counts=False):
        """RANSAC over correspondences corr int32 [m,2] = (source index, target index) (tl3d_cloud_ransac): `hypotheses` samples of
        three correspondences drawn by a counter-based generator from `seed`, rejected unless the three edge lengths agree within
        edge_ratio, posed by the triad construction and scored by the correspondences within max_dist.  A dict: T (4 x 4, source
        to target; the identity when nothing passed), status (1: a winner; 2: nothing passed), best_h, inliers, n_passed (hypotheses
        scored), m; with counts=True also counts (int32 per hypothesis, -1: rejected).  The same bytes in every run."""
        source, target = self._points(source), self._points(target)
        if hasattr(corr, "data_ptr"):
            import torch
            corr = corr.to(dtype=torch.int32).reshape(-1, 2).contiguous()
        else:
            corr = np.ascontiguousarray(corr, dtype=np.int32).reshape(-1, 2)
        m = len(corr)
        prm = abi.RansacParams(n_hypotheses=int(hypotheses), max_dist=float(max_dist), edge_ratio=float(edge_ratio),
                               seed=int(seed) & (2 ** 64 - 1), reserved=0)
        res = abi.RansacResult()
        cnt = self._like(corr, (int(hypotheses),), np.int32) if counts else None

        def p(a):
            return abi.ptr(a) if a is not None and len(a) else None
        abi.check(self._lib.tl3d_cloud_ransac(self._h, p(source), len(source), p(target), len(target), p(corr), m, C.byref(prm),
                                              C.byref(res), p(cnt)))
        out = dict(T=np.array(res.T[:], np.float64).reshape(4, 4), status=res.status, best_h=res.best_h, inliers=res.inliers,
                   n_passed=res.n_passed, m=res.m)
        if counts:
            out["counts"] = cnt
        return out

    # ---- measurement -----------------------------------------------------------------------
    def set_profile(self, count_records=False, time_kernels=False):
        abi.check(self._lib.tl3d_set_profile(self._h, int(count_records), int(time_kernels)))

    def set_tsdf_pairing(self, on: bool):
        """integrate() may update two consecutive overlapping frames per launch (default); off: one frame per launch."""
        abi.check(self._lib.tl3d_set_tsdf_pairing(self._h, 1 if on else 0))

    def stats(self) -> dict:
        s = abi.Stats()
        abi.check(self._lib.tl3d_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in abi.Stats._fields_}

    def reset_stats(self):
        abi.check(self._lib.tl3d_reset_stats(self._h))

    def event_record(self, which: int):
        abi.check(self._lib.tl3d_event_record(self._h, int(which)))

    def event_elapsed_ms(self) -> float:
        ms = C.c_float(0)
        abi.check(self._lib.tl3d_event_elapsed_ms(self._h, C.byref(ms)))
        return ms.value
