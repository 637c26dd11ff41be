"""Crafted grids, cameras and frames that put the two readers of the TSDF cell (csrc/tsdf_cell.h) -- the ray caster (kernels_raycast.hip,
DESIGN.md section 4.3) and the point-to-SDF tracker (kernels_track.hip, section 12) -- on their decision edges, and counters that
prove the edges are reached.  Not a test.

The geometry is DYADIC, as in icp_edges_common: voxel 2^-5, trunc = 4 voxels, origins multiples of the voxel; fx = fy = 32 with integer
cx, cy (the centre column and row have xf == 0 / yf == 0, every other ray moves a whole number of voxels per metre); R = I or a signed
axis permutation; camera centres on multiples of half a voxel.  Corner values are -1, 0 or +1 (sum = -32767 w, 0, 32767 w): exact in
f32, and a layer sequence +1, 0, -1 is a field of slope exactly one per voxel.

EXACT MARCHES.  Unobserved space steps by exactly one voxel; where 0 < F <= 0.15625 the step is exactly half a voxel (0.8 trunc F <
voxel / 2).  A step from a larger F is 0.8f * trunc * F, which f32 and fp64 round differently -- so an exact case never takes one: its
rays cross unobserved layers and meet the surface's shell at the fraction 7/8 of a cell (+1, 0): F = 1/8, half a voxel on F = -3/8, and
z* = z + 2^-8 lands on the zero layer; or at 15/32 of a cell (+1, -1): F = 1/16, then -15/16, and z* lies half-way between the layers.
z_near = 1 + 7/256 (or 1 + 15/1024) with the camera 1 m in front of the face puts the samples on those fractions.  Every f32
operation of such a case is exact, so the fp64 model rounded to f32 must give the restatement's (and the device's) very bits.

Families (cases()): range, box, steps, zeros, weights, colour, shapes for the ray caster; track for the tracker; generic: tilted poses,
compared with the fp64 model away from decisions only.  Every case names the edges it is there for (Case.edges): counters(case) must
report each of them at least once.

counters() does not go through raycast_reference or track_reference: it adds up the events of cell_edges_reference's own fp64 march
(one ray or sample at a time, decisions written from the rules).  On an exact case those are the f32 decisions too (the CPU test proves
the outputs equal bit for bit, sample counts included).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field, replace
from typing import Optional, Tuple

import numpy as np

import cell_edges_reference as cer

F32 = np.float32
VOXEL = 2.0 ** -5
TRUNC = 4 * VOXEL
FX = FY = 32.0
ORIGIN = (-0.25, -0.25, 1.0)
ZN78 = 1.0 + 7.0 / 256.0            # with the camera 1 m before a face: samples at the fraction 7/8 of their cells
ZN1532 = 1.0 + 15.0 / 1024.0        # ... at 15/32

I3 = np.eye(3)
LOOK_X = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])        # camera z = world x
LOOK_Y = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])        # camera z = world y
TURN_X = np.diag([1.0, -1.0, -1.0])                                            # looking along -z
TURN_Y = np.diag([-1.0, 1.0, -1.0])
# a half turn about z whose zeros carry the sign a product (-1) * 0 leaves: (R^T (0, yf, 1))_x = (-1 * 0 + -0 * yf) + -0 = -0.0 for yf >= 0
NEG_ZERO = np.array([[-1.0, -0.0, 0.0], [-0.0, -1.0, 0.0], [-0.0, -0.0, 1.0]])


def camera(width, height, cx=None, cy=None):
    return dict(width=width, height=height, fx=FX, fy=FY, cx=float(width // 2 if cx is None else cx), cy=float(height // 2 if cy is None else cy))


def pose_at(R, cg, origin=ORIGIN):
    """world -> camera (R, t) of the camera whose centre has the grid coordinates cg (voxel centres are the integers)"""
    C = np.array([origin[a] + (cg[a] + 0.5) * VOXEL for a in range(3)])
    return np.array(R, np.float64), -(np.array(R, np.float64) @ C)


def records(sums, weights):
    """record-ordered int32 {sum, weight} from [nx][ny][nz] volumes"""
    dims = sums.shape
    ii, jj, kk = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    out = np.zeros((sums.size, 2), np.int32)
    idx = cer.rec_index(ii.ravel(), jj.ravel(), kk.ravel(), dims)
    out[idx, 0] = sums.ravel()
    out[idx, 1] = weights.ravel()
    out.setflags(write=False)
    return out


def volumes(dims, layers, axis=2, w=1):
    """(t, w) volumes: layers {index along `axis`: value in (-1, 0, 1)} observed with weight w, the rest unobserved"""
    t = np.zeros(dims, np.int64)
    wt = np.zeros(dims, np.int64)
    sl = [slice(None)] * 3
    for k, val in layers.items():
        sl[axis] = k
        t[tuple(sl)] = val
        wt[tuple(sl)] = w
    return t, wt


def slab(first, n, dims_z):
    """layers first: +1, first + 1: 0, then -1 up to n layers in all"""
    return {first + i: (1, 0)[i] if i < 2 else -1 for i in range(n) if first + i < dims_z}


@dataclass(frozen=True)
class Case:
    name: str
    family: str
    kind: str                                  # "ray" or "track"
    dims: Tuple[int, int, int]
    rec: np.ndarray = field(repr=False, compare=False)
    cam: dict = field(compare=False)
    pose: tuple = field(repr=False, compare=False)
    edges: Tuple[str, ...] = ()
    exact: bool = True
    origin: Tuple[float, float, float] = ORIGIN
    min_depth: float = 0.5                     # the context's limits
    max_depth: float = 4.0
    min_weight: int = 0
    z_near: Optional[float] = None             # as handed to raycast(): None, 0 and negative mean the context's limit
    z_far: Optional[float] = None
    cen: Optional[np.ndarray] = field(default=None, repr=False, compare=False)
    named: Tuple[Tuple[int, int], ...] = ()    # the (u, v) rays a generic case is there for: never set aside
    model: bool = True                         # False: too large for the one-at-a-time fp64 model (restatement and device only)
    # tracker
    depth: Optional[np.ndarray] = field(default=None, repr=False, compare=False)
    stride: int = 1
    max_dist: float = TRUNC / 2
    scale: float = 1.0

    @property
    def z_range(self):
        """what tl3d_raycast resolves: a limit that is not positive means the context's own"""
        zn = self.z_near if self.z_near is not None and self.z_near > 0 else self.min_depth
        zf = self.z_far if self.z_far is not None and self.z_far > 0 else self.max_depth
        return float(F32(zn)), float(F32(zf))


# ---- ray-cast scenes -----------------------------------------------------------------------------------------------------------------
D16 = (16, 16, 24)
CAM95 = camera(9, 5)
FRONT = (7.5, 7.5, -32.0)                    # 1 m in front of the z = 0 face of a 16 x 16 x n grid


@functools.lru_cache(maxsize=None)
def scene_a(w=1, last=23):
    """unobserved up to layer 9, then +1, 0, -1 ...: the shell of an exact march; the zero layer is 11 (depth 1 + 11/32 from FRONT)"""
    t, wt = volumes(D16, {k: v for k, v in slab(10, 14, 24).items() if k <= last}, w=w)
    return records(t * 32767 * wt, wt)


def _ray(name, family, rec, edges, dims=D16, cam=CAM95, R=I3, cg=FRONT, **kw):
    return Case(name, family, "ray", dims, rec, cam, pose_at(R, cg), tuple(edges), **kw)


def _range_cases():
    a = scene_a()
    z_end = ZN78 + 10.0 / 32.0 + 1.0 / 64.0      # the sample that ends every ray of scene_a from FRONT: x_z = 11 + 3/8, F = -3/8
    below, above = float(np.nextafter(F32(z_end), F32(0))), float(np.nextafter(F32(z_end), F32(9)))
    lim = dict(min_depth=ZN78, max_depth=4.0)
    return [
        _ray("range_default", "range", a, ["end_hit", "half_voxel_steps"], **lim),
        _ray("range_zero", "range", a, ["end_hit"], z_near=0.0, z_far=0.0, **lim),
        _ray("range_negative", "range", a, ["end_hit"], z_near=-1.0, z_far=-2.0, **lim),
        _ray("range_explicit_past_ctx_max", "range", a, ["end_hit"], min_depth=0.5, max_depth=1.25, z_near=ZN78, z_far=2.0),
        _ray("range_ctx_max_before_surface", "range", a, ["ended_by_z_far"], min_depth=0.5, max_depth=1.25, z_near=ZN78),
        _ray("range_far_one_float_before", "range", a, ["ended_by_z_far"], z_near=ZN78, z_far=below),
        _ray("range_far_at_sample", "range", a, ["end_hit"], z_near=ZN78, z_far=z_end),
        _ray("range_far_one_float_past", "range", a, ["end_hit"], z_near=ZN78, z_far=above),
        _ray("range_near_inside", "range", a, ["first_sample_negative"], z_near=1.0 + 12.5 / 32.0),
        _ray("range_near_behind", "range", scene_a(last=16), ["ended_by_box_exit"], z_near=1.0 + 18.5 / 32.0),
        _ray("range_near_gt_far", "range", a, ["z_near_gt_z_far", "end_range_empty"], z_near=3.0, z_far=2.0),
    ]


def _last_layers(axis, flip=False):
    """a surface between the LAST two layers of `axis`: (+1, -1) on layers 14, 15 of a 16^3 grid, nothing else observed"""
    t, wt = volumes((16, 16, 16), {14: -1 if flip else 1, 15: 1 if flip else -1}, axis=axis)
    return records(t * 32767 * wt, wt)


def _box_cases():
    a = scene_a()
    zero_first = records(*(lambda t, w: (t * 32767 * w, w))(*volumes(D16, {10: 0, 11: 0, 12: -1, 13: -1})))
    full = records(*(lambda t, w: (t * 32767 * w, w))(*volumes(D16, {k: int(np.clip(12 - k, -1, 1)) for k in range(24)}, w=2)))
    d16 = (16, 16, 16)
    out = [
        _ray("box_parallel_inside", "box", a, ["axis_parallel_inside", "axis_parallel_negative_zero", "end_hit"], R=NEG_ZERO, z_near=ZN78),
        _ray("box_parallel_outside", "box", a, ["axis_parallel_outside", "axis_parallel_negative_zero", "end_range_empty"], R=NEG_ZERO,
             cg=(-1.0, 7.5, -32.0), z_near=ZN78),
        _ray("box_parallel_outside_high", "box", a, ["axis_parallel_outside"], cg=(15.5, 7.5, -32.0), z_near=ZN78),
        _ray("box_parallel_on_closed_end", "box", a, ["axis_parallel_inside", "sample_on_open_end", "ended_by_box_exit"], cg=(15.0, 7.5, -32.0),
             z_near=ZN78),
        _ray("box_entry_on_face", "box", zero_first, ["first_sample_on_face", "F_eq_0_prev_undefined"]),
        _ray("box_entry_on_face_full_grid", "box", full, ["first_sample_on_face", "end_hit"], exact=False),
        _ray("box_last_layers_z", "box", _last_layers(2), ["end_hit"], dims=d16, z_near=ZN1532),
        _ray("box_last_layers_x", "box", _last_layers(0), ["end_hit"], dims=d16, R=LOOK_X, cg=(-32.0, 7.5, 7.5), z_near=ZN1532),
        _ray("box_last_layers_y", "box", _last_layers(1), ["end_hit"], dims=d16, R=LOOK_Y, cg=(7.5, -32.0, 7.5), z_near=ZN1532),
        # from the far side: the first sample lies ON the open end x_z = 15 (the slab admits it, the cell refuses it), the next at 14
        _ray("box_far_face_entry", "box", _last_layers(2, flip=True), ["first_sample_on_face", "sample_on_open_end", "negative_after_undefined"], dims=d16,
             R=TURN_X, cg=(7.5, 7.5, 47.0)),
        _ray("box_far_face_surface", "box", _last_layers(2, flip=True), ["end_hit"], dims=d16, R=TURN_X, cg=(7.5, 7.5, 47.0), z_near=ZN1532),
        _ray("box_camera_inside", "box", a, ["end_hit"], cg=(7.5, 7.5, 5.0), min_depth=7.0 / 256.0),
        _ray("box_looking_away", "box", a, ["end_range_empty"], R=TURN_Y, z_near=ZN78),
    ]
    return out


LONG = (8, 8, 4104)
SKIM = (8, 8, 2056)
SKIM_SUM = 4096                                # t = 4096 / 32767: 0.8 trunc t < voxel / 2, so every step is the half voxel itself


@functools.lru_cache(maxsize=None)
def _long_scene(first):
    t, wt = volumes(LONG, slab(first, 7, LONG[2]))
    return records(t * 32767 * wt, wt)


@functools.lru_cache(maxsize=None)
def _skim_scene():
    s = np.full(SKIM, SKIM_SUM, np.int64)
    s[:, :, 2049:] = -32767
    return records(s, np.ones(SKIM, np.int64))


@functools.lru_cache(maxsize=None)
def _plane_scene(k):
    """13 observed layers around a zero crossing at k + 1/2: +1 up to layer k, -1 behind"""
    dims = (8, 8, 4400)
    t, wt = volumes(dims, {k + i: 1 if i <= 0 else -1 for i in range(-6, 7)})
    return records(t * 32767 * wt, wt)


def _steps_cases():
    kw = dict(cg=(3.5, 3.5, -32.0), z_near=ZN78, z_far=200.0)
    plane = dict(dims=(8, 8, 4400), cg=(3.5, 3.5, -32.0), z_far=200.0, exact=False, named=((4, 2),))
    return [
        # a long march that meets the plane's +1 side at a whole voxel and takes full 0.8 trunc F steps (inexact: device against
        # restatement only): the centre ray hits at 94.76584 after 2998 samples; 1200 layers further on it stops at 4096 with no hit
        _ray("steps_plane_at_3000", "steps", _plane_scene(3000), ["end_hit"], **plane),
        _ray("steps_plane_at_4200", "steps", _plane_scene(4200), ["end_cap"], **plane),
        # sample s of the centre ray lies at x_z = s + 7/8: the shell's first layer at 4094 makes sample 4095 -- the last one allowed -- the hit
        _ray("steps_cap_reached_by_the_hit", "steps", _long_scene(4094), ["end_hit"], dims=LONG, named=((4, 2),), **kw),
        # ... at 4095 sample 4095 is the positive one and the ray stops with its budget spent
        _ray("steps_cap_before_the_hit", "steps", _long_scene(4095), ["end_cap"], dims=LONG, named=((4, 2),), **kw),
        # 4096 half-voxel steps from x_z = 1/4 over F = 0.125...: sample 4096 would lie at 2048.25, in the cell (+, -1) that ends a ray
        _ray("steps_skim", "steps", _skim_scene(), ["end_cap", "half_voxel_steps"], dims=SKIM, named=((4, 2),), cg=(3.5, 3.5, -32.0),
             z_near=1.0 + 1.0 / 128.0, z_far=200.0),
    ]


def _zeros_cases():
    def rec_of(layers, dims=D16, edit=None):
        t, wt = volumes(dims, layers)
        if edit:
            edit(t, wt)
        return records(t * 32767 * wt, wt)

    def split(t, wt):                          # layer 12: +1 below y = 7.5, -1 above: F == 0 on the plane y = 7.5 with dF/dy != 0
        t[:, :8, 12] = 1
        t[:, 8:, 12] = -1

    def column(t, wt):                         # one voxel wide, unobserved, BEHIND the zero layer: z* of ray u = 7 lies in its cell
        wt[11, :, 22] = 0
        t[11, :, 22] = 0
    d32 = (16, 16, 32)
    return [
        _ray("zeros_slab", "zeros", rec_of({10: 1, 11: 0, 12: 0, 13: -1, 14: -1}), ["F_eq_0_prev_defined", "hit_normal_zero_gradient"], z_near=ZN78),
        _ray("zeros_on_a_slope", "zeros", rec_of({10: 1, 11: 0, 12: 0, 13: -1, 14: -1}, edit=split), ["F_eq_0_prev_defined", "end_hit"],
             cam=camera(9, 1), z_near=ZN78),
        _ray("zeros_first_defined", "zeros", rec_of({10: 0, 11: 0, 12: -1, 13: -1}), ["F_eq_0_prev_undefined", "end_behind"], z_near=ZN78),
        _ray("zeros_first_negative", "zeros", scene_a(), ["first_sample_negative", "end_behind"], z_near=1.0 + 11.25 / 32.0),
        _ray("zeros_unobserved_column", "zeros", rec_of(slab(20, 10, 32), dims=d32, edit=column), ["hit_normal_cell_undefined", "end_hit"], dims=d32,
             cg=(7.0, 7.5, -32.0), z_near=ZN78, named=((7, 2),)),
    ]


def _weights_cases():
    out = []
    for mw in (0, 1, 2, 3):
        eff = max(1, mw)
        t, wt = volumes(D16, slab(10, 14, 24))
        ii, jj = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
        low = ((ii // 2 + jj // 2) % 2 == 1)[:, :, None] & (wt > 0)
        wt = np.where(low, eff - 1, eff) * (wt > 0)
        out.append(_ray(f"weights_checker_mw{mw}", "weights", records(t * 32767 * wt, wt), ["w_eq_mw", "w_eq_mw_minus_1", "end_hit", "ended_by_box_exit"],
                        min_weight=mw, z_near=ZN78))
    out.append(_ray("weights_512", "weights", scene_a(w=512), ["end_hit"], min_weight=512, z_near=ZN78))
    t, wt = volumes(D16, slab(10, 14, 24))
    s = t * 32767 * wt
    s[wt == 0] = np.where(np.indices(D16).sum(axis=0) % 2 == 0, 12345, -777)[wt == 0]
    out.append(_ray("weights_zero_with_a_sum", "weights", records(s, wt), ["w0_sum_nonzero", "end_hit"], z_near=ZN78))
    rng = np.random.default_rng(5)
    kk = np.arange(24)[None, None, :]
    q = np.clip((12 - kk) * 9000 + rng.integers(-4000, 4001, size=D16), -32767, 32767)
    out.append(_ray("weights_60000", "weights", records(q * 60000, np.full(D16, 60000)), ["sum_not_f32", "end_hit"], exact=False, min_weight=60000))
    return out


def _centroids(dims):
    """[records][4] u64: count in the high half of word 1, sums of r | g << 32 in word 2, of b in word 3; every third voxel of a
    diagonal pattern has no points, the sums leave remainders"""
    ii, jj, kk = (g.ravel() for g in np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"))
    cnt = np.where((ii + jj) % 3 == 0, 0, 2 + (ii + 2 * jj + kk) % 5)
    r, g, b = ((cnt * (16 + (a * ii + jj) % 200) + (cnt > 0) * ((ii + a) % np.maximum(cnt, 1))).astype(np.uint64) for a in (1, 2, 3))
    cnt = cnt.astype(np.uint64)
    cen = np.zeros((ii.size, 4), np.uint64)
    idx = cer.rec_index(ii, jj, kk, dims)
    cen[idx, 1] = cnt << np.uint64(32)
    cen[idx, 2] = r | (g << np.uint64(32))
    cen[idx, 3] = b
    cen.setflags(write=False)
    return cen


def _colour_cases():
    d16 = (16, 16, 16)
    return [
        # the hit lies at x_z = 14.5: floor(x_z + 1/2) = 15, the grid's last voxel layer
        _ray("colour_last_half_voxel", "colour", _last_layers(2), ["colour_count_0", "colour_mean", "colour_division_rounds", "colour_last_voxel"], dims=d16,
             z_near=ZN1532, cen=_centroids(d16)),
        _ray("colour_zero_layer", "colour", scene_a(), ["colour_count_0", "colour_mean", "colour_division_rounds"], z_near=ZN78, cen=_centroids(D16)),
    ]


def _shapes_cases():
    return [_ray(f"shapes_{w}x{h}", "shapes", scene_a(), ["end_hit"], cam=camera(w, h), z_near=ZN78) for w, h in ((5, 3), (9, 5), (17, 33), (40, 24))]


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))


@functools.lru_cache(maxsize=None)
def _generic_scene():
    """every voxel seen twice, the surface between layers 12 and 13 bent by one layer over x, an unobserved block beside the view's centre"""
    ii, _, kk = np.meshgrid(*[np.arange(d) for d in D16], indexing="ij")
    t = np.clip(12 + (ii >= 8) - kk, -1, 1)
    wt = np.full(D16, 2, np.int64)
    wt[2:4, 10:13, 6:16] = 0
    return records(t * 32767 * wt, wt)


def _generic_cases():
    cam = camera(17, 13)
    out = []
    # z_near starts every ray INSIDE the box: a first sample on the entry face is a decision f32 and fp64 may take differently
    for i, (ang, cg, zn) in enumerate((((0.07, -0.11, 0.05), (7.3, 7.9, -20.2), 0.75), ((-0.13, 0.21, -0.3), (10.1, 6.2, -15.7), 0.625),
                                       ((0.31, 0.17, 1.1), (6.4, 4.1, -9.3), 0.4375))):
        out.append(_ray(f"generic_tilt_{i}", "generic", _generic_scene(), ["end_hit"], cam=cam, R=rot(*ang), cg=cg, exact=False, min_depth=0.125,
                        min_weight=2, z_near=zn))
    return out


# ---- tracker ---------------------------------------------------------------------------------------------------------------------------
TRACK_DIMS = (256, 136, 16)
TRACK_CG = (127.5, 67.5, 0.0)                # x_z = 32 d: one float of the depth is one float of the coordinate
TRACK_MIN, TRACK_MAX = 0.125, 0.4375         # x_z = 4 and 14
TILES_PER_WAVE, MEMBERS_CAP = 8, 256         # kernels_track.hip


def track_members(ws, hs):
    tiles = ((ws + 7) // 8) * ((hs + 7) // 8)
    return tiles, max(1, min(MEMBERS_CAP, (tiles + 4 * TILES_PER_WAVE - 1) // (4 * TILES_PER_WAVE)))


@functools.lru_cache(maxsize=None)
def track_scene():
    """F = 8 - x_z between layers 7 and 9, +1 before, -1 behind; two unobserved columns.  Their walls (x = 123, 126, 199, 201; y = 61, 70)
    are kept off the coordinates 127.5 +- 7.5 k and 127.5 +- 8.5 k (67.5 +- ... in y) on which the one-float neighbours of the gate depths
    fall for odd k: there x = cg + (xf d) * 32 needs more than 24 bits, and f32 and fp64 would put the sample on different sides"""
    t, wt = volumes(TRACK_DIMS, {k: int(np.clip(8 - k, -1, 1)) for k in range(16)})
    wt[124:126, 62:70, :] = 0
    wt[200, :, 8] = 0
    return records(t * 32767 * wt, wt)


def _below(x):
    return float(np.nextafter(F32(x), F32(0)))


def _above(x):
    return float(np.nextafter(F32(x), F32(9)))


# depths (x_z / 32) that sit on and beside the gate |F| == 1/2 (x_z = 7.5 and 8.5), inside it, on the zero, outside it, and the odd ones
_PLAIN = (7.5 / 32, 7.75 / 32, 8.5 / 32, 8.25 / 32, _below(7.5 / 32), _above(8.5 / 32), 0.25, 7.0 / 32, 9.5 / 32, 7.625 / 32, 8.125 / 32)
_ODD = (0.0, np.nan, np.inf, -np.inf, -1.0, TRACK_MIN, _above(TRACK_MIN), _below(TRACK_MIN), TRACK_MAX, _below(TRACK_MAX), _above(TRACK_MAX), 5.0 / 32)


@functools.lru_cache(maxsize=None)
def patchwork(width, height, divide=1.0, wide=False):
    """every pixel one of the plain depths in turn; every seventh pixel one of the odd ones.  divide: stored / divide, read with scale.
    wide: for the gates beyond 1/2, which would ACCEPT the one-float neighbours of the gate depths (24-bit summands: the sums would no
    longer be exact) -- |F| = 3/4 in their place, the wide gate itself"""
    n = np.arange(height)[:, None] * 131 + np.arange(width)[None, :] * 7
    plain = [{_below(7.5 / 32): 7.25 / 32, _above(8.5 / 32): 8.75 / 32}.get(q, q) if wide else q for q in _PLAIN]
    d = np.asarray(plain, F32)[(n // 3) % len(plain)]
    odd = (np.arange(height)[:, None] * 3 + np.arange(width)[None, :]) % 7 == 3
    d = np.where(odd, np.asarray(_ODD, F32)[(n // 5) % len(_ODD)], d).astype(F32)
    d = (d / F32(divide)).astype(F32)
    d.setflags(write=False)
    return d


def _track(name, w, h, stride, edges, depth=None, **kw):
    cam = camera(w, h)
    return Case(name, "track", "track", TRACK_DIMS, track_scene(), cam, pose_at(I3, TRACK_CG), tuple(edges), min_depth=TRACK_MIN, max_depth=TRACK_MAX,
                min_weight=1, depth=patchwork(w, h) if depth is None else depth, stride=stride, **kw)


def _track_cases():
    gate = ["F_eq_gate", "gated", "d_nan", "d_inf", "d_zero", "d_negative", "d_eq_min", "d_eq_max", "d_next_above_min", "d_next_below_max", "cell_undefined"]
    out = []
    out.append(_track("track_88x24_s1", 88, 24, 1, []))                      # 33 tiles: the first shape with a second member
    for (w, h) in ((9, 5), (64, 32), (65, 33)):
        for s in (1, 2, 3, 4):
            out.append(_track(f"track_{w}x{h}_s{s}", w, h, s, gate if w > 9 and s == 1 else []))      # (9 x 5: two tiles for four waves)
    for s in (1, 2, 3, 4):
        out.append(_track(f"track_1024x520_s{s}", 1024, 520, s, [], model=False))
    out.append(_track("track_scale_2", 65, 33, 1, ["scale_crosses_min", "scale_crosses_max", "F_eq_gate"], depth=patchwork(65, 33, 2.0), scale=2.0))
    out.append(_track("track_gate_cap", 65, 33, 1, ["gate_capped", "gated"], depth=patchwork(65, 33, wide=True), max_dist=2 * TRUNC))
    out.append(_track("track_gate_wide", 65, 33, 2, ["gated", "F_eq_gate"], depth=patchwork(65, 33, wide=True), max_dist=0.75 * TRUNC))
    # millimetres read with a scale that is no power of two: d * scale rounds, and crosses the limits somewhere
    mm = np.clip(np.rint(np.nan_to_num(patchwork(65, 33).astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0) * 1000.0), 0, 65535).astype(np.uint16)
    mm[4::5, 3::4] = 125
    mm[2::5, 1::4] = 437
    out.append(_track("track_u16_scaled", 65, 33, 1, ["gated"], depth=mm, scale=1.001, exact=False))
    out.append(_track("track_tilted", 65, 33, 1, ["gated"], exact=False))
    return out


def _finish(case):
    if case.name == "track_tilted":
        R, t = pose_at(rot(0.02, -0.03, 0.4), (126.9, 67.2, 0.3))
        return replace(case, pose=(R, t))
    return case


@functools.lru_cache(maxsize=None)
def cases():
    out = (_range_cases() + _box_cases() + _steps_cases() + _zeros_cases() + _weights_cases() + _colour_cases() + _shapes_cases() + _generic_cases() +
           [_finish(c) for c in _track_cases()])
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


FAMILIES = ("range", "box", "steps", "zeros", "weights", "colour", "shapes", "generic", "track")


def family(name):
    return [c for c in cases() if c.family == name]


def by_name(name):
    return next(c for c in cases() if c.name == name)


def frame_f32(case):
    """the f32 depth image the tracker reads from the slot: a 16-bit frame is millimetres / 1000 (one IEEE division)"""
    d = np.asarray(case.depth)
    return (d.astype(F32) / F32(1000.0)).astype(F32) if d.dtype == np.uint16 else d.astype(F32)


# ---- the model's answers and the counters ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model(name):
    """the fp64 model's outputs for a case, computed once: raycast -> (depth, normals, bgr, samples, margin, events); track -> dict"""
    c = by_name(name)
    assert c.model
    if c.kind == "ray":
        zn, zf = c.z_range
        return cer.raycast(c.rec, c.dims, c.origin, VOXEL, TRUNC, c.cam, c.pose, c.min_weight, zn, zf, c.cen)
    return cer.track_sums(c.rec, c.dims, c.origin, VOXEL, TRUNC, c.cam, frame_f32(c), c.pose, c.stride, c.max_dist, c.min_weight, c.min_depth,
                          c.max_depth, c.scale)


def counters(case):
    """how many rays (or samples) of the case took each named edge; record reads (w_eq_mw, ...) count corner reads"""
    m = model(case.name)
    if case.kind == "track":
        return dict(m["events"], n_src=m["n_src"], n_corr=m["n_corr"])
    total = {"n_rays": len(m[5]), "n_hits": int((m[0] > 0).sum())}
    for ev in m[5]:
        for k, v in ev.items():
            total[k] = total.get(k, 0) + v
    return total
