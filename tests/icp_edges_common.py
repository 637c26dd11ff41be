"""Crafted frame pairs that put the ICP association (csrc/icp_sample.h: icp_accumulate_core) and the maps it reads (normals_kernel,
smooth_depth_kernel) on their decision edges, and counters that prove the edges are hit.  Not a test.

The geometry is DYADIC, as in tsdf_edges_common: camera 40 x 24 (or another size around the same principal point), fx = fy = 32,
cx = 20, cy = 12, depth limits 0.5 / 4.0; planes at dyadic depths; poses R = I or a signed axis permutation, translations that are
multiples of 1/64.  Pixel rays (u - 20) / 32 are exact, a depth-1 plane gives pz = 1 whose reciprocal is exact, so every vertex,
projection and residual of such a pair is exact in f32 -- and the fp64 sums of the pass are exact too (Case.exact; the CPU test proves
it by adding the terms forwards, backwards and with math.fsum).

Families (cases()):
  validity   a source patchwork of odd pixels (0, NaN, inf, -1, the limits themselves and their f32 neighbours); source scales that
             carry d * sc across a limit (2 on 0.25 and 2.0; the non-dyadic 1.001 on 0.5 and on the float below 4).
  pz         tz = -1 on the depth-1 plane (pz == 0), tz = -5/4, a half turn about y (and one that looks back at the plane), a quarter
             turn about z, and the SUBNORMAL pz: rotation by 2^-127 about y, tz = -1, tx = 20/32 -- pixel (0, 12) has px = py = 0 and
             pz = 2^-127 * 20/32, whose reciprocal is finite only as the IEEE quotient (the kernels' division fallback); the references
             accept that one sample, so the fallback IS reachable through a rigid pose and the case is kept.
  ties       tx / ty odd multiples of 1/64: every uf / vf is n + 0.5.  A tie shows only where its two candidate pixels differ, so
             the target carries holes and depth steps beyond the jump: columns and rows of invalid normals beside valid ones.
             The window borders themselves (uf == -0.5, uf == W - 0.5) always land on the map's invalid 1-pixel frame: no output can
             tell which way they went; they are exercised, and only the totals constrain them.
  target     holes and their 4-neighbours, NaN, the border frame (radius r's wider one), neighbours at exactly depth_jump (1 and
             1 + 1/16 with jump 1/16) and one float beyond.
  gate       per pixel the largest source depth with dist2 <= md2 or the next float up, in a checkerboard, for max_dist 0.05,
             0.0625, 0.1 (md2 = f32(md) * f32(md): the contract of tl3d.h and the C oracle).
  walk       the same content tiled at the shapes and strides at which the sample walk, the phase-major rows and the software
             pipeline take their different paths (see WALK).
  smoothing  radius 0, 1, 2, 8 on tilted planes with holes and a wall (and, in the target family, on steps at exactly the jump): one
             of a symmetric pair invalid, out of the image or beyond the jump; a scaled source averaged in its own units.

counters() restates the per-sample rule in plain numpy on its own (its own single-rounding fma by round-to-odd, its own exits), not
through second_numpy.icp_sums; it takes the maps (the source depth the pass reads and the target's normal map) from whichever
reference the caller built them with.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Tuple

import numpy as np

from oracle import second_numpy as sn

F32 = np.float32
F64 = np.float64

FX = FY = 32.0
CX, CY = 20.0, 12.0
MIN_DEPTH, MAX_DEPTH = 0.5, 4.0
BASE_W, BASE_H = 40, 24

# members of a registration in the evaluation and the batched kernel (tl3d_internal.h: ICP_*_SAMPLES_PER_MEMBER, *_MEMBERS_CAP)
SAMPLES_PER_MEMBER = 8192
EVAL_MEMBERS_CAP, BATCH_MEMBERS_CAP = 256, 32


def _next(x, towards):
    return F32(np.nextafter(F32(x), F32(towards)))


def fma(a, b, c):
    """round_f32(a * b + c), one rounding: the exact product and its float64 sum with c ROUNDED TO ODD (53 >= 2 * 24 + 2 bits), then
    the cast -- a formulation of its own, not second_numpy's"""
    a, b, c = (np.asarray(x, F32).astype(F64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = np.asarray(p + c)
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0.0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
        return s.astype(F32)


# ---- images ----------------------------------------------------------------------------------------------------------------------
def _tiled(base, width, height):
    reps = ((height + BASE_H - 1) // BASE_H, (width + BASE_W - 1) // BASE_W)
    out = np.ascontiguousarray(np.tile(base, reps)[:height, :width])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tgt_flat(width=BASE_W, height=BASE_H):
    return _tiled(np.ones((BASE_H, BASE_W), F32), width, height)


@functools.lru_cache(maxsize=None)
def tgt_base(width=BASE_W, height=BASE_H):
    """plateaus at 1, 63/64 and 33/32, a band at 1.5, holes (one two pixels wide), NaN, inf, -1 and the limits themselves; the
    top-left 3 x 3 pixels are plain"""
    d = np.ones((BASE_H, BASE_W), F32)
    d[:, 8:14] = F32(63 / 64)
    d[14:18, 18:34] = F32(33 / 32)
    d[2:10, 22:26] = F32(1.5)
    for (u, v), val in (((5, 5), 0.0), ((30, 6), 0.0), ((16, 20), 0.0), ((17, 20), 0.0), ((28, 11), np.nan), ((35, 3), np.inf),
                        ((3, 18), -1.0), ((36, 20), MAX_DEPTH), ((12, 4), MIN_DEPTH)):
        d[v, u] = F32(val)
    return _tiled(d, width, height)


@functools.lru_cache(maxsize=None)
def tgt_jump(width=BASE_W, height=BASE_H):
    """1 beside 1 + 1/16 (a step of exactly the jump 1/16) and beside the float above it (one float beyond), in columns and rows"""
    d = np.ones((BASE_H, BASE_W), F32)
    hi, hi_next = F32(17 / 16), _next(17 / 16, 2)
    d[:, 6:10] = hi
    d[:, 16:20] = hi_next
    d[12:15, 24:37] = hi
    d[18:21, 24:37] = hi_next
    d[5, 30] = F32(0.0)
    return _tiled(d, width, height)


_ODD = (0.0, np.nan, np.inf, -1.0, MIN_DEPTH, _next(MIN_DEPTH, 1), MAX_DEPTH, _next(MAX_DEPTH, 0))


def _patch(width, height, plain, odd):
    n = (np.arange(height)[:, None] % BASE_H) * BASE_W + (np.arange(width)[None, :] % BASE_W)
    d = np.full((height, width), F32(plain), F32)
    pick = n % 5 == 3
    d[pick] = np.asarray(odd, F32)[(n[pick] // 5) % len(odd)]
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def src_patch(width=BASE_W, height=BASE_H):
    """the depth-1 plane; every fifth pixel is odd, in turn 0, NaN, inf, -1, 0.5, the float above, 4.0, the float below"""
    return _patch(width, height, 1.0, _ODD)


@functools.lru_cache(maxsize=None)
def src_patch_half(width=BASE_W, height=BASE_H):
    """read with scale 2: the plane at 0.5 (-> 1), odd pixels 0.25 (-> the lower limit) and 2.0 (-> the upper), their neighbours"""
    return _patch(width, height, 0.5, (0.0, np.nan, np.inf, -1.0, 0.25, _next(0.25, 1), 2.0, _next(2.0, 0)))


def _ramp(width, height):
    return (F32(1.0) + np.arange(width, dtype=F32)[None, :] / F32(256.0) + np.arange(height, dtype=F32)[:, None] / F32(512.0)).astype(F32)


@functools.lru_cache(maxsize=None)
def tgt_ramp(width=BASE_W, height=BASE_H):
    """a tilted plane with holes, a NaN and a wall: every window average is its own f32 sum"""
    d = _ramp(BASE_W, BASE_H)
    d[10:14, 27:29] = F32(2.0)
    for (u, v), val in (((5, 5), 0.0), ((6, 5), 0.0), ((30, 6), 0.0), ((28, 17), np.nan), ((15, 12), 0.0), ((0, 9), 0.0), ((39, 14), 0.0),
                        ((20, 0), 0.0), ((21, 23), 0.0)):
        d[v, u] = F32(val)
    return _tiled(d, width, height)


@functools.lru_cache(maxsize=None)
def src_ramp(width=BASE_W, height=BASE_H):
    d = _ramp(BASE_W, BASE_H) + F32(1 / 128)
    n = np.arange(BASE_H)[:, None] * BASE_W + np.arange(BASE_W)[None, :]
    pick = n % 7 == 4
    d[pick] = np.asarray(_ODD, F32)[(n[pick] // 7) % len(_ODD)]
    return _tiled(d, width, height)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def pose(t=(0.0, 0.0, 0.0), R=None):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = np.asarray(R, float)
    T[:3, 3] = t
    return T


HALF_TURN_Y = np.diag([-1.0, 1.0, -1.0])
QUARTER_TURN_Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
TINY = 2.0 ** -127
TINY_TURN_Y = np.array([[1.0, 0.0, TINY], [0.0, 1.0, 0.0], [-TINY, 0.0, 1.0]])       # cos = 1, sin = the angle, to every float


@dataclass(frozen=True)
class Case:
    """one source frame, one target frame and one pass"""
    name: str
    family: str
    src: np.ndarray = field(repr=False, compare=False)        # float32 [H, W], as uploaded
    tgt: np.ndarray = field(repr=False, compare=False)
    T: np.ndarray = field(repr=False, compare=False)          # 4 x 4, source camera -> target camera
    radius: int = 0                                           # normal smoothing of both maps
    jump: float = 1 / 16                                      # depth_jump of both maps
    scale: float = 1.0                                        # source scale
    stride: int = 1
    max_dist: float = 1 / 16
    exact: bool = False                                       # every term and every partial sum of the pass is exact in fp64

    @property
    def width(self):
        return self.src.shape[1]

    @property
    def height(self):
        return self.src.shape[0]

    @property
    def n_samples(self):
        return ((self.width + self.stride - 1) // self.stride) * ((self.height + self.stride - 1) // self.stride)


def geometry(case: Case) -> sn.Geometry:
    return sn.Geometry(case.width, case.height, FX, FY, CX, CY, MIN_DEPTH, MAX_DEPTH)


def c_oracle_for(case: Case):
    from oracle import c_oracle
    return c_oracle.Oracle(case.width, case.height, FX, FY, CX, CY, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)


@functools.lru_cache(maxsize=None)
def gate_frame(max_dist):
    """[H, W]: per pixel the largest depth d whose sample (at the identity pose, against the depth-1 plane) has dist2 <= md2, or the
    next float up -- in a checkerboard.  Also returns how many pixels have dist2 == md2 at the inner depth."""
    md = F32(max_dist)
    md2 = F32(md * md)
    x = ((np.arange(BASE_W, dtype=F32) - F32(CX)) / F32(FX))[None, :] * np.ones((BASE_H, 1), F32)
    y = ((np.arange(BASE_H, dtype=F32) - F32(CY)) / F32(FY))[:, None] * np.ones((1, BASE_W), F32)

    def dist2(d):
        dx, dy, dz = x * d - x, y * d - y, d - F32(1.0)
        return fma(dx, dx, fma(dy, dy, dz * dz))
    est = (1.0 + float(md) / np.sqrt(x.astype(F64) ** 2 + y.astype(F64) ** 2 + 1.0)).astype(F32)
    d = est.copy()
    for _ in range(64):
        d = np.nextafter(d, F32(0))
    inner = np.zeros_like(est)
    found = np.zeros(est.shape, bool)
    for _ in range(128):                                      # the last accepted float of a window of 128 around the estimate
        ok = dist2(d) <= md2
        inner = np.where(ok, d, inner)
        found |= ok
        d = np.nextafter(d, F32(8))
    assert found.all() and not (dist2(d) <= md2).any()
    outer = np.nextafter(inner, F32(8))
    assert not (dist2(outer) <= md2).any()
    uu, vv = np.meshgrid(np.arange(BASE_W), np.arange(BASE_H))
    frame = np.where((uu + vv) % 2 == 0, inner, outer).astype(F32)
    frame.setflags(write=False)
    return frame, int((dist2(inner) == md2).sum())


# shape -> (strides at radius 0, ((radius, stride), ...)): what each shape is there for
WALK = {
    (1, 1): ((1, 5), ()),                                     # a single pixel
    (3, 3): ((1, 2), ()),                                     # one valid normal
    (37, 1): ((1, 5), ()),                                    # no valid normal, n_src only
    (40, 24): ((1, 2, 3, 5), ((1, 1), (1, 2), (2, 3))),       # 960 samples: threads hold 3 or 4, a ragged trip
    (41, 25): ((1, 3), ((2, 1),)),                            # phase-major rows with W % 4 = 1; 1025 samples: one thread holds 5
    (42, 25): ((1, 2), ((2, 2),)),                            # W % 4 = 2
    (43, 25): ((1, 2, 3, 5), ((1, 1), (1, 3))),               # W % 4 = 3
    (300, 3): ((1, 5), ((1, 1),)),                            # Ws > 256: dvs == 0 with one member; a stride larger than H
    (131, 67): ((1, 2, 3, 5), ((1, 1), (1, 2))),              # 8777 samples: two members; stride 2: threads hold 8 or 9
    (700, 13): ((1, 2), ((1, 1),)),                           # two members and step = 512 < Ws
}


@functools.lru_cache(maxsize=None)
def cases() -> Tuple[Case, ...]:
    out = []
    tie_u = pose((1 / 64, 0.0, 0.0))

    def add(name, family, src, tgt, T=None, **kw):
        out.append(Case(name=name, family=family, src=src, tgt=tgt, T=pose() if T is None else T, **kw))
    # source validity
    add("valid_identity", "validity", src_patch(), tgt_flat(), exact=True)
    add("valid_scale2", "validity", src_patch_half(), tgt_flat(), scale=2.0, exact=True)
    add("valid_scale1001", "validity", src_patch(), tgt_flat(), scale=1.001)
    # pz <= 0, rotations
    add("pz_zero", "pz", src_patch(), tgt_flat(), pose((0.0, 0.0, -1.0)), exact=True)
    add("pz_negative", "pz", src_patch(), tgt_flat(), pose((0.0, 0.0, -1.25)), exact=True)
    add("half_turn_y", "pz", src_patch(), tgt_flat(), pose(R=HALF_TURN_Y), exact=True)
    add("half_turn_y_back", "pz", src_patch(), tgt_base(), pose((0.0, 0.0, 2.0), HALF_TURN_Y), jump=1 / 128, exact=True)
    add("quarter_turn_z_tie", "pz", src_patch(), tgt_base(), pose((0.0, 1 / 64, 0.0), QUARTER_TURN_Z), jump=1 / 128, exact=True)
    add("pz_subnormal", "pz", tgt_flat(), tgt_flat(), pose((20 / 32, 0.0, -1.0), TINY_TURN_Y), max_dist=2.0)
    # rounding ties
    for name, t in (("tie_u", (1 / 64, 0, 0)), ("tie_v", (0, 1 / 64, 0)), ("tie_uv", (1 / 64, 1 / 64, 0)), ("tie_u_neg", (-1 / 64, 0, 0)),
                    ("tie_uv_neg", (-1 / 64, -1 / 64, 0)), ("tie_uv_far", (3 / 64, -5 / 64, 0))):
        add(name, "ties", src_patch(), tgt_base(), pose(t), jump=1 / 128, exact=True)
    for r in (1, 2):
        add(f"tie_u_r{r}", "ties", src_patch(), tgt_base(), tie_u, radius=r, jump=1 / 128)
        add(f"tie_uv_r{r}", "ties", src_patch(), tgt_base(), pose((1 / 64, 1 / 64, 0)), radius=r, jump=1 / 128)
    # target validity
    add("target_base", "target", src_patch(), tgt_base(), jump=1 / 128, exact=True)
    add("target_base_seams_at_jump", "target", src_patch(), tgt_base(), jump=1 / 64)
    add("target_jump", "target", tgt_flat(), tgt_jump(), max_dist=1 / 8)
    add("target_jump_tie", "target", tgt_flat(), tgt_jump(), pose((1 / 64, 1 / 64, 0)), max_dist=1 / 8)
    for r in (1, 2, 8):
        add(f"target_base_r{r}", "target", src_patch(), tgt_base(), radius=r, jump=1 / 128)
        add(f"target_jump_r{r}", "target", tgt_flat(), tgt_jump(), radius=r, max_dist=1 / 8)
    # the gate
    for md in (0.05, 0.0625, 0.1):
        add(f"gate_{md}", "gate", gate_frame(md)[0], tgt_flat(), max_dist=md)
    # the sample walk
    for (w, h), (strides, smoothed) in WALK.items():
        for s in strides:
            add(f"walk_{w}x{h}_s{s}", "walk", src_patch(w, h), tgt_base(w, h), tie_u, stride=s, jump=1 / 128, exact=True)
        for r, s in smoothed:
            add(f"walk_{w}x{h}_s{s}_r{r}", "walk", src_patch(w, h), tgt_base(w, h), tie_u, stride=s, radius=r, jump=1 / 128)
    # smoothing
    for r in (0, 1, 2, 8):
        for s in (1, 2):
            add(f"smooth_r{r}_s{s}", "smoothing", src_ramp(), tgt_ramp(), tie_u, radius=r, stride=s)
    add("smooth_r2_43x25", "smoothing", src_ramp(43, 25), tgt_ramp(43, 25), tie_u, radius=2)
    add("smooth_r1_scale2", "smoothing", (src_ramp() * F32(0.5)).astype(F32), tgt_ramp(), tie_u, radius=1, scale=2.0)
    add("smooth_r2_scale1001", "smoothing", src_ramp(), tgt_ramp(), tie_u, radius=2, scale=1.001)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


FAMILIES = ("validity", "pz", "ties", "target", "gate", "walk", "smoothing")


def family(name):
    return [c for c in cases() if c.family == name]


# ---- the maps a pass reads, from either reference -----------------------------------------------------------------------------------
def maps_numpy(case: Case):
    """(source depth the pass reads, depth map the target's normals are taken from, target normal map) by second_numpy"""
    g = geometry(case)
    if case.radius == 0:
        return np.asarray(case.src, F32), np.asarray(case.tgt, F32), sn.normals(g, case.tgt, 1.0, case.jump)
    src = sn.smooth_depth(g, case.src, case.scale, case.jump, case.radius)
    tsd = sn.smooth_depth(g, case.tgt, 1.0, case.jump, case.radius)
    return src, tsd, sn.normals(g, tsd, 1.0, case.jump, step=case.radius)


def maps_c(case: Case):
    """the same three maps by the C oracle"""
    orc = c_oracle_for(case)
    if case.radius == 0:
        return np.asarray(case.src, F32), np.asarray(case.tgt, F32), orc.normals(case.tgt, 1.0, case.jump)
    src, _ = orc.normals_smooth(case.src, case.radius, case.scale, case.jump)
    tsd, nmap = orc.normals_smooth(case.tgt, case.radius, 1.0, case.jump)
    return src, tsd, nmap


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the per-sample rule, restated -------------------------------------------------------------------------------------------------
SRC_INVALID, PZ_NOT_POSITIVE, OUT_OF_WINDOW, TARGET_INVALID, GATED, ACCEPTED = range(6)
# why a pixel of the target's normal map is invalid
T_OK, T_BORDER, T_HOLE, T_NEIGHBOUR, T_JUMP, T_DEGENERATE = range(6)


def target_reasons(case: Case, tdepth, nmap):
    """per pixel: why the normal map holds nothing there (T_*), the largest |neighbour - centre| where all five are valid, and
    whether a T_JUMP pixel is ONE FLOAT beyond the jump: valid if every neighbour's depth were the next float towards the centre's"""
    H, W = tdepth.shape
    step = max(1, case.radius)
    d = np.asarray(tdepth, F32)
    with np.errstate(invalid="ignore"):
        valid = (d > F32(MIN_DEPTH)) & (d < F32(MAX_DEPTH))
    reason = np.full((H, W), T_BORDER, np.int64)
    worst = np.full((H, W), np.nan, F32)
    near = np.zeros((H, W), bool)
    for v in range(step, H - step):
        for u in range(step, W - step):
            nb = ((v, u - step), (v, u + step), (v - step, u), (v + step, u))
            if not valid[v, u]:
                reason[v, u] = T_HOLE
            elif not all(valid[p] for p in nb):
                reason[v, u] = T_NEIGHBOUR
            else:
                worst[v, u] = max(abs(F32(d[p] - d[v, u])) for p in nb)
                reason[v, u] = T_JUMP if not worst[v, u] <= F32(case.jump) else T_OK
                near[v, u] = reason[v, u] == T_JUMP and all(abs(F32(np.nextafter(d[p], d[v, u]) - d[v, u])) <= F32(case.jump) for p in nb)
    has = np.asarray(nmap)[..., 3] > 0
    reason[(reason == T_OK) & ~has] = T_DEGENERATE
    assert np.array_equal(reason == T_OK, has), case.name
    return reason, worst, near


def sample_rule(case: Case, src_map, nmap, d=None):
    """every sample of the stride grid through the rule, row-major; d: the scaled source depths to use instead of src_map * scale"""
    W, H = case.width, case.height
    us, vs = np.arange(0, W, case.stride), np.arange(0, H, case.stride)
    raw = np.asarray(src_map, F32)[np.ix_(vs, us)]
    T = np.asarray(case.T, F64)
    r, t = T[:3, :3].astype(F32), T[:3, 3].astype(F32)
    fx, fy, cx, cy = F32(FX), F32(FY), F32(CX), F32(CY)
    md2 = F32(F32(case.max_dist) * F32(case.max_dist))
    with np.errstate(all="ignore"):
        if d is None:
            d = raw * F32(case.scale)
        valid = (d > F32(MIN_DEPTH)) & (d < F32(MAX_DEPTH))
        p0 = ((us.astype(F32) - cx) / fx)[None, :] * d
        p1 = ((vs.astype(F32) - cy) / fy)[:, None] * d
        px, py, pz = (fma(r[a, 0], p0, fma(r[a, 1], p1, fma(r[a, 2], d, t[a]))) for a in range(3))
        front = pz > F32(0)
        inv = F32(1.0) / pz
        uf = fma(fx * px, inv, cx)
        vf = fma(fy * py, inv, cy)
        inwin = (uf >= F32(-0.5)) & (uf < F32(W) - F32(0.5)) & (vf >= F32(-0.5)) & (vf < F32(H) - F32(0.5))
        reach = valid & front & inwin
        ut = np.where(reach, np.minimum(np.floor(uf + F32(0.5)), W - 1), 0).astype(np.int64)
        vt = np.where(reach, np.minimum(np.floor(vf + F32(0.5)), H - 1), 0).astype(np.int64)
        nd = np.asarray(nmap, F32)[vt, ut]
        nx, ny, nz, dt = (nd[..., i] for i in range(4))
        tvalid = dt > F32(0)
        qx = ((ut.astype(F32) - cx) / fx) * dt
        qy = ((vt.astype(F32) - cy) / fy) * dt
        dx, dy, dz = px - qx, py - qy, pz - dt
        dist2 = fma(dx, dx, fma(dy, dy, dz * dz))
        gate = dist2 <= md2
        res = fma(dx, nx, fma(dy, ny, dz * nz))
        J = (fma(py, nz, -(pz * ny)), fma(pz, nx, -(px * nz)), fma(px, ny, -(py * nx)), nx, ny, nz)
    code = np.full(d.shape, ACCEPTED, np.int64)
    code[~gate] = GATED
    code[~tvalid] = TARGET_INVALID
    code[~inwin] = OUT_OF_WINDOW
    code[~front] = PZ_NOT_POSITIVE
    code[~valid] = SRC_INVALID
    return dict(raw=raw, d=d, valid=valid, px=px, py=py, pz=pz, front=front, uf=uf, vf=vf, inwin=inwin, reach=reach, ut=ut, vt=vt,
                tvalid=tvalid, dist2=dist2, md2=md2, code=code, res=res, J=J)


def terms(case: Case, src_map, nmap):
    """the accepted samples' J [6, n] and r [n] as float64, in the oracle's sample order"""
    m = sample_rule(case, src_map, nmap)
    ok = m["code"] == ACCEPTED
    return np.stack([j[ok].astype(F64) for j in m["J"]]), m["res"][ok].astype(F64)


COUNTER_NAMES = ("n_samples", "n_src", "n_corr",
                 "src_zero", "src_nan", "src_inf", "src_negative", "src_eq_min", "src_eq_max", "src_next_above_min", "src_next_below_max",
                 "src_scale_makes_valid", "src_scale_makes_invalid",
                 "pz_eq_0", "pz_lt_0", "pz_subnormal", "pz_subnormal_accepted",
                 "out_of_window", "uf_eq_left", "uf_eq_right", "vf_eq_top", "vf_eq_bottom",
                 "tie_u", "tie_v", "tie_uv", "tie_u_candidates_differ", "tie_v_candidates_differ",
                 "target_border", "target_hole", "target_neighbour", "target_jump", "target_degenerate", "target_at_jump", "target_one_float_past_jump",
                 "gate_eq", "gate_one_float_inside", "gate_one_float_outside", "gated", "accepted")


def counters(case: Case, src_map=None, tdepth=None, nmap=None) -> dict:
    """how many samples of the pass end at each exit of the rule / sit on each edge; the maps default to second_numpy's"""
    if nmap is None:
        src_map, tdepth, nmap = maps_numpy(case)
    W, H = case.width, case.height
    m = sample_rule(case, src_map, nmap)
    reason, worst, near = target_reasons(case, tdepth, nmap)
    code, d, raw, reach = m["code"], m["d"], m["raw"], m["reach"]
    has = np.asarray(nmap)[..., 3] > 0
    with np.errstate(all="ignore"):
        raw_valid = (raw > F32(MIN_DEPTH)) & (raw < F32(MAX_DEPTH))
        sees = m["valid"] & m["front"]
        tie_u = reach & (m["uf"] - np.floor(m["uf"]) == F32(0.5))
        tie_v = reach & (m["vf"] - np.floor(m["vf"]) == F32(0.5))
        ulo = np.where(tie_u, np.floor(m["uf"]), 0).astype(np.int64)
        vlo = np.where(tie_v, np.floor(m["vf"]), 0).astype(np.int64)
        u_both = tie_u & (ulo >= 0) & (ulo + 1 <= W - 1)
        v_both = tie_v & (vlo >= 0) & (vlo + 1 <= H - 1)
        u_diff = u_both & (has[m["vt"], np.clip(ulo, 0, W - 1)] != has[m["vt"], np.clip(ulo + 1, 0, W - 1)])
        v_diff = v_both & (has[np.clip(vlo, 0, H - 1), m["ut"]] != has[np.clip(vlo + 1, 0, H - 1), m["ut"]])
        hit_reason = reason[m["vt"], m["ut"]]
        hit_worst = worst[m["vt"], m["ut"]]
        at_target = code == TARGET_INVALID
        up = sample_rule(case, src_map, nmap, d=np.nextafter(d, F32(np.inf)))["code"]
        down = sample_rule(case, src_map, nmap, d=np.nextafter(d, F32(0)))["code"]
        out = dict(
            n_samples=code.size, n_src=m["valid"].sum(), n_corr=(code == ACCEPTED).sum(),
            src_zero=(d == 0).sum(), src_nan=np.isnan(d).sum(), src_inf=np.isinf(d).sum(), src_negative=(d < 0).sum(),
            src_eq_min=(d == F32(MIN_DEPTH)).sum(), src_eq_max=(d == F32(MAX_DEPTH)).sum(),
            src_next_above_min=(d == _next(MIN_DEPTH, 1)).sum(), src_next_below_max=(d == _next(MAX_DEPTH, 0)).sum(),
            src_scale_makes_valid=(m["valid"] & ~raw_valid).sum(), src_scale_makes_invalid=(~m["valid"] & raw_valid).sum(),
            pz_eq_0=(m["valid"] & (m["pz"] == 0)).sum(), pz_lt_0=(m["valid"] & (m["pz"] < 0)).sum(),
            pz_subnormal=(sees & (m["pz"] < F32(2.0 ** -126))).sum(),
            pz_subnormal_accepted=((code == ACCEPTED) & (m["pz"] < F32(2.0 ** -126))).sum(),
            out_of_window=(code == OUT_OF_WINDOW).sum(),
            uf_eq_left=(sees & (m["uf"] == F32(-0.5))).sum(), uf_eq_right=(sees & (m["uf"] == F32(W) - F32(0.5))).sum(),
            vf_eq_top=(sees & (m["vf"] == F32(-0.5))).sum(), vf_eq_bottom=(sees & (m["vf"] == F32(H) - F32(0.5))).sum(),
            tie_u=tie_u.sum(), tie_v=tie_v.sum(), tie_uv=(tie_u & tie_v).sum(),
            tie_u_candidates_differ=u_diff.sum(), tie_v_candidates_differ=v_diff.sum(),
            target_border=(at_target & (hit_reason == T_BORDER)).sum(), target_hole=(at_target & (hit_reason == T_HOLE)).sum(),
            target_neighbour=(at_target & (hit_reason == T_NEIGHBOUR)).sum(), target_jump=(at_target & (hit_reason == T_JUMP)).sum(),
            target_degenerate=(at_target & (hit_reason == T_DEGENERATE)).sum(),
            target_at_jump=(reach & m["tvalid"] & (hit_worst == F32(case.jump))).sum(),
            target_one_float_past_jump=(at_target & near[m["vt"], m["ut"]]).sum(),
            gate_eq=(reach & m["tvalid"] & (m["dist2"] == m["md2"])).sum(),
            gate_one_float_inside=((code == ACCEPTED) & (up == GATED)).sum(),
            gate_one_float_outside=((code == GATED) & (down == ACCEPTED)).sum(),
            gated=(code == GATED).sum(), accepted=(code == ACCEPTED).sum())
    assert not (at_target & (hit_reason == T_OK)).any(), case.name
    return {k: int(out[k]) for k in COUNTER_NAMES}


# ---- the sample walk ---------------------------------------------------------------------------------------------------------------
def members(n_samples, cap=EVAL_MEMBERS_CAP):
    return int(min(cap, max(1, (n_samples + SAMPLES_PER_MEMBER - 1) // SAMPLES_PER_MEMBER)))


def samples_per_thread(n_samples, n_members):
    """how many samples each of the n_members * 256 threads holds: thread i takes samples i, i + n_members * 256, ..."""
    i = np.arange(n_members * 256)
    return np.maximum(0, (n_samples - i + n_members * 256 - 1) // (n_members * 256))
