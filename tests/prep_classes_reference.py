"""A plain numpy model of the TSDF prep chain (kernels_tsdf_prep.hip): the tile pyramid, the brick class, the sub-brick class, and the
per-voxel truth the classes must be conservative against.  TEST REFERENCE ONLY.

It restates the rule from the kernels' comments and code in f32 scalars, one brick at a time.  It is NOT kept bit-equal with the
GPU: the kernels project with v_rcp_f32 (1 ulp) and the compiler may fuse their multiply-adds, so the model's pixel bounds can
differ from the GPU's in the last bits.  perturbations() moves the bounds by far more than that (a quarter pixel, half a percent
of a voxel); a case whose class survives all of them is ROBUST and only such cases are compared with the GPU.

`fault` switches ONE deliberate mistake on (FAULTS); tests/test_prep_classes_reference_cpu.py shows that each is caught by a named
case of tests/prep_classes_common.py -- that is what proves the crafted inputs discriminate.
"""
from __future__ import annotations

import functools
import itertools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from oracle import second_numpy as sn

F32 = np.float32
INF = F32(np.inf)
TILE0_SHIFT = 3
MAX_LEVELS = 14
SKIP, MIXED, FREE = 0, 1, 2

FAULTS = ("drop_last_col", "drop_last_row", "allvalid_lost_above_0", "allvalid_lost_above_1", "allvalid_lost_above_2",
          "swap_min_max_in_skip", "window_3x3", "walk_first_row_only", "level_one_too_fine", "partial_tile_invalid", "ignore_inside")
PYRAMID_FAULTS = FAULTS[:5] + ("partial_tile_invalid",)


@dataclass(frozen=True)
class Setup:
    """camera, depth limits and grid"""
    W: int
    H: int
    fx: float
    fy: float
    cx: float
    cy: float
    mind: float
    maxd: float
    dims: Tuple[int, int, int]
    origin: Tuple[float, float, float]
    voxel: float
    trunc: float

    def geometry(self) -> sn.Geometry:
        return sn.Geometry(self.W, self.H, self.fx, self.fy, self.cx, self.cy, self.mind, self.maxd, self.dims, self.origin, self.voxel,
                           self.trunc)

    @property
    def nb(self):
        return tuple(d // 8 for d in self.dims)


# ---- tile pyramid ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def level_shapes(W, H):
    """((ntx, nty), ...) per level, as make_pyramid: 8-px tiles, halved (rounded up) until one tile is left"""
    nx, ny = (W + 7) // 8, (H + 7) // 8
    out = []
    while True:
        out.append((nx, ny))
        if (nx == 1 and ny == 1) or len(out) == MAX_LEVELS:
            return tuple(out)
        nx, ny = (nx + 1) // 2, (ny + 1) // 2


def scaled(s: Setup, depth, scale=1.0):
    """(scaled depth, valid) as every TSDF kernel reads a pixel"""
    d = (np.ascontiguousarray(depth, F32) * F32(scale)).astype(F32)
    with np.errstate(invalid="ignore"):
        return d, (d > F32(s.mind)) & (d < F32(s.maxd))


def _pad(a, rows, cols, fill):
    out = np.full((rows, cols), fill, a.dtype)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def pyramid_by_reduction(s: Setup, depth, scale=1.0, fault=None):
    """[(min, max, allvalid)] per level, arrays [nty, ntx]: level 0 from the pixels the image has of each tile, every other level as
    the 2x2 reduction of the one below over the children that exist"""
    d, valid = scaled(s, depth, scale)
    shapes = level_shapes(s.W, s.H)
    ntx, nty = shapes[0]
    lo = _pad(np.where(valid, d, INF), 8 * nty, 8 * ntx, INF).reshape(nty, 8, ntx, 8).min(axis=(1, 3))
    hi = _pad(np.where(valid, d, -INF), 8 * nty, 8 * ntx, -INF).reshape(nty, 8, ntx, 8).max(axis=(1, 3))
    bad = _pad(~valid, 8 * nty, 8 * ntx, fault == "partial_tile_invalid").reshape(nty, 8, ntx, 8).any(axis=(1, 3))
    levels = [(lo.astype(F32), hi.astype(F32), ~bad)]
    for L in range(1, len(shapes)):
        lo, hi, ok = levels[-1]
        if L >= 3 and fault == "drop_last_col" and lo.shape[1] & 1:
            lo, hi, ok = lo[:, :-1], hi[:, :-1], ok[:, :-1]
        if L >= 3 and fault == "drop_last_row" and lo.shape[0] & 1:
            lo, hi, ok = lo[:-1], hi[:-1], ok[:-1]
        ntx, nty = shapes[L]
        lo = _pad(lo, 2 * nty, 2 * ntx, INF).reshape(nty, 2, ntx, 2).min(axis=(1, 3))
        hi = _pad(hi, 2 * nty, 2 * ntx, -INF).reshape(nty, 2, ntx, 2).max(axis=(1, 3))
        ok = _pad(ok, 2 * nty, 2 * ntx, True).reshape(nty, 2, ntx, 2).all(axis=(1, 3))
        for k in (0, 1, 2):
            if fault == f"allvalid_lost_above_{k}" and L > k:
                ok = np.ones_like(ok)
        levels.append((lo, hi, ok))
    return levels


def pyramid_brute_force(s: Setup, depth, scale=1.0):
    """the same tables straight from the pixels of every tile of every level"""
    d, valid = scaled(s, depth, scale)
    levels = []
    for L, (ntx, nty) in enumerate(level_shapes(s.W, s.H)):
        t = 8 << L
        lo, hi, ok = np.full((nty, ntx), INF, F32), np.full((nty, ntx), -INF, F32), np.ones((nty, ntx), bool)
        for ty in range(nty):
            for tx in range(ntx):
                dd, vv = d[t * ty:t * ty + t, t * tx:t * tx + t], valid[t * ty:t * ty + t, t * tx:t * tx + t]
                assert dd.size > 0
                if vv.any():
                    lo[ty, tx], hi[ty, tx] = dd[vv].min(), dd[vv].max()
                ok[ty, tx] = vv.all()
        levels.append((lo, hi, ok))
    return levels


# ---- frustum, poses --------------------------------------------------------------------------------------------------------------------
def frustum(s: Setup):
    """make_frustum (api_fuse.hip): the image's side planes, widened by one pixel on every side; doubles, rounded to f32 at the end"""
    aL, aR = (-1.5 - s.cx) / s.fx, (s.W + 0.5 - s.cx) / s.fx
    aT, aB = (-1.5 - s.cy) / s.fy, (s.H + 0.5 - s.cy) / s.fy
    f = {}
    n = math.sqrt(1.0 + aL * aL); f["lx"], f["lz"] = F32(1.0 / n), F32(-aL / n)
    n = math.sqrt(1.0 + aR * aR); f["rx"], f["rz"] = F32(-1.0 / n), F32(aR / n)
    n = math.sqrt(1.0 + aT * aT); f["ty"], f["tz"] = F32(1.0 / n), F32(-aT / n)
    n = math.sqrt(1.0 + aB * aB); f["by"], f["bz"] = F32(-1.0 / n), F32(aB / n)
    return f


def _sphere_in_view(fr, x, y, z, rad):
    return bool((z + rad > 0) and (fr["lx"] * x + fr["lz"] * z >= -rad) and (fr["rx"] * x + fr["rz"] * z >= -rad) and
                (fr["ty"] * y + fr["tz"] * z >= -rad) and (fr["by"] * y + fr["bz"] * z >= -rad))


def _fma(a, b, c):
    """scalar fma: the f32 product is exact in a double, the sum is rounded there and once more to f32 (a double rounding that can
    move the last bit of one value in 2^29: far inside what a robust case tolerates)"""
    return F32(float(a) * float(b) + float(c))


def _cam_point(r, t, x, y, z):
    return (r[0] * x + r[1] * y + r[2] * z + t[0], r[3] * x + r[4] * y + r[5] * z + t[1], r[6] * x + r[7] * y + r[8] * z + t[2])


@dataclass(frozen=True)
class Box:
    """what a classifier knows of a box of voxels before it looks at the pyramid: `early` = its class if decided already (else
    None), the pixel bounds widened by 1.5 px and the camera depths of the voxel centres / corners"""
    early: Optional[int]
    why: str = ""
    umin: float = 0.0
    umax: float = 0.0
    vmin: float = 0.0
    vmax: float = 0.0
    zmin: float = 0.0
    zmax: float = 0.0


def brick_box(s: Setup, R, t, bx, by, bz) -> Box:
    """brick_cull up to the pyramid lookups: the cell's and the brick's sphere against the widened frustum, the camera-plane guard,
    the eight corners"""
    r, tt = sn._pose32(R, t)
    fr = frustum(s)
    vs, o = F32(s.voxel), [F32(v) for v in s.origin]
    ccx, ccy, ccz = bx >> 2, by >> 2, bz >> 2
    crad = F32(27.712812) * vs * F32(1.01)
    q = [_fma(F32(c * 32 + 16), vs, o[a]) for a, c in enumerate((ccx, ccy, ccz))]
    if not _sphere_in_view(fr, *_cam_point(r, tt, *q), crad):
        return Box(SKIP, "cell")
    rad = F32(6.9282032) * vs * F32(1.01)
    w = [_fma(F32(b * 8 + 4), vs, o[a]) for a, b in enumerate((bx, by, bz))]
    cxm, cym, czm = _cam_point(r, tt, *w)
    if not _sphere_in_view(fr, cxm, cym, czm, rad):
        return Box(SKIP, "sphere")
    if not (czm - rad > F32(1e-3)):
        return Box(MIXED, "camera plane")
    h = F32(4.0) * vs
    us, vv, zs = [], [], []
    for k in range(8):
        sx, sy, sz = (h if k & 1 else -h), (h if k & 2 else -h), (h if k & 4 else -h)
        x = cxm + r[0] * sx + r[1] * sy + r[2] * sz
        y = cym + r[3] * sx + r[4] * sy + r[5] * sz
        z = czm + r[6] * sx + r[7] * sy + r[8] * sz
        iz = F32(1.0) / z
        us.append(F32(s.fx) * x * iz + F32(s.cx))
        vv.append(F32(s.fy) * y * iz + F32(s.cy))
        zs.append(z)
    return Box(None, "", float(min(us)) - 1.5, float(max(us)) + 1.5, float(min(vv)) - 1.5, float(max(vv)) + 1.5, float(min(zs)), float(max(zs)))


def subbrick_box(s: Setup, R, t, i0, j0, k0) -> Box:
    """classify_subbrick up to the pyramid lookups: the eight extreme voxel centres of the 4x4x4 sub-brick at voxel (i0, j0, k0) by
    the per-voxel position sequence"""
    r, tt = sn._pose32(R, t)
    vs, o = F32(s.voxel), [F32(v) for v in s.origin]
    wx = [_fma(F32(i0 + 3 * h) + F32(0.5), vs, o[0]) for h in (0, 1)]
    wy = [_fma(F32(j0 + 3 * h) + F32(0.5), vs, o[1]) for h in (0, 1)]
    wz = [_fma(F32(k0 + 3 * h) + F32(0.5), vs, o[2]) for h in (0, 1)]
    pts = []
    for hz, hy, hx in itertools.product((0, 1), repeat=3):
        pts.append(tuple(_fma(r[3 * a], wx[hx], _fma(r[3 * a + 1], wy[hy], _fma(r[3 * a + 2], wz[hz], tt[a]))) for a in range(3)))
    zmin, zmax = min(p[2] for p in pts), max(p[2] for p in pts)
    if not (zmin > F32(1e-3)):
        return Box(MIXED, "camera plane")
    us = [F32(s.fx) * x * (F32(1.0) / z) + F32(s.cx) for x, _, z in pts]
    vv = [F32(s.fy) * y * (F32(1.0) / z) + F32(s.cy) for _, y, z in pts]
    return Box(None, "", float(min(us)) - 1.5, float(max(us)) + 1.5, float(min(vv)) - 1.5, float(max(vv)) + 1.5, float(zmin), float(zmax))


# ---- the three rules on one box ----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Verdict:
    cls: int
    why: str = ""
    level: int = -1
    tiles: Tuple[Tuple[int, int], ...] = ()       # (tx, ty) in the order they are looked at (repeats left out)
    window: Tuple[int, int] = (0, 0)              # tiles per axis of the pixel box at `level`
    inside: bool = False


def classify_box(s: Setup, a, zmin, zmax, inside, fault=None):
    """a = (min, max, allvalid) over a superset of the box's pixels; 1 % of a voxel on depths, 0.1 % on the truncation distance"""
    m = F32(0.01) * F32(s.voxel)
    trunc = F32(s.trunc)
    lo, hi, ok = F32(a[0]), F32(a[1]), bool(a[2])
    far = lo if fault == "swap_min_max_in_skip" else hi
    if not (far > -INF) or (F32(zmin) - m > far + trunc):
        return SKIP
    if inside and ok and (lo - (F32(zmax) + m) >= trunc * F32(1.001)):
        return FREE
    return MIXED


def box_class(s: Setup, pyr, box: Box, kind, fault=None, pert=(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)) -> Verdict:
    """class of a box from the pyramid: the pixel-box tests, the level choice, the lookup window, classify_box.
    kind "brick": finest level with <= 4 tiles per axis, a clamped 4x4 loop; "sub": finest level with <= 8 tiles, walked row by row.
    pert = what is added to (umin, umax, vmin, vmax, zmin, zmax)"""
    v, a = _lookup(s, pyr, box, kind, fault, pert[:4])
    if a is None:
        return v
    cls = classify_box(s, a, F32(box.zmin + pert[4]), F32(box.zmax + pert[5]), v.inside or fault == "ignore_inside", fault)
    return Verdict(cls, "box", v.level, v.tiles, v.window, v.inside)


def _lookup(s: Setup, pyr, box: Box, kind, fault, pert_uv):
    """(the verdict, final if there is nothing to look up; else what the looked-at tiles say: (min, max, allvalid))"""
    if box.early is not None:
        return Verdict(box.early, box.why), None
    umin, umax, vmin, vmax = (F32(b + p) for b, p in zip((box.umin, box.umax, box.vmin, box.vmax), pert_uv))
    W, H = s.W, s.H
    if umax < 0 or vmax < 0 or umin > F32(W - 1) or vmin > F32(H - 1):
        return Verdict(SKIP, "pixel box"), None
    inside = bool(umin >= 0 and vmin >= 0 and umax <= F32(W - 1) and vmax <= F32(H - 1))
    pu0, pu1 = max(0, int(math.floor(umin))), min(W - 1, int(math.ceil(umax)))
    pv0, pv1 = max(0, int(math.floor(vmin))), min(H - 1, int(math.ceil(vmax)))
    nlev = len(pyr)

    def span(L):
        sh = TILE0_SHIFT + L
        return (pu1 >> sh) - (pu0 >> sh) + 1, (pv1 >> sh) - (pv0 >> sh) + 1

    L = 0
    if kind == "brick":
        while L < nlev - 1 and max(span(L)) > 4:
            L += 1
    else:
        while L < nlev - 1 and span(L)[0] * span(L)[1] > 8:
            L += 1
    if fault == "level_one_too_fine" and L > 0:
        L -= 1
    nu, nv = span(L)
    tu0, tv0 = pu0 >> (TILE0_SHIFT + L), pv0 >> (TILE0_SHIFT + L)
    tiles = []
    if kind == "brick":
        n = 3 if fault == "window_3x3" else 4
        for dv in range(n):
            for du in range(n):
                tiles.append((min(tu0 + du, tu0 + nu - 1), min(tv0 + dv, tv0 + nv - 1)))
    else:
        du = dv = 0
        for _ in range(8):
            tiles.append((tu0 + du, tv0 + dv))
            if du + 1 < nu:
                du += 1
            elif dv + 1 < nv and fault != "walk_first_row_only":
                du, dv = 0, dv + 1
    tiles = tuple(dict.fromkeys(tiles))
    lo, hi, ok = pyr[L]
    a = (min(lo[ty, tx] for tx, ty in tiles), max(hi[ty, tx] for tx, ty in tiles), all(ok[ty, tx] for tx, ty in tiles))
    return Verdict(MIXED, "box", L, tiles, (nu, nv), inside), a


def _moves(e):
    return ((0.0, 0.0), (-e, e), (e, -e), (e, e), (-e, -e))


def perturbations(s: Setup):
    """the 125 moves of a box a robust case must survive: each pixel axis grown, shrunk or shifted by 0.25 px, the depth range
    likewise by 0.5 % of a voxel"""
    for mu in _moves(0.25):
        for mv in _moves(0.25):
            for mz in _moves(0.005 * s.voxel):
                yield mu + mv + mz


def robust_classes(s: Setup, pyr, box: Box, kind):
    """(the unperturbed verdict, the set of (class, level, window, inside) over all perturbations()) -- the lookup is made once per
    move of the pixel box, the depth rule once per move of the depth range on top of it"""
    v0 = box_class(s, pyr, box, kind)
    if box.early is not None:
        return v0, {(v0.cls, -1, (0, 0), False)}
    seen = set()
    for mu in _moves(0.25):
        for mv in _moves(0.25):
            v, a = _lookup(s, pyr, box, kind, None, mu + mv)
            if a is None:
                seen.add((v.cls, v.level, v.window, v.inside))
                continue
            for mz in _moves(0.005 * s.voxel):
                cls = classify_box(s, a, F32(box.zmin + mz[0]), F32(box.zmax + mz[1]), v.inside)
                seen.add((cls, v.level, v.window, v.inside))
    return v0, seen


def subbrick_origin(bx, by, bz, sb):
    return bx * 8 + (sb & 1) * 4, by * 8 + ((sb >> 1) & 1) * 4, bz * 8 + (sb >> 2) * 4


def classify_frame(s: Setup, depth, R, t, scale=1.0, fault=None, subs=True, pyr=None):
    """{(bx, by, bz): (brick Verdict, [8 sub-brick Verdicts] of a MIXED brick or None)}"""
    if pyr is None:
        pyr = pyramid_by_reduction(s, depth, scale, fault if fault in PYRAMID_FAULTS else None)
    out = {}
    for bz, by, bx in itertools.product(*(range(n) for n in s.nb[::-1])):
        v = box_class(s, pyr, brick_box(s, R, t, bx, by, bz), "brick", fault)
        sv = None
        if subs and v.cls == MIXED:
            sv = [box_class(s, pyr, subbrick_box(s, R, t, *subbrick_origin(bx, by, bz, sb)), "sub", fault) for sb in range(8)]
        out[(bx, by, bz)] = (v, sv)
    return out


def robust_counts(s: Setup, depth, R, t, scale=1.0):
    """(most bricks a rule as tight as the model's may visit, fewest it must call FREE): a brick counts as visited if ANY
    perturbation leaves it MIXED or FREE, as free only if EVERY perturbation calls it FREE; plus the unperturbed (visited, free)"""
    pyr = pyramid_by_reduction(s, depth, scale)
    vis_hi = free_lo = vis = free = 0
    for bz, by, bx in itertools.product(*(range(n) for n in s.nb[::-1])):
        v0, seen = robust_classes(s, pyr, brick_box(s, R, t, bx, by, bz), "brick")
        classes = {c[0] for c in seen}
        vis_hi += classes != {SKIP}
        free_lo += classes == {FREE}
        vis += v0.cls != SKIP
        free += v0.cls == FREE
    return int(vis_hi), int(free_lo), int(vis), int(free)


# ---- per-voxel truth ---------------------------------------------------------------------------------------------------------------------
def voxel_truth(s: Setup, depth, R, t, scale=1.0):
    """per voxel [nz, ny, nx]: updated?, quantised value, in-window?, pixel (u, v) -- the second oracle's own helpers"""
    g = s.geometry()
    nx, ny, nz = g.dims
    r, tt = sn._pose32(R, t)
    half = F32(0.5)
    wx = sn.fma32(np.arange(nx, dtype=F32) + half, g.voxel, g.origin[0])
    wy = sn.fma32(np.arange(ny, dtype=F32) + half, g.voxel, g.origin[1])
    wz = sn.fma32(np.arange(nz, dtype=F32) + half, g.voxel, g.origin[2])
    K, J, I = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    xc, yc, zc = sn._transform(r, tt, wx[I], wy[J], wz[K])
    win, u, v = sn._project(g, xc, yc, zc)
    d, valid = scaled(s, depth, scale)
    with np.errstate(invalid="ignore", over="ignore"):
        dd = d[v, u]
        sdf = dd - zc
        upd = win & valid[v, u] & (sdf >= -g.trunc)
        q = np.rint(np.minimum(F32(1.0), sdf * g.inv_trunc) * F32(32767.0))
    q = np.where(upd, q, 0).astype(np.int64)
    return dict(upd=upd, q=q, win=win, u=u, v=v, zc=zc)


def permitted(truth, cell):
    """(skip permitted, free permitted) per box of cell^3 voxels, arrays [nz/cell, ny/cell, nx/cell]: skip iff no voxel is updated,
    free iff every voxel is updated with q = 32767"""
    upd, q = truth["upd"], truth["q"]
    nz, ny, nx = upd.shape
    shape = (nz // cell, cell, ny // cell, cell, nx // cell, cell)
    skip_ok = ~upd.reshape(shape).any(axis=(1, 3, 5))
    free_ok = (upd & (q == 32767)).reshape(shape).all(axis=(1, 3, 5))
    return skip_ok, free_ok


def unsound(s: Setup, classes, truth):
    """the (brick, sub-brick or None, class) answers of classify_frame that the per-voxel truth forbids"""
    bs, bf = permitted(truth, 8)
    ss, sf = permitted(truth, 4)
    bad = []
    for (bx, by, bz), (v, sv) in classes.items():
        if (v.cls == SKIP and not bs[bz, by, bx]) or (v.cls == FREE and not bf[bz, by, bx]):
            bad.append(((bx, by, bz), None, v.cls))
        for sb, w in enumerate(sv or ()):
            i0, j0, k0 = subbrick_origin(bx, by, bz, sb)
            if (w.cls == SKIP and not ss[k0 // 4, j0 // 4, i0 // 4]) or (w.cls == FREE and not sf[k0 // 4, j0 // 4, i0 // 4]):
                bad.append(((bx, by, bz), sb, w.cls))
    return bad
