"""Crafted frames that put the TSDF update on its decision edges, and counters that prove the edges are hit.

The geometry is DYADIC: camera 40 x 24, fx = fy = 32, cx = 20, cy = 12; grid 16 x 16 x 24 voxels of 1/32 at
(-1/4, -1/4, 1/2 - 1/64) with trunc = 1/8; poses R = I (or a signed axis permutation) with translations that are multiples of
1/64 (one of them + 2^-20).  Every voxel centre, camera point and signed distance is then exact in f32, the slice k = 16 lies at
zc = 1 where 1/zc is exact, and the pixel coordinates of that slice fall exactly on rounding ties n + 0.5, on tile borders and --
for the shifted poses -- on the window borders -0.5 and W - 0.5.

The depth image is a patchwork of one THEME per 8x8-pixel tile (the unit of the update kernel's per-voxel tile test): surfaces
exactly trunc behind / in front of the zc = 1 slice, their f32 neighbours, the half-way rounding tie, far walls and near walls;
two tiles in three carry one ODD pixel (invalid values, the depth limits themselves, a near value in a far tile and the other
way round).  Variants (ragged and tiny cameras, one-brick and five-brick grids, all 24 axis permutations, general rotations,
scales, 16-bit frames, degenerate frames) are built from the family by functions below.

counters() restates the 8x8 tile rule of the update kernel in plain numpy and counts, per frame, how many voxels sit on each
edge; tests/test_tsdf_edges_reference_cpu.py pins the counts, so an edit that silently loses an edge fails there.
"""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass, field, replace
from typing import Optional, Tuple

import numpy as np

from oracle import second_numpy as sn

F32 = np.float32

CAM = dict(width=40, height=24, fx=32.0, fy=32.0, cx=20.0, cy=12.0)
MIN_DEPTH, MAX_DEPTH = 0.5, 4.0
DIMS = (16, 16, 24)
VOXEL = 1.0 / 32
ORIGIN = (-0.25, -0.25, 0.5 - 1.0 / 64)
TRUNC = 0.125


def _next(x, towards):
    return float(np.nextafter(F32(x), F32(towards)))


BAND = float(F32(1.0) + F32(0.125) * F32(1.0005))          # sdf in the STRICT interior of [trunc, 1.001 trunc) under zc = 1
T10005 = float(F32(1.125) * F32(1.0005))
THEMES = dict(behind=0.875, behind_lo=_next(0.875, 0), front=1.125, front_lo=_next(1.125, 0), front_hi=T10005, half=1.0625,
              far=3.0, near=0.6, band=BAND)
# one theme per tile; the zc = 1 slice of the t = 0 pose covers pixels 13..28 x 5..20, i.e. tile columns 1..3 of every row
_LAYOUT = (("far", "behind", "front", "front_lo", "near"),
           ("near", "behind_lo", "half", "band", "far"),
           ("half", "front_hi", "behind", "front", "far"))
# the odd pixel of the n-th odd tile ("swap": a near value in a far tile, a far value in any other)
_ODD = (0.0, float("nan"), float("inf"), -1.0, 0.5, _next(0.5, 1), "swap", 4.0, "swap", _next(4.0, 0))


def tile_theme(tx, ty):
    return _LAYOUT[ty % 3][(tx + ty // 3) % 5]


def tile_odd(tx, ty):
    """None, or the odd value of tile (tx, ty): two tiles in three have one"""
    n = tx + 5 * ty
    if n % 3 == 2:
        return None
    v = _ODD[(n - n // 3) % len(_ODD)]
    if v == "swap":
        return THEMES["behind"] if tile_theme(tx, ty) == "far" else THEMES["far"]
    return v


@functools.lru_cache(maxsize=None)
def patchwork(width, height):
    """The themed image of any size: tiles beyond the 5 x 3 of the family repeat the layout (shifted by one per three rows), and a
    tile's odd pixel moves inside what the image leaves of the tile -- a partial last column / row gets themes and odd pixels.
    One read-only array per size: frames that share the image share the object."""
    d = np.zeros((height, width), F32)
    for ty in range((height + 7) // 8):
        for tx in range((width + 7) // 8):
            tw, th = min(8, width - 8 * tx), min(8, height - 8 * ty)
            d[8 * ty:8 * ty + th, 8 * tx:8 * tx + tw] = F32(THEMES[tile_theme(tx, ty)])
            odd = tile_odd(tx, ty)
            if odd is not None:
                n = tx + 5 * ty
                d[8 * ty + (5 * n + 2) % th, 8 * tx + (3 * n + 1) % tw] = F32(odd)
    d.setflags(write=False)
    return d


@dataclass(frozen=True)
class Case:
    """one frame and the grid it is fused into"""
    name: str
    depth: np.ndarray = field(repr=False, compare=False)      # float32 [H, W] as the oracle reads it (a u16 frame: converted)
    R: np.ndarray = field(repr=False, compare=False)
    t: np.ndarray = field(repr=False, compare=False)
    cam: dict = field(default_factory=lambda: dict(CAM))
    dims: Tuple[int, int, int] = DIMS
    origin: Tuple[float, float, float] = ORIGIN
    scale: float = 1.0
    dyadic: bool = True                                       # the exact-rational model applies
    mm: Optional[np.ndarray] = field(default=None, repr=False, compare=False)    # the uint16 millimetre image, if that is what is uploaded

    @property
    def pose(self):
        return (self.R, self.t)

    @property
    def upload(self):
        return self.depth if self.mm is None else self.mm


def geometry(case: Case) -> sn.Geometry:
    c = case.cam
    return sn.Geometry(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], MIN_DEPTH, MAX_DEPTH, case.dims, case.origin,
                       VOXEL, TRUNC)


def c_oracle_for(case: Case):
    from oracle import c_oracle
    c = case.cam
    return c_oracle.Oracle(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], min_depth=MIN_DEPTH, max_depth=MAX_DEPTH,
                           dims=case.dims, origin=case.origin, voxel_size=VOXEL, sdf_trunc=TRUNC)


# ---- poses ---------------------------------------------------------------------------------------------------------------------
I3 = np.eye(3)
TRANSLATIONS = (
    ("t0", (0.0, 0.0, 0.0)),                       # ties uf = n + 0.5 on the zc = 1 slice, some on tile borders
    ("left", (-13 / 32, 0.0, 0.0)),                # uf == -0.5 exactly: inside the window
    ("right", (12 / 32, 0.0, 0.0)),                # uf == W - 0.5 exactly: outside
    ("top", (0.0, -13 / 32, 0.0)),                 # vf == -0.5
    ("bottom", (0.0, 12 / 32, 0.0)),               # vf == H - 0.5
    ("zhalf", (0.0, 0.0, -0.5)),                   # slice k = 0 on the camera plane
    ("zone", (0.0, 0.0, -1.0)),                    # slice k = 16 on the camera plane, sixteen slices behind the camera
    ("eps_x", (1 / 64, 0.0, -1.0 + 2.0 ** -20)),   # a row of voxels at xc = 0, zc = 2^-20 (below the classifiers' 1e-3 guard): vf far outside
    ("eps_xy", (1 / 64, 1 / 64, -1.0 + 2.0 ** -20)),   # ... and the voxel (7, 7, 16) at xc = yc = 0: IN the window, pixel (20, 12)
)


def axis_permutations():
    """the 24 proper signed axis permutations (rotations of the cube), exact in f32"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for row, (col, s) in enumerate(zip(perm, signs)):
                R[row, col] = s
            if np.linalg.det(R) > 0:
                out.append(R)
    assert len(out) == 24
    return out


def grid_centre(dims=DIMS, origin=ORIGIN):
    return np.array([origin[a] + 0.5 * dims[a] * VOXEL for a in range(3)])


def recentre(R, dims=DIMS, origin=ORIGIN):
    """t such that the grid centre goes to (0, 0, its own depth): a multiple of 1/64 for an axis permutation"""
    c = grid_centre(dims, origin)
    return np.array([0.0, 0.0, grid_centre()[2]]) - np.asarray(R) @ c


def general_rotations():
    """two rotations with no zero entry (compared with the oracles only)"""
    out = []
    for axis, deg in (((1.0, 2.0, 3.0), 17.0), ((-2.0, 1.0, 0.5), -31.0)):
        a = np.array(axis) / np.linalg.norm(axis)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        th = np.deg2rad(deg)
        out.append(np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K))
    return out


# ---- the family and its variants -----------------------------------------------------------------------------------------------
def base_case(name="t0", t=(0.0, 0.0, 0.0), R=I3, **kw):
    return Case(name=name, depth=patchwork(CAM["width"], CAM["height"]), R=np.asarray(R, float), t=np.asarray(t, float), **kw)


def family():
    """R = I with the nine translations: what the counters are pinned for"""
    return [base_case(n, t) for n, t in TRANSLATIONS]


def permutation_cases():
    return [base_case(f"perm{i:02d}", recentre(R), R) for i, R in enumerate(axis_permutations())]


def with_camera(case, width, height, name, depth=None, **cam_kw):
    cam = dict(case.cam, width=width, height=height, **cam_kw)
    return replace(case, name=name, cam=cam, depth=patchwork(width, height) if depth is None else depth)


def crop(depth, u0, v0, w, h):
    return np.ascontiguousarray(depth[v0:v0 + h, u0:u0 + w])


def with_grid(case, dims, first_voxel, name):
    """a grid of `dims` voxels whose voxel (0, 0, 0) is voxel `first_voxel` of the family's lattice"""
    origin = tuple(ORIGIN[a] + first_voxel[a] * VOXEL for a in range(3))
    return replace(case, name=name, dims=tuple(dims), origin=origin)


def as_u16(case, name):
    """the frame rounded to millimetres (what a 16-bit PNG holds); every kind of special value once in the corner tile"""
    with np.errstate(invalid="ignore"):
        mm = np.where(np.isfinite(case.depth) & (case.depth > 0), np.rint(case.depth.astype(np.float64) * 1000.0), 0.0)
    mm = np.clip(mm, 0, 65535).astype(np.uint16)
    mm[1, 1:5] = (0, 65535, 500, 501)                # hole, saturated, min_depth in millimetres (invalid), the first valid value
    return replace(case, name=name, mm=mm, depth=mm.astype(F32) / F32(1000.0))


def variants():
    t0 = base_case()
    out = []
    # ragged cameras: themes and odd pixels in the partial last tile column (2 px) and row (3 px)
    out.append(with_camera(t0, 42, 27, "ragged_t0"))
    out.append(with_camera(base_case("right", (12 / 32, 0.0, 0.0)), 42, 27, "ragged_right"))
    out.append(with_camera(base_case("bottom", (0.0, 12 / 32, 0.0)), 42, 27, "ragged_bottom"))
    # 4 x 3 pixels around the corner where four tiles of the family meet: one pyramid level, less than one tile
    out.append(with_camera(t0, 4, 3, "tiny", depth=crop(t0.depth, 14, 6, 4, 3), fx=4.0, fy=4.0, cx=2.0, cy=1.5))
    # one brick around the zc = 1 slice; five bricks in x (crosses a 4-brick cell), ties from u = 0.5 to W - 0.5
    out.append(with_grid(t0, (8, 8, 8), (4, 4, 12), "one_brick"))
    out.append(with_grid(t0, (40, 8, 8), (-12, 4, 12), "five_bricks"))
    out.append(with_grid(base_case("left", (-1 / 64, 0.0, 0.0)), (40, 8, 8), (-12, 4, 12), "five_bricks_half_px"))
    out.append(with_grid(t0, (40, 16, 24), (-12, 0, 0), "largest"))
    # scales: image halved (exact), image divided by 3 (inexact)
    out.append(replace(t0, name="scale2", depth=t0.depth * F32(0.5), scale=2.0))
    out.append(replace(t0, name="scale3", depth=(t0.depth / F32(3.0)).astype(F32), scale=3.0, dyadic=False))
    for i, R in enumerate(general_rotations()):
        out.append(base_case(f"rot{i}", recentre(R), R, dyadic=False))
    # 16-bit millimetre frames (0.6 m and 3 m are exact multiples; the f32 neighbours collapse onto the millimetre grid)
    out.append(as_u16(t0, "u16_t0"))
    out.append(as_u16(base_case("left", (-13 / 32, 0.0, 0.0)), "u16_left"))
    out.append(no_valid_pixel())
    out.append(last_pixel_only())
    out.append(all_free())
    return out


def no_valid_pixel(name="no_valid"):
    """holes, NaN and max_depth itself, in turn"""
    n = np.arange(CAM["height"] * CAM["width"]).reshape(CAM["height"], CAM["width"]) % 3
    return replace(base_case(name), depth=np.choose(n, [F32(0.0), F32(np.nan), F32(MAX_DEPTH)]).astype(F32))


def last_pixel_only(name="last_pixel"):
    """the only valid pixel is (W - 1, H - 1); the pose looks at it through the grid"""
    d = np.zeros((CAM["height"], CAM["width"]), F32)
    d[-1, -1] = F32(1.0625)
    return replace(base_case(name, (12 / 32 - 1 / 64, 4 / 32 - 1 / 64, 0.0)), depth=d)


def all_free(name="all_free"):
    return replace(base_case(name), depth=np.full((CAM["height"], CAM["width"]), 3.0, F32))


def saturating_behind(name="all_behind"):
    """every voxel of the zc = 1 slice gets sdf == -trunc, q == -32767"""
    return replace(base_case(name), depth=np.full((CAM["height"], CAM["width"]), 0.875, F32))


def all_cases():
    return family() + permutation_cases() + variants()


# ---- intermediates of the per-voxel rule (the numpy oracle's own helpers) and the tile rule ----------------------------------------
def intermediates(case: Case):
    g = geometry(case)
    nx, ny, nz = g.dims
    r, tt = sn._pose32(case.R, case.t)
    half = F32(0.5)
    wx = sn.fma32(np.arange(nx, dtype=F32) + half, g.voxel, g.origin[0])
    wy = sn.fma32(np.arange(ny, dtype=F32) + half, g.voxel, g.origin[1])
    wz = sn.fma32(np.arange(nz, dtype=F32) + half, g.voxel, g.origin[2])
    K, J, I = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    xc, yc, zc = sn._transform(r, tt, wx[I], wy[J], wz[K])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = F32(1.0) / zc
        uf = sn.fma32(g.fx * xc, inv, g.cx)
        vf = sn.fma32(g.fy * yc, inv, g.cy)
    win, u, v = sn._project(g, xc, yc, zc)
    d = (np.ascontiguousarray(case.depth, F32) * F32(case.scale)).astype(F32)
    with np.errstate(invalid="ignore"):
        valid_img = (d > g.mind) & (d < g.maxd)
    return dict(g=g, I=I, J=J, K=K, xc=xc, yc=yc, zc=zc, uf=uf, vf=vf, win=win, u=u, v=v, d_img=d, valid_img=valid_img)


def tile_tables(d_img, valid_img):
    """per 8x8 tile (over the pixels the image has of it): lowest depth if every pixel is valid else -inf, highest valid depth
    (-inf if none), number of invalid pixels"""
    H, W = d_img.shape
    nty, ntx = (H + 7) // 8, (W + 7) // 8
    lo = np.full((nty, ntx), -np.inf, F32)
    hi = np.full((nty, ntx), -np.inf, F32)
    bad = np.zeros((nty, ntx), np.int64)
    for ty in range(nty):
        for tx in range(ntx):
            dd, ok = d_img[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8], valid_img[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
            bad[ty, tx] = (~ok).sum()
            if ok.any():
                hi[ty, tx] = dd[ok].max()
            if ok.all():
                lo[ty, tx] = dd.min()
    return lo, hi, bad


COUNTER_NAMES = ("ties", "ties_on_tile_border", "u_eq_left", "u_eq_right", "v_eq_top", "v_eq_bottom", "sdf_eq_minus_trunc",
                 "sdf_just_below_minus_trunc", "sdf_eq_trunc", "sdf_in_free_band", "sdf_inside_free_band", "half_way_tie",
                 "hi_eq_minus_trunc", "over_single_invalid_pixel", "tile_free", "tile_skip", "tile_open", "open_ends_one",
                 "open_ends_without_update", "zc_eq_0", "zc_lt_0", "zc_below_guard")


def counters(case: Case) -> dict:
    m = intermediates(case)
    g, zc, uf, vf, win, u, v = m["g"], m["zc"], m["uf"], m["vf"], m["win"], m["u"], m["v"]
    trunc = g.trunc
    trunc_free = F32(trunc * F32(1.001))
    front = zc > 0
    wl, hl = F32(g.W) - F32(0.5), F32(g.H) - F32(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        u_in = front & (uf >= F32(-0.5)) & (uf < wl)
        v_in = front & (vf >= F32(-0.5)) & (vf < hl)
        tie_u = win & (uf - np.floor(uf) == F32(0.5))
        tie_v = win & (vf - np.floor(vf) == F32(0.5))
        border_u = tie_u & ((np.floor(uf) + 1) % 8 == 0)
        border_v = tie_v & ((np.floor(vf) + 1) % 8 == 0)
        d = m["d_img"][v, u]
        ok_pix = win & m["valid_img"][v, u]
        sdf = d - zc
        upd = ok_pix & (sdf >= -trunc)
        tsdf = np.minimum(F32(1.0), sdf * g.inv_trunc)
        prod = tsdf * F32(32767.0)
        lo, hi, bad = tile_tables(m["d_img"], m["valid_img"])
        tlo, thi, tbad = lo[v >> 3, u >> 3], hi[v >> 3, u >> 3], bad[v >> 3, u >> 3]
        free = win & (tlo - zc >= trunc_free)
        skip = win & ~(thi - zc >= -trunc)
        opn = win & ~free & ~skip
        out = dict(
            ties=(tie_u | tie_v).sum(), ties_on_tile_border=(border_u | border_v).sum(),
            u_eq_left=(front & v_in & (uf == F32(-0.5))).sum(), u_eq_right=(front & v_in & (uf == wl)).sum(),
            v_eq_top=(front & u_in & (vf == F32(-0.5))).sum(), v_eq_bottom=(front & u_in & (vf == hl)).sum(),
            sdf_eq_minus_trunc=(ok_pix & (sdf == -trunc)).sum(),
            sdf_just_below_minus_trunc=(ok_pix & (sdf < -trunc) & (sdf >= -trunc * F32(1.000001))).sum(),
            sdf_eq_trunc=(ok_pix & (sdf == trunc)).sum(),
            sdf_in_free_band=(ok_pix & (sdf >= trunc) & (sdf < trunc_free)).sum(),
            sdf_inside_free_band=(ok_pix & (sdf > trunc) & (sdf < trunc_free)).sum(),
            half_way_tie=(upd & (np.abs(prod - np.trunc(prod)) == F32(0.5))).sum(),
            hi_eq_minus_trunc=(win & (thi - zc == -trunc)).sum(),
            over_single_invalid_pixel=(win & ~m["valid_img"][v, u] & (tbad == 1)).sum(),
            tile_free=free.sum(), tile_skip=skip.sum(), tile_open=opn.sum(),
            open_ends_one=(opn & upd & (tsdf == F32(1.0))).sum(), open_ends_without_update=(opn & ~upd).sum(),
            zc_eq_0=(zc == 0).sum(), zc_lt_0=(zc < 0).sum(), zc_below_guard=((zc > 0) & (zc < F32(1e-3))).sum())
    # the tile rule is conservative: what it decides is what the per-voxel rule decides
    assert not (free & ~(upd & (tsdf == F32(1.0)))).any() and not (skip & upd).any(), case.name
    return {k: int(out[k]) for k in COUNTER_NAMES}

