"""Crafted grids for the point-extraction tests (tests/test_extract_reference_cpu.py on the CPU, tests/test_gpu_extract.py on the
GPU: the same seeds, the same bytes).  A voxel is drawn from a CLASS TABLE, not from a smooth field, so every combination of the
values at which the rule could go wrong meets every other across an edge of every axis."""
import functools
import itertools

import numpy as np

import extract_reference as er
from helpers_cpu import ulp_diff

MW = 2                                            # the min_weight the sweeps use next to 0
W_LIMIT = 65536                                   # TL3D_TSDF_MAX_WEIGHT
N_LIMIT = 1 << 20                                 # the centroid channel's documented limit of points per voxel
HALF_GATE = 0.5                                   # the max_abs_tsdf with voxels exactly on it
CAM = dict(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5)

MIN_WEIGHTS = (0, MW)
MIN_COUNTS = (0, 1, 2, 3)
GATES = (1.0, HALF_GATE)
# (mode, min_count, min_weight, max_abs_tsdf): centroid mode over everything, TSDF mode over what it reads
SWEEP = [(0, mc, mw, g) for mc in MIN_COUNTS for mw in MIN_WEIGHTS for g in GATES] + [(1, 1, mw, 1.0) for mw in MIN_WEIGHTS]


def sweep_id(p):
    return "mode%d-count%d-weight%d-gate%g" % p if isinstance(p, tuple) else str(p)


# ---- the class tables ---------------------------------------------------------------------------------------------------------
def tsdf_classes(w_limit=W_LIMIT):
    """[(weight, sum)]: weight 0; weights mw-1, mw, 3 and the limit with the sums 0, +-1, +-32767 w, the two integers on either
    side of 0.98 * 32767 w in both signs and +-floor(32767 w / 2) (the mean is exactly +-0.5 when w is even); and weight 50, where
    0.98 * 32767 w is the integer 1605583: a mean exactly on the 0.98 band."""
    out = [(0, 0)]
    for w in (MW - 1, MW, 3, w_limit):
        full, lo98, half = er.QSCALE * w, 98 * er.QSCALE * w // 100, er.QSCALE * w // 2
        assert 100 * lo98 < 98 * er.QSCALE * w < 100 * (lo98 + 1)
        out += [(w, s) for s in (0, 1, -1, full, -full, lo98, -lo98, lo98 + 1, -(lo98 + 1), half, -half)]
    assert 98 * er.QSCALE * 50 == 100 * 1605583
    out += [(50, 1605583), (50, -1605583)]
    assert len(set(out)) == len(out)
    return out


def _pairs_missing(cls, k, axis):
    lo = tuple(slice(0, -1) if q == axis else slice(None) for q in range(3))
    hi = tuple(slice(1, None) if q == axis else slice(None) for q in range(3))
    return np.flatnonzero(np.bincount((cls[lo] * k + cls[hi]).ravel(), minlength=k * k) == 0)


def tsdf_class_volume(dims, seed, k, cover=True):
    """int64 [nx, ny, nz] of class numbers < k, uniformly random, then (cover) repaired until every ordered pair of classes lies
    on an edge of each axis (a missing pair is planted on a random edge; planting may break another pair, so repeat)."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, k, size=dims)
    for _ in range(200 if cover else 0):
        clean = True
        for a in range(3):
            for m in _pairs_missing(cls, k, a):
                clean = False
                v = [int(rng.integers(0, dims[q] - (q == a))) for q in range(3)]
                cls[tuple(v)] = m // k
                v[a] += 1
                cls[tuple(v)] = m % k
        if clean:
            return cls
    assert not cover, "the class volume did not settle"
    return cls


def tsdf_volumes(dims, seed, w_limit=W_LIMIT, cover=True):
    table = np.array(tsdf_classes(w_limit), np.int64)
    cls = tsdf_class_volume(dims, seed, len(table), cover)
    return dict(weight=table[cls, 0], sum=table[cls, 1])


def centroid_volumes(dims, seed):
    """n in {0, 1, 2, 3, 2^20}; each position sum 0, n * 4095 or random between; each colour sum n c + r with r in {0, n - 1}, or 255 n"""
    rng = np.random.default_rng(seed)
    n = np.array([0, 1, 2, 3, N_LIMIT], np.int64)[rng.choice(5, size=dims, p=[0.3, 0.2, 0.15, 0.15, 0.2])]
    vol = dict(n=n)
    for f in ("px", "py", "pz"):
        kind = rng.integers(0, 3, size=dims)
        between = (rng.random(dims) * (n * (er.FRAC_ONE - 1) + 1)).astype(np.int64)
        vol[f] = np.where(kind == 0, 0, np.where(kind == 1, n * (er.FRAC_ONE - 1), np.minimum(between, n * (er.FRAC_ONE - 1))))
    for f in ("cr", "cg", "cb"):
        kind = rng.integers(0, 3, size=dims)
        c = rng.integers(0, 255, size=dims)
        vol[f] = np.where(kind == 0, n * c, np.where(kind == 1, n * c + np.maximum(n - 1, 0), 255 * n))
    return vol


# ---- the grids ------------------------------------------------------------------------------------------------------------------
# name -> geometry.  A: 7.5 extraction chunks of 2048 records.  S: 64 bricks in four states.  B: a block with an offset at which the
# f32 rounding of a position is coarse (1 << 22 voxels of 1 cm: 4 mm per ulp) and a core that the grid overhangs on four faces.
# L: 1025 chunks, one more than the single-block scan has threads.
GEOMETRY = dict(
    A=dict(dims=(24, 16, 40), origin=(-0.37, 0.11, 1.03), voxel=0.01, seed=101),
    S=dict(dims=(32, 32, 32), origin=(0.13, -0.29, 0.61), voxel=0.0125, seed=202),
    B=dict(dims=(32, 32, 32), origin=(-1.7, 0.23, -3.1), voxel=0.01, seed=303, voxel_offset=(16, 4096, 1 << 22),
           core=((8, 0, 8), (24, 32, 32))),
    L=dict(dims=(8, 8, 32776), origin=(0.05, -0.04, -7.3), voxel=0.003, seed=404),
    W=dict(dims=(32, 32, 32), origin=(-0.21, 0.4, 0.77), voxel=0.007, seed=505),          # the whole grid the 8 blocks tile
    P=dict(dims=(16, 16, 16), origin=(-0.16, -0.16, 0.84), voxel=0.02, seed=606),         # the pending-free-space image
)
BRICK_STATES = ("both", "tsdf", "centroid", "neither")


def brick_states(seed):
    """int [4, 4, 4] of BRICK_STATES numbers in which every ordered pair of states meets across a brick face on each axis"""
    for s in itertools.count(seed):
        st = np.random.default_rng(s).integers(0, 4, size=(4, 4, 4))
        if all(len(_pairs_missing(st, 4, a)) == 0 for a in range(3)):
            return st


def _frozen(a):
    if a is not None:
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def grid(name):
    """dict(dims, origin, voxel, voxel_offset, core, vol, tsdf, centroid): volumes and record images, read-only"""
    g = dict(voxel_offset=(0, 0, 0), core=None)
    g.update(GEOMETRY[name])
    dims, seed = g["dims"], g.pop("seed")
    # P gets one more observation on the device: its weights stop one short of the limit; 16^3 is too small to hold every pair
    vol = tsdf_volumes(dims, seed, w_limit=W_LIMIT - (name == "P"), cover=name != "P")
    if name not in ("L", "P"):
        vol.update(centroid_volumes(dims, seed + 1))
    if name == "S":
        g["states"] = brick_states(seed + 2)
        st = np.repeat(np.repeat(np.repeat(g["states"], 8, 0), 8, 1), 8, 2)
        for f in er.FIELDS_TSDF:
            vol[f] = np.where((st == 0) | (st == 1), vol[f], 0)
        for f in er.FIELDS_CENTROID:
            vol[f] = np.where((st == 0) | (st == 2), vol[f], 0)
    tsdf, cen = er.records_from_volumes(vol)
    g.update(vol={f: _frozen(v) for f, v in vol.items()}, tsdf=_frozen(tsdf), centroid=_frozen(cen))
    return g


def reference(g, mode, min_count=1, min_weight=0, max_abs_tsdf=1.0, form="contract", vol=None, **kw):
    kw.setdefault("voxel_offset", g["voxel_offset"])
    kw.setdefault("core", g["core"])
    return er.extract(g["vol"] if vol is None else vol, g["dims"], g["origin"], g["voxel"], mode=mode, min_count=min_count,
                      min_weight=min_weight, max_abs_tsdf=max_abs_tsdf, form=form, **kw)


@functools.lru_cache(maxsize=None)
def swept(name, params, form):
    """the reference of grid `name` at one SWEEP entry, computed once and shared (read-only)"""
    mode, mc, mw, gate = params
    xyz, rgb = reference(grid(name), mode, mc, mw, gate, form=form)
    return _frozen(xyz), _frozen(rgb)


# ---- comparisons ----------------------------------------------------------------------------------------------------------------
def bits(xyz):
    return np.ascontiguousarray(xyz, np.float32).view(np.uint32)


def assert_bit_equal(got, want, what=""):
    """count, order, positions and colours"""
    (gx, gc), (wx, wc) = got, want
    assert gx.shape == wx.shape and gc.shape == wc.shape, (what, gx.shape, wx.shape)
    assert gx.dtype == np.float32 and gc.dtype == np.uint8
    assert np.array_equal(gc, wc), (what, "colours", int((gc != wc).any(axis=1).sum()))
    assert np.array_equal(bits(gx), bits(wx)), (what, "positions", int((bits(gx) != bits(wx)).any(axis=1).sum()))


def assert_within_exact_bound(got, exact, what=""):
    """The bound of the `exact` form: same count, order and colours; every coordinate within 1 float32 ulp (the fp64 expression
    errs by a few 2^-53 relative, so its f32 rounding is the correctly rounded value or that value's neighbour), and at most 1
    coordinate in 1000 not bit-equal.  Returns (coordinates that differ, coordinates)."""
    (gx, gc), (ex, ec) = got, exact
    assert gx.shape == ex.shape, (what, gx.shape, ex.shape)
    assert np.array_equal(gc, ec), (what, "colours")
    d = ulp_diff(gx, ex)
    off, total = int((d != 0).sum()), int(d.size)
    print(f"{what}: {off} of {total} coordinates differ from the exact form, max {int(d.max()) if total else 0} ulp")
    assert total == 0 or d.max() <= 1, (what, int(d.max()))
    assert 1000 * off <= total, (what, off, total)
    return off, total
