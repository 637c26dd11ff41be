"""Shared by the outlier-filter tests (CPU and GPU): the point clouds at the edges of the filter's k-NN (kernels_sor.hip), two
fp64 references of the per-point mean neighbour distance that share no code, and the mask rule.  No GPU imports.  Not a test.

Every reference is fp64 and starts from the float32 points the kernel is given: differences of float32 values are exact in
fp64, so kernel and references differ only in the rounding of the squares' sum, the square roots and the sum of at most 64 of
them."""
import functools

import numpy as np

RATIOS = (2.0, 0.0)              # the pipeline's default; and 0: the threshold is mu, roughly half the points on each side
MARGIN = 1e-9                    # no reference mean may lie this close (relative) to its threshold: see margin_count
CELL_CAP = 2.0 ** 27             # the filter doubles its cell until the grid has at most this many cells (sor_mean_distance)


# ---- generators -----------------------------------------------------------------------------------------------------------------
def cube(seed, n, side=(1.0, 1.0, 1.0), cluster=0):
    """n uniform points in a box of the given sides; cluster > 0 appends a tight normal blob (sigma = 1 % of the side) at its centre"""
    rng = np.random.default_rng(seed)
    side = np.asarray(side, np.float64)
    p = rng.uniform(0, 1, (n, 3)) * side
    if cluster > 0:
        p = np.vstack([p, rng.normal(0.5, 0.01, (cluster, 3)) * side])
    return p.astype(np.float32)


def ring(seed, n, outliers):
    """the cloud of tests/test_gpu_dense_api.py (_cloud, same draws in the same order): a noisy cylinder and uniform outliers"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 2 * np.pi, n)
    b = rng.uniform(-0.4, 0.4, n)
    pts = np.stack([0.5 * np.cos(a), b, 0.5 * np.sin(a)], 1) + rng.normal(0, 0.0015, (n, 3))
    out = rng.uniform(-0.9, 0.9, (outliers, 3))
    return np.vstack([pts, out]).astype(np.float32)


LATTICE_DIMS, LATTICE_STEP = (12, 10, 8), 0.25


def _lattice():
    g = np.stack(np.meshgrid(*[np.arange(d) for d in LATTICE_DIMS], indexing="ij"), axis=-1).reshape(-1, 3)
    return (g * LATTICE_STEP).astype(np.float32)


def lattice_interior():
    """mask of the lattice points with all 26 neighbours: 0 < index < 11, 9, 7"""
    g = np.stack(np.meshgrid(*[np.arange(d) for d in LATTICE_DIMS], indexing="ij"), axis=-1).reshape(-1, 3)
    return np.all((g > 0) & (g < np.array(LATTICE_DIMS) - 1), axis=1)


# mean distance of an interior lattice point: itself, 6 face neighbours (k = 7); + 12 edge and 8 corner neighbours (k = 27)
LATTICE_KNOWN = {7: 6 * LATTICE_STEP / 7, 27: (6 + 12 * np.sqrt(2.0) + 8 * np.sqrt(3.0)) * LATTICE_STEP / 27}


def _flat(seed, n, axes):
    p = cube(seed, n)
    p[:, axes] = np.float32(0.3)
    return p


def _dups():
    p = cube(9, 3000)
    return np.vstack([p, np.repeat(p[0:1], 24, axis=0), np.repeat(p[1:2], 9, axis=0)])      # 25 x point 0, 10 x point 1


def _offset():
    return (cube(10, 5000, cluster=200).astype(np.float64) + np.array([500.0, -300.0, 40.0])).astype(np.float32)


# ---- cases: name -> (points, k list, cell_size) -----------------------------------------------------------------------------------
# doubling: 100 000 points in the unit cube at a 0.4 mm cell.  sor_mean_distance takes floor(extent / cell) + 1 cells per axis and
# doubles the cell while their product is above 2^27 = 1.34e8.  The extent is just under 1, so: 0.0004 -> 2500^3 = 1.6e10,
# 0.0008 -> 1250^3 = 2.0e9, 0.0016 -> 625^3 = 2.4e8, 0.0032 -> 313^3 = 3.1e7: three doublings (final_cell recomputes this).
_CASES = {
    "ring": (lambda: ring(0, 40000, 400), (20,), 0.02),
    "k_edges": (lambda: cube(1, 3000, cluster=300), (1, 2, 31, 32, 33, 63, 64), 0.05),
    **{f"tiny_n{n}": ((lambda n=n: cube(2, n)), (20,), 0.1) for n in (1, 2, 3, 19, 20, 21)},            # k clamped to n, k = n, k = n - 1
    "same": (lambda: np.tile(np.float32([0.25, -1.5, 3.0]), (30, 1)), (20,), 0.1),
    "lattice": (_lattice, (7, 27), 0.25),                                                           # points sit on cell faces
    "plane": (lambda: _flat(3, 5000, [2]), (20,), 0.02),                                            # nz = 1
    "line": (lambda: _flat(4, 2000, [1, 2]), (20,), 0.02),                                          # ny = nz = 1
    "slab": (lambda: cube(5, 6000, side=(4.0, 0.2, 0.05)), (20,), 0.02),
    "fine": (lambda: cube(6, 1500), (20,), 0.01),                                                   # ~15 shells of mostly empty cells
    "coarse": (lambda: cube(7, 4000), (20, 64), 10.0),                                              # a single cell
    "doubling": (lambda: cube(8, 100000), (20,), 0.0004),
    "dups": (_dups, (20,), 0.05),
    "offset": (_offset, (20,), 0.02),
}
CASES = tuple(_CASES)
CASE_K = tuple((name, k) for name in CASES for k in _CASES[name][1])
BRUTE_MAX_N = 8000               # the O(n^2) second formulation runs on every case up to this size


def case_id(v):
    return v if isinstance(v, str) else (f"k{v}" if isinstance(v, int) else f"ratio{v}")


@functools.lru_cache(maxsize=None)
def points(name):
    p = np.ascontiguousarray(_CASES[name][0](), dtype=np.float32)
    p.setflags(write=False)
    return p


def ks(name):
    return _CASES[name][1]


def cell_size(name):
    return _CASES[name][2]


# ---- references --------------------------------------------------------------------------------------------------------------------
def ref_means(p32, k):
    """per point the mean distance to its min(k, n) nearest neighbours, itself included: scipy's k-d tree on the fp64 points"""
    from scipy.spatial import cKDTree
    p = np.asarray(p32, dtype=np.float64)
    n = len(p)
    k = min(k, n)
    dist, _ = cKDTree(p).query(p, k=k)
    return dist.reshape(n, k).mean(axis=1)


def brute_means(p32, k, chunk=256):
    """the same quantity with no tree: all squared differences, sorted, the square root of the first k, averaged"""
    p = np.asarray(p32, dtype=np.float64)
    n = len(p)
    k = min(k, n)
    out = np.empty(n, np.float64)
    for s in range(0, n, chunk):
        d = p[s:s + chunk, None, :] - p[None, :, :]
        d2 = (d * d).sum(axis=-1)
        d2.sort(axis=1)
        out[s:s + chunk] = np.sqrt(d2[:, :k]).mean(axis=1)
    return out


def ref_mask(means, ratio):
    """(threshold, keep mask) by the rule of oracle.ref_numpy.statistical_outlier_open3d: valid = mean > 0; at most one valid
    point: keep the valid ones (threshold +inf); else mu and the Bessel-corrected sigma over the valid points, keep
    0 < mean < mu + ratio * sigma"""
    ok = means > 0
    m = int(ok.sum())
    if m <= 1:
        return np.inf, ok
    mu = means[ok].sum() / m
    sigma = np.sqrt(((means[ok] - mu) ** 2).sum() / (m - 1))
    thr = mu + ratio * sigma
    return thr, ok & (means < thr)


def margin_count(means, thr):
    """points whose mean lies within MARGIN (relative) of the threshold.  The kernel's means agree with the reference's to 1e-12
    and its mu and sigma are sums of the same numbers in another order, so its threshold agrees to ~1e-12 as well: with no
    point inside 1e-9 the two masks are identical, not merely close.  An infinite threshold (<= 1 valid point) has no margin."""
    if not np.isfinite(thr):
        return 0
    return int((np.abs(means - thr) <= MARGIN * thr).sum())


@functools.lru_cache(maxsize=None)
def case_ref_means(name, k):
    m = ref_means(points(name), k)
    m.setflags(write=False)
    return m


def final_cell(p32, cell):
    """(cell, cells per axis, doublings) the filter ends with: the rule of sor_mean_distance restated"""
    lo, hi = np.asarray(p32).min(axis=0).astype(np.float64), np.asarray(p32).max(axis=0).astype(np.float64)
    doublings = 0
    while True:
        dims = np.floor((hi - lo) / cell) + 1
        if dims[0] * dims[1] * dims[2] <= CELL_CAP and np.all(dims < 2e9):
            return cell, tuple(int(d) for d in dims), doublings
        cell *= 2.0
        doublings += 1
