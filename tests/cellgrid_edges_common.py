"""The cases of the cell-index edge tests (tests/test_cellgrid_edges_reference_cpu.py, tests/test_gpu_cellgrid_edges.py): clouds
that put the uniform cell index of csrc/cellgrid.h, which the outlier filter, the nearest searches, cloud normals and plane
segmentation share, at the edges of its count / scan / fill and of its shell walk.  No GPU imports.  Not a test.

Every coordinate is a small multiple of 1/64 and every cell size a power of two, so binning has no rounding to argue about: the grid
has floor((max - min) / cell) + 1 cells per axis, the number each case states, and each case also states how many points its
first and its last cell hold.  1024 is the scan's chunk (cell_chunks): the lines have one cell per point and put the cell count
at one cell, one chunk minus one, exactly one, one over, and two chunks plus one.  The end of the last cell comes from
start[ncell], the entry behind the last chunk's scan.

The thin case puts the shell walk (cell_shell_walk) at its edges: a grid of 1 x 2 x 8 cells, four points in the corner cell
(0, 0, 0) and 22 in each of the two cells at z = 7, nothing between.  A walk from the corner with k > 4 finds shells 1 to 6 empty
and its neighbours in shell 7; the one cell along x makes every row's run begin and end in the same cell and puts the end cells of
every interior row outside the grid on both sides; along y one of the two neighbours is always outside."""
import functools

import numpy as np

import nearest_reference as nr
import sor_common as sc

KS = (1, 20, 33)
LINE_NS = (1, 2, 1023, 1024, 1025, 2049)
LAST_FULL_NS = (1024, 1025)
MAX_DROPPED = 0.25               # of the (case, k, ratio) triples, for a reference mean within sc.MARGIN of its threshold


def _line(n):
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n)
    return p


def _last_full(n):
    extra = np.zeros((39, 3))
    extra[:, 0] = n - 1 + np.arange(1, 40) / 64.0
    return np.concatenate([_line(n), extra])


PLANE_NX, PLANE_NY = 33, 32


def _plane():
    x, y = np.meshgrid(np.arange(PLANE_NX), np.arange(PLANE_NY), indexing="xy")        # row y is PLANE_NX consecutive points
    p = np.stack([x, y, 0 * x], -1).reshape(-1, 3).astype(np.float64)
    last = p[-PLANE_NX:] + [0.25, 0, 0]                                                 # the last row of cells, doubled
    return np.concatenate([p, last])


THIN_KS = (20, 33)               # of the filter's k-NN; every one needs shell 7 from the corner
THIN_K_NORMALS = 5               # the corner cell holds 4


def _thin():
    r = np.random.default_rng(0)
    far = []
    for half in (0, 1):                                                                 # the cells (0, half, 7)
        pts = set()
        while len(pts) < 22:
            pts.add((int(r.integers(0, 64)), int(r.integers(0, 64)) + 64 * half, int(r.integers(0, 64)) + 7 * 64))
        far += sorted(pts)
    return np.array([[0, 0, 0], [5, 3, 2], [2, 9, 4], [7, 1, 11]] + far) / 64.0


def _box():
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3) / 8.0
    return g[np.random.default_rng(3).permutation(len(g))[:30]]                         # 30 distinct points of [0, 1)^3


# name -> (points, cell size, cells per axis, points in the first cell, points in the last cell)
_CASES = {
    **{f"line_{n}": ((lambda n=n: _line(n)), 1.0, (n, 1, 1), 1, 1) for n in LINE_NS},
    **{f"last_full_{n}": ((lambda n=n: _last_full(n)), 1.0, (n, 1, 1), 1, 40) for n in LAST_FULL_NS},
    "plane": (_plane, 1.0, (PLANE_NX, PLANE_NY, 1), 1, 2),
    "box": (_box, 64.0, (1, 1, 1), 30, 30),
    "thin": (_thin, 1.0, (1, 2, 8), 4, 22),
}
THIN = "thin"                                                         # has its own tests: not one of CASES
CASES = tuple(c for c in _CASES if c != THIN)
NEAREST_ORDER_CASES = tuple(c for c in CASES if c != "box")          # cases 1-3 of the query-order check


@functools.lru_cache(maxsize=None)
def points(name):
    p = np.ascontiguousarray(_CASES[name][0](), dtype=np.float32)
    assert np.array_equal(p.astype(np.float64), _CASES[name][0]())   # exactly representable
    p.setflags(write=False)
    return p


def cell_size(name):
    return _CASES[name][1]


def dims(name):
    return _CASES[name][2]


def occupancy(name):
    """(points in the first cell, points in the last cell) as the case intends them"""
    return _CASES[name][3:5]


def binned(name):
    """(cells per axis, points per cell in cell order): the rule of cell_grid_make and cell_of restated"""
    p, cell = points(name).astype(np.float64), cell_size(name)
    lo, hi = p.min(axis=0), p.max(axis=0)
    n = (np.floor((hi - lo) / cell) + 1).astype(np.int64)
    c = np.clip(np.floor((p - lo) * (1.0 / cell)), 0, n - 1).astype(np.int64)
    lin = (c[:, 2] * n[1] + c[:, 1]) * n[0] + c[:, 0]
    return tuple(int(v) for v in n), np.bincount(lin, minlength=int(n.prod()))


@functools.lru_cache(maxsize=None)
def ref_means(name, k):
    m = sc.ref_means(points(name), k)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def mask_triples():
    """the (case, k, ratio) triples whose reference means all keep sc.MARGIN from the threshold -- the others are dropped, and at
    most MAX_DROPPED of all may be"""
    every = [(name, k, r) for name in CASES for k in KS for r in sc.RATIOS]
    kept = tuple(t for t in every if sc.margin_count(ref_means(t[0], t[1]), sc.ref_mask(ref_means(t[0], t[1]), t[2])[0]) == 0)
    assert len(every) - len(kept) <= MAX_DROPPED * len(every), (len(every), len(kept))
    return kept


# ---- the nearest searches ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def queries(name):
    """the cloud shifted by (1/4, 1/8, 0), and four points outside its box (N: the cells along x)"""
    t, n = points(name), dims(name)[0]
    out = np.float32([[-3, 0, 0], [n + 5, 2, 0], [0.5, -6, 0.5], [n - 1, 0.25, 9]])
    q = np.ascontiguousarray(np.concatenate([t + np.float32([0.25, 0.125, 0]), out]), dtype=np.float32)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def thin_queries():
    """inside the box: the corner, the empty middle (the nearest target is three shells off, back for one query and on for the
    other) and the far end; and one point outside the box beyond the thin axis, level with the corner"""
    q = np.ascontiguousarray(np.float32([[0.25, 0.125, 0.5], [0.5, 1.5, 0.25], [0.125, 0.75, 3.5], [0.75, 1.25, 4.25], [0.5, 0.5, 7.5],
                                         [3.0, 0.25, 0.125]]))
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def point_ref(name):
    return nr.nearest_points_ref(thin_queries() if name == THIN else queries(name), points(name))


@functools.lru_cache(maxsize=None)
def plane_triangles():
    """the plane's lattice with two triangles per quad (the doubled points are vertices no triangle uses)"""
    idx = np.arange(PLANE_NX * PLANE_NY).reshape(PLANE_NY, PLANE_NX)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    t = np.ascontiguousarray(np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]), dtype=np.uint32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def plane_tri_ref():
    return nr.nearest_triangles_ref(queries("plane"), points("plane"), plane_triangles())


def plane_tri_diag():
    used = points("plane")[np.unique(plane_triangles())].astype(np.float64)
    return float(np.linalg.norm(used.max(axis=0) - used.min(axis=0)))


@functools.lru_cache(maxsize=None)
def dirty_cloud():
    """what leaves a large, dirty scratch behind: 200 000 random targets at cell 0.01 (10^6 cells), a few queries"""
    r = np.random.default_rng(17)
    t = np.ascontiguousarray(r.uniform(0, 1, (200000, 3)), dtype=np.float32)
    q = np.ascontiguousarray(r.uniform(-0.1, 1.1, (500, 3)), dtype=np.float32)
    return q, t, 0.01
