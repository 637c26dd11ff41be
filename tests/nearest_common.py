"""The cases of the nearest-neighbour tests (tests/test_nearest_reference_cpu.py, tests/test_gpu_nearest.py): the smallest shapes
at which the search can go wrong.  Every case is built once, float32, and never modified; the references are cached per case.

EPS_TRI: the largest disagreement, relative to a case's box diagonal, between the two formulations of the point-to-triangle
distance (nearest_reference.tri_dist_matrix in fp64, tri_dist_second in long double) over all triangle cases.  The CPU test
measures and asserts it; the GPU test's tolerance is TRI_TOL_FACTOR x EPS_TRI x diagonal, and tri_gap_ok() asserts that no other
triangle's distance lies between that tolerance and TRI_GAP_FACTOR x EPS_TRI x diagonal above a query's best: what is nearer than
the tolerance is a minimiser too (triangles that share the nearest edge or corner), everything else is three orders away, so a
missed triangle cannot hide under the tolerance."""
import functools

import numpy as np

import nearest_reference as nr

EPS_TRI = 2.5e-16
TRI_TOL_FACTOR = 16
TRI_GAP_FACTOR = 1000
POINT_RTOL = 1e-12

f32 = np.float32


def _a(x):
    return np.ascontiguousarray(np.asarray(x, dtype=f32).reshape(-1, 3))


# ---- points: name -> (query, target, cell_size, dyadic) ---------------------------------------------------------------------------
def _lattice():
    g = np.arange(4) * 0.5
    t = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    t = t[np.random.default_rng(5).permutation(len(t))]
    e = np.stack(np.meshgrid(g[:3] + 0.25, g, g, indexing="ij"), -1).reshape(-1, 3)            # edge centres: 2-way ties
    fc = np.stack(np.meshgrid(g[:3] + 0.25, g[:3] + 0.25, g, indexing="ij"), -1).reshape(-1, 3)  # face centres: 4-way
    cc = np.stack(np.meshgrid(g[:3] + 0.25, g[:3] + 0.25, g[:3] + 0.25, indexing="ij"), -1).reshape(-1, 3)   # cell centres: 8-way
    return np.concatenate([e, e[:, [1, 0, 2]], fc, fc[:, [2, 0, 1]], cc]), t


def _shell_plane(n, seed):
    r = np.random.default_rng(seed)
    v = r.normal(size=(n // 2, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * (1 + 0.01 * r.normal(size=(n // 2, 1)))
    pl = np.concatenate([r.uniform(-1.5, 1.5, size=(n - n // 2, 2)), np.full((n - n // 2, 1), -1.2)], axis=1)
    return np.concatenate([v, pl])


@functools.lru_cache(maxsize=None)
def point_case(name):
    r = np.random.default_rng(sum(map(ord, name)))
    if name == "one_target":
        return _a(r.uniform(-1, 1, (7, 3))), _a([[0.25, -0.5, 1.0]]), 0.5, False
    if name == "one_query":
        return _a([[0.1, 0.2, 0.3]]), _a(r.uniform(-1, 1, (40, 3))), 0.4, False
    if name == "self":
        t = _a(r.uniform(-1, 1, (300, 3)))
        t[100:110] = t[5]                                                    # duplicates: the smallest index of them
        return t, t, 0.25, False
    if name == "five_copies":
        t = _a(r.integers(-8, 8, (60, 3)) / 4.0)
        t[[7, 19, 23, 40, 58]] = [0.125, 0.125, 0.125]
        q = _a([[0.125, 0.125, 0.125], [0.1875, 0.125, 0.125], [0.125, 0.0625, 0.125]])
        return q, t, 0.5, True
    if name == "lattice":
        q, t = _lattice()
        return _a(q), _a(t), 0.5, True
    if name == "outside":
        t = _a(r.uniform(0, 1, (200, 3)))
        diag = 100 * np.sqrt(3.0)
        q = [[1.001, 0.5, 0.5], [-0.001, 0.3, 0.9], [0.5, 0.5, -0.002], [101, 0.5, 0.5], [0.5, -100, 0.5],
             [100, 100, 100], [-diag, -diag, -diag], [30, -40, 0.5]]
        return _a(q), t, 0.125, False
    if name == "l_shape":
        arm = np.arange(0, 10.5, 0.5)
        t = np.concatenate([np.stack([arm, 0 * arm, 0 * arm], 1), np.stack([0 * arm, arm, 0 * arm], 1), [[10, 6.4, 0], [10, 7.05, 0]]])
        q = [[10.5, 6.9, 0], [12, 3, 0], [14, 6, 0.5], [5, 5, 0], [-3, 11, 1]]
        return _a(q), _a(t), 1.0, False
    if name == "boundaries":
        t = _a(np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 3) * 0.5)
        q = [[1.0, 0.75, 0.75], [1.0, 1.0, 0.75], [2.0, 2.0, 2.0], [0, 0, 0], [1.5, 1.5, 1.75], [2.0, 0.25, 2.0]]
        return _a(q), t, 0.5, True
    if name == "plane":
        t = np.concatenate([r.uniform(-1, 1, (150, 2)), np.full((150, 1), 0.5)], 1)
        return _a(r.uniform(-1.5, 1.5, (50, 3))), _a(t), 0.2, False
    if name == "line":
        t = np.concatenate([np.full((80, 2), 0.25), r.uniform(-2, 2, (80, 1))], 1)
        return _a(r.uniform(-2.5, 2.5, (40, 3))), _a(t), 0.1, False
    if name == "all_equal":
        return _a(r.uniform(-1, 1, (20, 3))), _a(np.full((30, 3), 0.375)), 0.1, False
    if name == "lone_point":
        t = np.concatenate([r.uniform(0, 0.2, (400, 3)), [[5.0, 0.1, 0.1]]])
        q = [[3.0, 0.1, 0.1], [2.7, 0.15, 0.05], [0.1, 0.1, 0.1], [5.5, 0.1, 0.1]]                # the first two: the lone point, 50 cells off
        return _a(q), _a(t), 0.1, False
    if name == "spread":                                                     # at 1/8 of its cell the grid would have 640^3 cells: it doubles
        return _a(r.uniform(0.5, 7.5, (100, 3))), _a(r.uniform(0, 8, (2000, 3))), 0.1, False
    if name == "shell_plane":
        return _a(r.uniform(-1.8, 1.8, (3000, 3))), _a(_shell_plane(5000, 11)), 0.08, False
    if name.startswith("nq"):
        return _a(r.uniform(-1.2, 1.2, (int(name[2:]), 3))), _a(_shell_plane(700, 13)), 0.2, False
    raise KeyError(name)


POINT_CASES = ["one_target", "one_query", "self", "five_copies", "lattice", "outside", "l_shape", "boundaries", "plane", "line",
               "all_equal", "lone_point", "spread", "shell_plane", "nq63", "nq64", "nq65", "nq257"]
CELL_FACTORS = [0.125, 1.0, 64.0, None]                     # None: the library's default cell


@functools.lru_cache(maxsize=None)
def point_ref(name):
    q, t, _, _ = point_case(name)
    return nr.nearest_points_ref(q, t)


# ---- triangles: name -> (query, xyz, tris, cell_size, dyadic) ---------------------------------------------------------------------
def _icosphere(levels):
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.array(x, float) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                w = v[i] + v[j]
                v.append(w / np.linalg.norm(w))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f)


def _cube():
    v = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], float)
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return v, np.array(f)


def _heightfield(n, seed):
    r = np.random.default_rng(seed)
    g = np.arange(n) / (n - 1.0)
    x, y = np.meshgrid(g, g, indexing="ij")
    z = 0.1 * np.sin(5 * x) * np.cos(4 * y) + 0.01 * r.normal(size=x.shape)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    return np.stack([x, y, z], -1).reshape(-1, 3), np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])


BIG_TRI = [[0, 0, 0], [200, 0, 0], [0, 200, 16]]


def _small_sheet():
    g = np.arange(0, 51) * 0.5
    x, y = np.meshgrid(g, g * 2, indexing="ij")                             # 51 x 51 vertices -> 5000 quads -> 10000 triangles
    v = np.stack([x + 210, y, 0 * x - 5], -1).reshape(-1, 3)
    idx = np.arange(51 * 51).reshape(51, 51)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    return v, np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])


@functools.lru_cache(maxsize=None)
def tri_case(name):
    r = np.random.default_rng(sum(map(ord, name)))
    t32 = lambda t: np.ascontiguousarray(np.asarray(t, dtype=np.uint32).reshape(-1, 3))     # noqa: E731
    if name == "regions":
        v = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
        q = []
        for z in (1.0, -1.0, 0.0):                                           # above, below, in the plane
            q += [[1, 1, z], [-1, -1, z], [5, -1, z], [-1, 5, z], [2, -1, z], [-1, 2, z], [3, 3, z]]      # interior, 3 corners, 3 edges
        q += [[2, 0, 0], [2, 2, 0], [0, 1, 0], [4, 0, 0], [0, 0, 0], [0, 4, 0]]                       # on the edges, at the corners: d = 0
        return _a(q), _a(v), t32([[0, 1, 2]]), 1.0, True
    if name == "degenerate":
        v = [[0, 0, 0], [1, 0, 0], [3, 0, 0], [0, 2, 2], [2, 2, 2], [-4, -4, 1]]
        t = [[0, 1, 2], [3, 3, 4], [5, 5, 5], [2, 0, 1], [3, 4, 3]]          # collinear, (a, a, b), a point, and two re-orderings
        q = [[2, 1, 0], [-1, 1, 0], [4, 0, 1], [1, 2, 3], [-4, -4, 2], [-3, -3, 1], [1.5, 0.5, 0.25], [3, 2, 2], [1, 3, 2]]
        return _a(q), _a(v), t32(t), 1.0, True
    if name == "big":
        q = [[50, 50, 3], [60.5, 40.25, -2], [100, 20, 9], [30, 120, 6.5], [90, 90, 1]]
        return _a(q), _a(BIG_TRI), t32([[0, 1, 2]]), 1.0, False
    if name == "big_and_small":
        sv, st = _small_sheet()
        v = np.concatenate([np.array(BIG_TRI, float), sv])
        t = np.concatenate([[[0, 1, 2]], st + 3])
        q = [[50, 50, 3], [60.5, 40.25, -2], [220.3, 10.2, -4], [215.1, 40.7, -6.5], [205, 30, -1], [100, 20, 9], [230.2, 49.1, -5.5]]
        return _a(q), _a(v), t32(t), 1.0, False
    if name == "cube":
        v, t = _cube()
        q = np.concatenate([r.uniform(0.05, 0.95, (20, 3)), r.uniform(-1, 2, (40, 3)),
                            [[0.5, 0.5, 1.5], [0.25, 0.25, 1], [1, 0.5, 0.5], [0, 0, 0], [0.5, 0.5, 0.5], [1.5, 1.5, 0.5], [2, 2, 2]]])
        return _a(q), _a(v), t32(t), 0.5, False
    if name == "cube_ties":                                                  # dyadic: above the shared diagonal of a face, at the centre
        v, t = _cube()
        q = [[0.5, 0.5, 1.5], [0.25, 0.25, 1.25], [0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, -0.5, 0.5], [2, 2, 0.5]]
        return _a(q), _a(v), t32(t), 0.5, True
    if name == "icosphere":
        v, t = _icosphere(2)
        q = np.concatenate([r.uniform(-0.5, 0.5, (40, 3)), r.uniform(-2, 2, (60, 3)), v[::7], v[t[::9]].mean(axis=1)])
        return _a(q), _a(v), t32(t), 0.25, False
    if name == "heightfield":
        v, t = _heightfield(32, 3)
        q = np.concatenate([r.uniform(-0.2, 1.2, (2000, 2)), r.uniform(-0.4, 0.4, (2000, 1))], 1)
        return _a(q), _a(v), t32(t), 1 / 31.0, False
    raise KeyError(name)


TRI_CASES = ["regions", "degenerate", "big", "big_and_small", "cube", "cube_ties", "icosphere", "heightfield"]


def tri_diag(name):
    _, v, t, _, _ = tri_case(name)
    used = v[np.unique(t)].astype(np.float64)
    return float(np.linalg.norm(used.max(axis=0) - used.min(axis=0)))


@functools.lru_cache(maxsize=None)
def tri_ref(name):
    q, v, t, _, _ = tri_case(name)
    return nr.nearest_triangles_ref(q, v, t)


def tri_tol(name):
    return TRI_TOL_FACTOR * EPS_TRI * tri_diag(name)


def tri_gap_ok(name):
    """no triangle's reference distance lies in (tolerance, TRI_GAP_FACTOR x EPS_TRI x diagonal] above a query's best"""
    d, _, m = tri_ref(name)
    above = m - d[:, None]
    lo, hi = tri_tol(name), TRI_GAP_FACTOR * EPS_TRI * tri_diag(name)
    return not np.any((above > lo) & (above <= hi))
