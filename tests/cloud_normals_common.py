"""Shared by the cloud-normal tests (CPU and GPU): the clouds at the edges of tl3d_estimate_normals (kernels_normals.hip; the
definition is in include/tl3d.h), two fp64 references that share no code, and the bars.  No GPU imports.  Not a test.

ref    scipy's k-d tree for the neighbours, the centred covariance, numpy.linalg.eigh.
brute  all pairwise d^2, a stable sort (so the order is (d^2, index): the one that implements the tie rule), the covariance summed
       member by member, lambda0 from eigvalsh and the normal as the largest cross product of two rows of C - lambda0 I.

The bars are derived, not measured.  Kernel and references work in fp64 from differences of float32 coordinates, which are exact in
fp64.  Sums of at most 64 terms in another association move C's entries by at most about 64 ulp of |C| ~ lambda2; a backward-stable
eigen-solver adds a few more; by Davis-Kahan sin(angle) <= 2 |dC| / (lambda1 - lambda0).  So, per point,
    sin(angle between got and ref, up to sign when unoriented) <= 2^-22 + 1024 * 2^-52 * lambda2 / (lambda1 - lambda0)
with 2^-22 the float32 rounding of three components and lambda from the reference; a wrong or missing neighbour moves a normal by
many orders more.  Curvature: |got - ref| <= 2^-22 + 1024 * 2^-52.  Length: | |n| - 1 | <= 2^-22.  A point leaves the angle check
only when its bound exceeds 1e-3, i.e. (lambda1 - lambda0) / lambda2 < 2.3e-10; none of the random cases has such a point (asserted
on the reference)."""
import functools

import numpy as np

import sor_common as sc

F32 = 2.0 ** -22
EPS = 1024 * 2.0 ** -52
EXCLUDE = 1e-3
K_RANDOM = (3, 4, 30, 32, 33, 63, 64)          # both instantiations of the kernel (32 and 64 list entries) and their edge
CELLS = (0.005, 0.05, 0.3, 10.0)

# name -> (points, cell_size); the generators are those of the outlier filter's tests
_RANDOM = {
    "ring": (lambda: sc.ring(0, 4000, 40), 0.02),
    "k_edges": (lambda: sc.points("k_edges"), 0.05),
    "slab": (lambda: sc.points("slab"), 0.02),
    "offset": (lambda: sc.points("offset"), 0.02),          # coordinates near 500
    "coarse": (lambda: sc.points("coarse"), 10.0),          # one cell
    "fine": (lambda: sc.points("fine"), 0.01),              # many empty shells
    "tiny_n3": (lambda: sc.cube(2, 3), 0.1),                # k clamped to n
    "tiny_n4": (lambda: sc.cube(2, 4), 0.1),
    "tiny_n19": (lambda: sc.cube(2, 19), 0.1),
}
RANDOM = tuple(_RANDOM)
RANDOM_K = tuple((name, k) for name in RANDOM for k in K_RANDOM)


def _plane_lattice():
    """20 x 20 points at spacing 0.25 in the plane z = 0.25: every neighbourhood lies in the plane, whatever the ties do"""
    g = np.stack(np.meshgrid(np.arange(20), np.arange(20), indexing="ij"), axis=-1).reshape(-1, 2)
    return np.concatenate([g * 0.25, np.full((len(g), 1), 0.25)], axis=1).astype(np.float32)


TIE4 = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
RADIUS6 = np.float32([[0, 0, 0], [0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, 4]])

_OTHER = {
    "tiny_n1": (lambda: sc.cube(2, 1), 0.1),
    "tiny_n2": (lambda: sc.cube(2, 2), 0.1),
    "same": (lambda: sc.points("same"), 0.1),
    "dups": (lambda: sc.points("dups"), 0.05),
    "plane_lattice": (_plane_lattice, 0.25),
    "line": (lambda: sc.points("line"), 0.02),
    "lattice": (lambda: sc.points("lattice"), 0.25),
    "tie4": (lambda: TIE4, 0.5),
    "tie4_reversed": (lambda: TIE4[::-1], 0.5),
    "radius6": (lambda: RADIUS6, 0.3),
}


def case_id(v):
    return v if isinstance(v, str) else f"k{v}"


@functools.lru_cache(maxsize=None)
def points(name):
    gen = _RANDOM[name][0] if name in _RANDOM else _OTHER[name][0]
    p = np.ascontiguousarray(gen(), dtype=np.float32)
    p.setflags(write=False)
    return p


def cell_size(name):
    return (_RANDOM[name] if name in _RANDOM else _OTHER[name])[1]


def ring_viewpoints():
    """8 viewpoints on a circle of radius 2 around the ring's axis (y), outside the cylinder of radius 0.5"""
    a = np.arange(8) * (2 * np.pi / 8) + 0.1
    return np.stack([2.0 * np.cos(a), np.zeros(8), 2.0 * np.sin(a)], axis=1)


# ---- references --------------------------------------------------------------------------------------------------------------------
class Result:
    """normals fp64 [n,3] (zero rows where degenerate), curvature fp64 [n], lam fp64 [n,3] ascending, members [n], degenerate mask"""
    def __init__(self, normals, curvature, lam, members, degenerate):
        self.normals, self.curvature, self.lam, self.members, self.degenerate = normals, curvature, lam, members, degenerate
        for a in (normals, curvature, lam, members, degenerate):
            a.setflags(write=False)


def _orient(normals, p, viewpoints):
    """towards the nearest viewpoint, the smaller index on a tie (argmin takes the first); n . (c - p) == 0 stays"""
    if viewpoints is None or len(viewpoints) == 0:
        return normals
    c = np.asarray(viewpoints, np.float64).reshape(-1, 3)
    d = c[None, :, :] - p[:, None, :]
    to = d[np.arange(len(p)), (d * d).sum(axis=-1).argmin(axis=1)]
    flip = (normals * to).sum(axis=1) < 0
    return np.where(flip[:, None], -normals, normals)


def _finish(normals, lam, members, p, viewpoints):
    degenerate = (members < 3) | (lam[:, 2] == 0)
    tot = lam.sum(axis=1)
    curvature = np.where(degenerate | (tot == 0), 0.0, lam[:, 0] / np.where(tot == 0, 1.0, tot))
    normals = np.where(degenerate[:, None], 0.0, normals)
    return Result(_orient(normals, p, viewpoints), curvature, lam, members, degenerate)


def ref(p32, k, max_radius=0.0, viewpoints=None):
    from scipy.spatial import cKDTree
    p = np.asarray(p32, dtype=np.float64)
    n = len(p)
    k = min(k, n)
    _, idx = cKDTree(p).query(p, k=k)
    e = p[idx.reshape(n, k)] - p[:, None, :]
    w = np.ones((n, k))
    if max_radius > 0:
        w = ((e * e).sum(axis=-1) <= max_radius * max_radius).astype(np.float64)
    members = w.sum(axis=1).astype(np.int64)
    m = (e * w[:, :, None]).sum(axis=1) / np.maximum(members, 1)[:, None]
    d = (e - m[:, None, :]) * w[:, :, None]
    lam, vec = np.linalg.eigh(np.einsum("nki,nkj->nij", d, d))
    return _finish(vec[:, :, 0], lam, members, p, viewpoints)


def brute_neighbours(p32, kmax=64, chunk=512, rows=None):
    """index [n, min(kmax, n)] of every point's nearest neighbours in the order (d^2, index), and their d^2.  No tree: every pair.
    Per row the candidates are cut down with a partition first (m of them, in index order) and sorted stably; where the cut could
    have split a tie that reaches into the first kmax, the whole row block is sorted instead.  rows: for these points only."""
    p = np.asarray(p32, dtype=np.float64)
    n = len(p)
    q = p if rows is None else p[rows]
    kk, m = min(kmax, n), min(n, kmax + 32)
    idx, d2o = np.empty((len(q), kk), np.int64), np.empty((len(q), kk), np.float64)
    for s in range(0, len(q), chunk):
        d = q[s:s + chunk, None, :] - p[None, :, :]
        d2 = (d * d).sum(axis=-1)
        ri = np.arange(len(d2))[:, None]
        cand = np.sort(np.argpartition(d2, m - 1, axis=1)[:, :m], axis=1) if m < n else np.broadcast_to(np.arange(n), d2.shape)
        o = np.argsort(d2[ri, cand], axis=1, kind="stable")
        order, sd = cand[ri, o], d2[ri, cand][ri, o]
        if m < n and not np.all(sd[:, kk - 1] < sd[:, m - 1]):
            order = np.argsort(d2, axis=1, kind="stable")
            sd = d2[ri, order]
        idx[s:s + chunk], d2o[s:s + chunk] = order[:, :kk], sd[:, :kk]
    return idx, d2o


def brute(p32, k, max_radius=0.0, viewpoints=None, neighbours=None, rows=None):
    """rows: the result for these points only (their neighbours are still taken from the whole cloud)"""
    cloud = np.asarray(p32, dtype=np.float64)
    k = min(k, len(cloud))
    idx, d2 = neighbours if neighbours is not None else brute_neighbours(cloud, k, rows=rows)
    idx, d2 = idx[:, :k], d2[:, :k]
    p = cloud if rows is None else cloud[rows]
    n = len(p)
    inside = d2 <= max_radius * max_radius if max_radius > 0 else np.ones_like(d2, dtype=bool)
    members = inside.sum(axis=1)
    tot = np.zeros((n, 3))
    for j in range(k):                                     # member by member, in (d^2, index) order
        tot += np.where(inside[:, j, None], cloud[idx[:, j]] - p, 0.0)
    m = tot / np.maximum(members, 1)[:, None]
    cov = np.zeros((n, 3, 3))
    for j in range(k):
        d = np.where(inside[:, j, None], cloud[idx[:, j]] - p - m, 0.0)
        cov += d[:, :, None] * d[:, None, :]
    lam = np.linalg.eigvalsh(cov)
    mat = cov - lam[:, 0, None, None] * np.eye(3)
    cr = np.stack([np.cross(mat[:, 0], mat[:, 1]), np.cross(mat[:, 0], mat[:, 2]), np.cross(mat[:, 1], mat[:, 2])], axis=1)
    nrm = np.linalg.norm(cr, axis=2)
    best = cr[np.arange(n), nrm.argmax(axis=1)]
    normals = best / np.maximum(nrm.max(axis=1), 1e-300)[:, None]
    return _finish(normals, lam, members, p, viewpoints)


@functools.lru_cache(maxsize=None)
def case_ref(name, k):
    return ref(points(name), k)


@functools.lru_cache(maxsize=None)
def case_neighbours(name):
    return brute_neighbours(points(name))


# ---- the bars ----------------------------------------------------------------------------------------------------------------------
def angle_bound(lam):
    gap = lam[:, 1] - lam[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(gap > 0, F32 + EPS * lam[:, 2] / np.where(gap > 0, gap, 1.0), np.inf)


def excluded(r):
    """points of a reference result that leave the angle check: not degenerate, and a bound above EXCLUDE"""
    return ~r.degenerate & (angle_bound(r.lam) > EXCLUDE)


def sin_angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(np.cross(a, b), axis=1)


def check(got_normals, got_curvature, r, oriented, what, allow_excluded=False):
    """Holds a result (normals [n,3], curvature [n] or None) to the reference result r by the bars above; prints the figures first."""
    g = np.asarray(got_normals, np.float64)
    assert g.shape == r.normals.shape, f"{what}: shape {g.shape}"
    deg = r.degenerate
    assert np.all(g[deg] == 0), f"{what}: a degenerate point has a normal"
    assert np.all(np.any(g[~deg] != 0, axis=1)), f"{what}: a zero normal where the reference has one"
    length = np.abs(np.linalg.norm(g[~deg], axis=1) - 1.0)
    bound = angle_bound(r.lam)
    out = excluded(r)
    tested = ~deg & ~out
    s = sin_angle(g[tested], r.normals[tested])
    worst = float((s / bound[tested]).max()) if s.size else 0.0
    cerr = np.abs(np.asarray(got_curvature, np.float64) - r.curvature) if got_curvature is not None else np.zeros(1)
    print(f"{what}: n={len(g)} degenerate {int(deg.sum())} excluded {int(out.sum())} max |len-1| {length.max() if length.size else 0.0:.3g} "
          f"max sin {s.max() if s.size else 0.0:.3g} max sin/bound {worst:.3g} max curvature err {cerr.max():.3g}")
    assert allow_excluded or not out.any(), f"{what}: {int(out.sum())} points leave the angle check"
    assert np.all(length <= F32), f"{what}: {int((length > F32).sum())} normals are not unit"
    assert np.all(s <= bound[tested]), f"{what}: {int((s > bound[tested]).sum())} normals off, worst at point {int(np.flatnonzero(tested)[(s / bound[tested]).argmax()])}"
    if oriented:
        dots = (g[tested] * r.normals[tested]).sum(axis=1)
        assert np.all(dots > 0), f"{what}: {int((dots <= 0).sum())} normals point the other way"
    if got_curvature is not None:
        assert np.all(cerr <= F32 + EPS), f"{what}: {int((cerr > F32 + EPS).sum())} curvatures off"
        assert np.all(np.asarray(got_curvature)[deg] == 0), f"{what}: a degenerate point has a curvature"
