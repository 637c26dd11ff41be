"""Two numpy / scipy formulations of tl3d_segment_planes (the definition is in include/tl3d.h) that share no
code with each other or with the kernels.  No GPU imports.  Not a test.

tree   scipy's k-d tree for the pairs within a slightly larger radius, the exact fp64 predicate on them, scipy's
       connected_components, the label of a component = its smallest index, the moments in Python integers, the plane from the
       integer sums by the definition's fp64 sequence and numpy.linalg.eigh.
grow   plain breadth-first region growing from the smallest unvisited index over a brute-force neighbour test (every point against
       all others), the plane from a two-pass centred covariance of the fp64 coordinates.  For small clouds.

Both evaluate the link predicate as the definition writes it: fp64 on the f32 inputs converted exactly, plain products and sums in
x, y, z order (numpy's elementwise operations round once each and fuse nothing)."""
from fractions import Fraction

import numpy as np

Q = 2.0 ** 20
PLANE_DTYPE = np.dtype([("normal", np.float64, (3,)), ("d", np.float64), ("centroid", np.float64, (3,)), ("rms", np.float64),
                        ("count", np.int64), ("seed", np.int64)])


class Params:
    def __init__(self, radius, min_cos, max_offset, max_curvature=0.0, min_points=3, max_rms=0.0, signed_normals=True):
        self.radius, self.min_cos, self.max_offset = float(radius), float(min_cos), float(max_offset)
        self.max_curvature, self.min_points, self.max_rms = float(max_curvature), int(min_points), float(max_rms)
        self.signed_normals = bool(signed_normals)

    def replace(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Params(**d)


class Result:
    """plane_id int32 [n]; counts (eligible, regions, candidates, planes); planes: PLANE_DTYPE records in ascending seed; label
    int64 [n] (-1: not eligible); sums: per accepted plane (count, [3], [6], [3]) as Python integers; lam: per accepted plane"""
    def __init__(self, plane_id, counts, planes, label, sums, lam):
        self.plane_id, self.counts, self.planes, self.label, self.sums, self.lam = plane_id, tuple(counts), planes, label, sums, lam
        for a in (plane_id, planes, label):
            a.setflags(write=False)


def eligible(nrm32, curv32, prm):
    n = np.asarray(nrm32, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        l2 = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
        ok = np.isfinite(l2) & (l2 > 0)
        if curv32 is not None and prm.max_curvature > 0:
            ok &= np.asarray(curv32, np.float32).astype(np.float64) <= prm.max_curvature
    return ok


def linked(p, n, i, j, prm):
    """the predicate for the index arrays i, j (p, n: fp64 copies of the f32 inputs), as the thread of the larger index evaluates it"""
    d = p[j] - p[i]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    s = n[i, 0] * n[j, 0] + n[i, 1] * n[j, 1] + n[i, 2] * n[j, 2]
    if not prm.signed_normals:
        s = np.abs(s)
    oi = np.abs(n[i, 0] * d[:, 0] + n[i, 1] * d[:, 1] + n[i, 2] * d[:, 2])
    oj = np.abs(n[j, 0] * -d[:, 0] + n[j, 1] * -d[:, 1] + n[j, 2] * -d[:, 2])
    return (d2 <= prm.radius * prm.radius) & (s >= prm.min_cos) & (oi <= prm.max_offset) & (oj <= prm.max_offset)


def quantise(x32):
    return np.rint(np.asarray(x32, np.float32).astype(np.float64) * Q).astype(np.int64)       # rint: half to even, as llrint


def integer_sums(p32, n32, members, seed):
    """(count, sum e [3], sum e_a e_b [xx, yy, zz, xy, xz, yz], sum N [3]) in Python integers"""
    q = quantise(p32)
    e = (q[members] - q[seed]).astype(object)
    nn = np.rint(np.clip(np.asarray(n32, np.float32)[members].astype(np.float64) * Q, -2.0 ** 31, 2.0 ** 31)).astype(np.int64).astype(object)
    se = [int(e[:, a].sum()) for a in range(3)]
    see = [int((e[:, a] * e[:, b]).sum()) for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
    return len(members), se, see, [int(nn[:, a].sum()) for a in range(3)]


def _dbl128(v):
    """the kernel's conversion of a 128-bit integer: the high and the low 64 bits converted, then one sum"""
    m = abs(v)
    d = float(m >> 64) * 18446744073709551616.0 + float(m & ((1 << 64) - 1))
    return -d if v < 0 else d


def plane_from_sums(sums, qseed):
    """The definition's fp64 sequence with numpy's eigh in the place of the Jacobi sweeps: (normal, d, centroid, rms, lam)"""
    cnt, se, see, sn = sums
    c = float(cnt)
    s = [float(v) for v in se]
    cov = [_dbl128(see[k]) - s[a] * s[b] / c for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)))]
    mat = np.array([[cov[0], cov[3], cov[4]], [cov[3], cov[1], cov[5]], [cov[4], cov[5], cov[2]]])
    lam, vec = np.linalg.eigh(mat)
    nv = vec[:, 0] / np.linalg.norm(vec[:, 0])
    if nv[0] * float(sn[0]) + nv[1] * float(sn[1]) + nv[2] * float(sn[2]) < 0:
        nv = -nv
    cen = np.array([(float(qseed[a]) + s[a] / c) / Q for a in range(3)])
    rms = np.sqrt(max(lam[0], 0.0) / c) / Q
    return nv, float(nv[0] * cen[0] + nv[1] * cen[1] + nv[2] * cen[2]), cen, float(rms), lam


def exact_covariance(sums):
    """count * C as exact integers (3x3 nested lists): count * sum e_a e_b - sum e_a * sum e_b"""
    cnt, se, see, _ = sums
    idx = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (0, 2): 4, (1, 2): 5}
    return [[cnt * see[idx[(min(a, b), max(a, b))]] - se[a] * se[b] for b in range(3)] for a in range(3)]


def plane_extended(sums, qseed, digits=60):
    """(normal, d, centroid, rms, lam) from the exact sums in extended precision: mpmath's symmetric eigen-solver at `digits`
    decimal digits on the exactly known covariance when mpmath is there; otherwise numpy.longdouble for everything but the
    eigen-decomposition, which numpy has in fp64 only (its error, a few ulp of |C|, is then part of what the bar allows)."""
    cnt, se, _, sn = sums
    cc = exact_covariance(sums)
    try:
        import mpmath as mp
    except ImportError:
        mp = None
    if mp is not None:
        with mp.workdps(digits):
            mat = mp.matrix(3, 3)
            for a in range(3):
                for b in range(3):
                    mat[a, b] = mp.mpf(cc[a][b]) / cnt
            ev, evec = mp.eigsy(mat)
            order = sorted(range(3), key=lambda k: ev[k])
            lam = [ev[k] for k in order]
            v = [evec[a, order[0]] for a in range(3)]
            nrm = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
            v = [x / nrm for x in v]
            if v[0] * sn[0] + v[1] * sn[1] + v[2] * sn[2] < 0:
                v = [-x for x in v]
            cen = [(mp.mpf(int(qseed[a])) + mp.mpf(se[a]) / cnt) / mp.mpf(2) ** 20 for a in range(3)]
            d = v[0] * cen[0] + v[1] * cen[1] + v[2] * cen[2]
            rms = mp.sqrt(max(lam[0], mp.mpf(0)) / cnt) / mp.mpf(2) ** 20
            return (np.array([float(x) for x in v]), float(d), np.array([float(x) for x in cen]), float(rms),
                    np.array([float(x) for x in lam]))
    mat = np.array([[float(Fraction(cc[a][b], cnt)) for b in range(3)] for a in range(3)])
    lam, vec = np.linalg.eigh(mat)
    ld = np.longdouble
    v = vec[:, 0].astype(ld)
    v = v / np.sqrt((v * v).sum())
    if v[0] * ld(sn[0]) + v[1] * ld(sn[1]) + v[2] * ld(sn[2]) < 0:
        v = -v
    cen = np.array([(ld(int(qseed[a])) + ld(se[a]) / ld(cnt)) / ld(Q) for a in range(3)])
    return (v.astype(np.float64), float((v * cen).sum()), cen.astype(np.float64), float(np.sqrt(max(lam[0], 0.0) / cnt) / Q), lam)


def _check_input(p32, n32):
    p32, n32 = np.asarray(p32, np.float32).reshape(-1, 3), np.asarray(n32, np.float32).reshape(-1, 3)
    assert len(p32) == len(n32) and np.isfinite(p32).all() and (np.abs(p32) < 2.0 ** 22).all()
    return p32, n32


def _finish(p32, n32, ok, label, prm, plane_of):
    """label: the smallest index of each eligible point's region; plane_of(members, seed) -> (record fields, sums, lam)"""
    n = len(p32)
    plane_id = np.full(n, -1, np.int32)
    seeds, counts = np.unique(label[ok], return_counts=True)
    planes, sums_out, lam_out = [], [], []
    n_cand = 0
    order = np.argsort(label, kind="stable")
    first = np.searchsorted(label[order], seeds)
    for seed, cnt, f in zip(seeds, counts, first):
        if cnt < prm.min_points:
            continue
        n_cand += 1
        members = np.sort(order[f:f + cnt])
        (nv, d, cen, rms, lam), sums = plane_of(members, int(seed))
        if lam[2] > 0 and (prm.max_rms <= 0 or rms <= prm.max_rms):
            plane_id[members] = len(planes)
            planes.append((nv, d, cen, rms, cnt, seed))
            sums_out.append(sums)
            lam_out.append(lam)
    rec = np.zeros(len(planes), PLANE_DTYPE)
    for k, row in enumerate(planes):
        rec[k] = row
    return Result(plane_id, (int(ok.sum()), len(seeds), n_cand, len(planes)), rec, np.where(ok, label, -1), sums_out, lam_out)


def segment_tree(p32, n32, curv32, prm):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    p32, n32 = _check_input(p32, n32)
    p, nn = p32.astype(np.float64), n32.astype(np.float64)
    n = len(p)
    ok = eligible(n32, curv32, prm)
    el = np.flatnonzero(ok)
    label = np.arange(n, dtype=np.int64)
    if len(el) > 1:
        pairs = cKDTree(p[el]).query_pairs(prm.radius * (1 + 1e-9) + 1e-300, output_type="ndarray")
        i, j = el[pairs[:, 0]], el[pairs[:, 1]]
        with np.errstate(invalid="ignore", over="ignore"):
            keep = linked(p, nn, np.maximum(i, j), np.minimum(i, j), prm)
        i, j = i[keep], j[keep]
        _, comp = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n)), directed=False)
        smallest = np.full(comp.max() + 1, n, np.int64)
        np.minimum.at(smallest, comp, np.arange(n))
        label = smallest[comp]
    q = quantise(p32)

    def plane_of(members, seed):
        sums = integer_sums(p32, n32, members, seed)
        return plane_from_sums(sums, q[seed]), sums

    return _finish(p32, n32, ok, label, prm, plane_of)


def segment_grow(p32, n32, curv32, prm):
    p32, n32 = _check_input(p32, n32)
    p, nn = p32.astype(np.float64), n32.astype(np.float64)
    n = len(p)
    ok = eligible(n32, curv32, prm)
    label = np.full(n, -1, np.int64)
    for seed in range(n):                                       # ascending: a region is named by the first index that reaches it
        if not ok[seed] or label[seed] >= 0:
            continue
        label[seed] = seed
        queue = [seed]
        while queue:
            i = queue.pop()
            d = p - p[i]                                        # every point against i; the predicate only where d^2 lets it through
            near = np.flatnonzero((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] <= prm.radius * prm.radius) & ok & (label < 0))
            with np.errstate(invalid="ignore", over="ignore"):
                hit = linked(p, nn, np.maximum(near, i), np.minimum(near, i), prm)
            new = near[hit]
            label[new] = seed
            queue.extend(new.tolist())

    def plane_of(members, seed):
        e = p[members]
        m = e.mean(axis=0)
        d = e - m
        lam, vec = np.linalg.eigh(d.T @ d)
        nv = vec[:, 0]
        if (nv * nn[members].sum(axis=0)).sum() < 0:
            nv = -nv
        return (nv, float(nv @ m), m, float(np.sqrt(max(lam[0], 0.0) / len(members))), lam), None

    return _finish(p32, n32, ok, np.where(ok, label, np.arange(n)), prm, plane_of)
