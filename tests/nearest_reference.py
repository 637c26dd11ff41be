"""Brute-force fp64 references of the nearest-neighbour searches (tl3d_nearest_points / tl3d_nearest_triangles): every query against
every target, no grid, no early exit.  numpy only.

Points: differences of the float32 coordinates in fp64 (what the kernel takes too), (dx*dx + dy*dy) + dz*dz, the first minimum
(numpy's argmin: the smallest index among exact ties), one square root.

Triangles: Ericson's region form (Real-Time Collision Detection, 5.1.5: vertex regions, edge regions, interior by barycentric
coordinates) for triangles with a normal.  The region form divides 0 by 0 on a triangle without one (collinear or repeated corners:
it is then a segment or a point), so those take the minimum over their three closed edges.  `tri_dist_second` is the second
formulation the CPU test holds it against: the minimum over the face projection (where it falls inside), the three segments and
the three corners, in np.longdouble."""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float32).reshape(-1, 3).astype(np.float64)


def point_d2_matrix(query, target):
    q, t = _f64(query), _f64(target)
    d = t[None, :, :] - q[:, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest_points_ref(query, target, chunk=512):
    """(dist float64 [n], index int32 [n]); an empty target gives +inf / -1"""
    q = _f64(query)
    n = len(q)
    if len(target) == 0:
        return np.full(n, np.inf), np.full(n, -1, np.int32)
    dist, idx = np.empty(n), np.empty(n, np.int32)
    for s in range(0, n, chunk):
        d2 = point_d2_matrix(query[s:s + chunk], target)
        i = d2.argmin(axis=1)
        idx[s:s + chunk] = i
        dist[s:s + chunk] = np.sqrt(d2[np.arange(len(i)), i])
    return dist, idx


def point_dist_to(query, target, index):
    d = _f64(target)[np.asarray(index, dtype=np.int64)] - _f64(query)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _seg_dist(p, a, b):
    """distance from p to the closed segment [a, b] (a == b: the point), broadcasting"""
    ab, ap = b - a, p - a
    den = _dot(ab, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(den > 0, _dot(ap, ab) / np.where(den > 0, den, 1), 0)
    t = np.clip(t, 0, 1)
    c = ap - t[..., None] * ab
    return np.sqrt(_dot(c, c))


def _ericson(p, a, b, c):
    """distance from p to the triangle (a, b, c) by the region form; arrays broadcast to [..., 3]; triangles with a normal only"""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    shape = np.broadcast(d1, d3).shape
    closest = np.empty(shape + (3,), p.dtype)
    todo = np.ones(shape, bool)

    def put(mask, value):
        nonlocal todo
        m = todo & mask
        closest[m] = np.broadcast_to(value, shape + (3,))[m]
        todo = todo & ~m

    def safe(num, den):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den != 0, num / np.where(den != 0, den, 1), 0)

    put((d1 <= 0) & (d2 <= 0), a)
    put((d3 >= 0) & (d4 <= d3), b)
    put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + safe(d1, d1 - d3)[..., None] * ab)
    put((d6 >= 0) & (d5 <= d6), c)
    put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + safe(d2, d2 - d6)[..., None] * ac)
    put((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + safe(d4 - d3, (d4 - d3) + (d5 - d6))[..., None] * (c - b))
    den = va + vb + vc
    v, w = safe(vb, den), safe(vc, den)
    put(np.ones(shape, bool), a + v[..., None] * ab + w[..., None] * ac)
    d = p - closest
    return np.sqrt(_dot(d, d))


def _corners(xyz, tris, dtype):
    v = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(dtype)
    t = np.asarray(tris).reshape(-1, 3).astype(np.int64)
    return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]


def tri_dist_matrix(query, xyz, tris, chunk=256):
    """fp64 [n_query, n_tri]: the reference distance of every query to every triangle"""
    a, b, c = _corners(xyz, tris, np.float64)
    q = _f64(query)
    n = np.cross(b - a, c - a)
    flat = _dot(n, n) == 0
    out = np.empty((len(q), len(a)))
    for s in range(0, len(q), chunk):
        p = q[s:s + chunk, None, :]
        d = _ericson(p, a[None], b[None], c[None])
        if flat.any():
            af, bf, cf = a[None, flat], b[None, flat], c[None, flat]
            d[:, flat] = np.minimum(_seg_dist(p, af, bf), np.minimum(_seg_dist(p, bf, cf), _seg_dist(p, cf, af)))
        out[s:s + chunk] = d
    return out


def tri_dist_second(query, xyz, tris, chunk=128):
    """np.longdouble [n_query, n_tri]: the minimum over the face projection where it falls inside, three segments, three corners"""
    L = np.longdouble
    a, b, c = _corners(xyz, tris, L)
    q = np.asarray(query, dtype=np.float32).reshape(-1, 3).astype(L)
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    out = np.empty((len(q), len(a)), L)
    for s in range(0, len(q), chunk):
        p = q[s:s + chunk, None, :]
        best = np.minimum(_seg_dist(p, a[None], b[None]), np.minimum(_seg_dist(p, b[None], c[None]), _seg_dist(p, c[None], a[None])))
        for corner in (a, b, c):
            d = p - corner[None]
            best = np.minimum(best, np.sqrt(_dot(d, d)))
        # the foot of the perpendicular: p - (n . (p - a)) n / (n . n); inside when it is on the inner side of all three edges
        with np.errstate(divide="ignore", invalid="ignore"):
            h = _dot(n[None], p - a[None])
            foot = p - (h / np.where(nn > 0, nn, 1))[..., None] * n[None]
            inside = nn[None] > 0
            for u, v in ((a, b), (b, c), (c, a)):
                inside = inside & (_dot(np.cross((v - u)[None], foot - u[None]), n[None]) >= 0)
            face = np.abs(h) / np.sqrt(np.where(nn > 0, nn, 1))[None]
        out[s:s + chunk] = np.where(inside, np.minimum(best, face), best)
    return out


def nearest_triangles_ref(query, xyz, tris):
    """(dist float64 [n], tri int32 [n], the whole matrix); no triangles: +inf / -1"""
    nq = len(np.asarray(query).reshape(-1, 3))
    if len(np.asarray(tris).reshape(-1, 3)) == 0:
        return np.full(nq, np.inf), np.full(nq, -1, np.int32), np.zeros((nq, 0))
    m = tri_dist_matrix(query, xyz, tris)
    i = m.argmin(axis=1)
    return m[np.arange(nq), i], i.astype(np.int32), m
