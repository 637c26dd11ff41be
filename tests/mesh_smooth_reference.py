"""numpy / Python-integer restatement of the mesh smoothing and vertex normal rules: what
tl3d_mesh_smooth_taubin and tl3d_mesh_vertex_normals must give, bit for bit.  Every sum is taken in Python integers (object
arrays), which have no width; every fp64 operation is one IEEE operation, in the contract's order."""
import numpy as np

Q_SCALE = 16777216.0
RANGE = 1048576.0
TWO64 = 18446744073709551616.0
_MASK64 = (1 << 64) - 1


def quantise(x):
    """Q(x) = (int64) rint((double) x * 2^24), halves to even, as an int64 array"""
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * Q_SCALE).astype(np.int64)


def dbl(n) -> float:
    """a wide integer as a double, by the contract: sign and magnitude apart, |n| = hi 2^64 + lo, (double)hi * 2^64 + (double)lo"""
    n = int(n)
    m = -n if n < 0 else n
    d = float(m >> 64) * TWO64 + float(m & _MASK64)                     # int -> float rounds to nearest even, as the device's conversion
    return -d if n < 0 else d


def _dbl_array(a):
    """dbl() of every element of an object array of integers, as float64"""
    flat = a.reshape(-1)
    if not len(flat):
        return np.zeros(a.shape, np.float64)
    m = np.abs(flat)
    hi = (m >> 64).astype(np.float64)                                   # (each element through float(): to nearest even)
    lo = (m & _MASK64).astype(np.uint64).astype(np.float64)
    d = hi * TWO64 + lo
    return np.where((flat < 0).astype(bool), -d, d).reshape(a.shape)


def check_input(xyz, tris):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.uint32).reshape(-1, 3)
    if len(tris) and int(tris.max()) >= len(xyz):
        raise ValueError("triangle index out of range")
    if not (np.abs(xyz) <= np.float32(RANGE)).all():                   # false for NaN
        raise ValueError("vertex not finite or beyond 2^20 m")
    return xyz, tris


def unique_edges(tris, n_vert):
    """(edges int64 [E,2] with u < v, each once; valence uint32 [n_vert])"""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e = e[e[:, 0] != e[:, 1]]
    key = np.unique(np.minimum(e[:, 0], e[:, 1]) << 32 | np.maximum(e[:, 0], e[:, 1]))
    e = np.stack([key >> 32, key & 0xFFFFFFFF], axis=1)
    val = np.bincount(e.reshape(-1), minlength=n_vert).astype(np.uint32) if n_vert else np.zeros(0, np.uint32)
    return e, val


def step(xyz, edges, valence, s):
    """one Jacobi step with factor s"""
    x = np.asarray(xyz, np.float32)
    qi = quantise(x)
    q = qi.astype(object)
    # the neighbour sums in two 32-bit halves, Q = hi 2^32 + lo with 0 <= lo < 2^32: each half's sum stays below 2^63 for any
    # valence below 2^31, and the halves are put together in Python integers
    hi, lo = np.zeros(qi.shape, np.int64), np.zeros(qi.shape, np.int64)
    for a, b in ((0, 1), (1, 0)):
        if len(edges):
            np.add.at(hi, edges[:, a], qi[edges[:, b]] >> 32)
            np.add.at(lo, edges[:, a], qi[edges[:, b]] & 0xFFFFFFFF)
    S = hi.astype(object) * (1 << 32) + lo.astype(object)
    k = valence.astype(np.int64)
    D = S - k.astype(object)[:, None] * q
    moved = k > 0
    out = x.copy()
    if moved.any():
        den = k[moved].astype(np.float64)[:, None] * Q_SCALE
        t = _dbl_array(D[moved]) / den
        w = np.float64(s) * t
        out[moved] = (x[moved].astype(np.float64) + w).astype(np.float32)
    return out


def smooth(xyz, tris, iterations, lam=0.5, mu=-0.53):
    """(xyz f32 [V,3], info): info has edges, valence (u32 [V]) and max_valence"""
    if not (0 <= int(iterations) <= 1000 and 0.0 < lam <= 1.0 and -2.0 <= mu <= 0.0):
        raise ValueError("parameter out of range")
    xyz, tris = check_input(xyz, tris)
    edges, val = unique_edges(tris, len(xyz))
    out = xyz.copy()
    for _ in range(int(iterations)):
        out = step(out, edges, val, lam)
        out = step(out, edges, val, mu)
        if not (np.abs(out) <= np.float32(RANGE)).all():
            raise ValueError("smoothing diverged")
    return out, dict(edges=len(edges), valence=val, max_valence=int(val.max()) if len(val) else 0)


def face_vectors(xyz, tris):
    """F of every triangle in exact integers: object array [T,3]"""
    q = quantise(xyz).astype(object)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    e1, e2 = q[t[:, 1]] - q[t[:, 0]], q[t[:, 2]] - q[t[:, 0]]
    F = np.empty((len(t), 3), object)
    F[:, 0] = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    F[:, 1] = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    F[:, 2] = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return F


def normal_sums(xyz, tris):
    """N_v in exact integers: object array [V,3]"""
    xyz, tris = check_input(xyz, tris)
    N = np.zeros((len(xyz), 3), object)
    if len(tris):
        F = face_vectors(xyz, tris)
        t = tris.astype(np.int64)
        for c in range(3):
            np.add.at(N, t[:, c], F)
    return N


def normals(xyz, tris):
    """(normals f32 [V,3], the number of zero normals)"""
    N = normal_sums(xyz, tris)
    out = np.zeros(N.shape, np.float32)
    zero = np.array([not (a or b or c) for a, b, c in N], bool) if len(N) else np.zeros(0, bool)
    if (~zero).any():
        n = _dbl_array(N[~zero])
        L = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        out[~zero] = (n / L[:, None]).astype(np.float32)
    return out, int(zero.sum())
