"""Inputs the mesh smoothing tests share (CPU and GPU): the noisy icosphere, the small shapes on which counting and summing go
wrong, the fan, the sheets around the compaction chunk, the soup, the extreme coordinates, and the renumbering of a mesh."""
import numpy as np

CHUNK = 2048                                                        # compact.h's elements per block

SPHERE = dict(subdivisions=3, radius=0.4, centre=(0.3, -0.2, 1.1), sigma=0.004, seed=0)


def icosphere(subdivisions):
    """unit icosphere, outward winding: (xyz float64 [V,3], tris int64 [T,3]); 3 subdivisions: 642 vertices, 1280 triangles"""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    verts = [np.array(a, np.float64) / np.linalg.norm(a) for a in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]
        nxt = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    return np.array(verts, np.float64), np.array(faces, np.int64)


def noisy_sphere():
    """the icosphere of SPHERE with radial noise: (xyz f32 [642,3], tris u32 [1280,3], unit directions float64 [642,3])"""
    d, tris = icosphere(SPHERE["subdivisions"])
    rng = np.random.default_rng(SPHERE["seed"])
    r = SPHERE["radius"] + rng.normal(0.0, SPHERE["sigma"], len(d))
    xyz = (np.array(SPHERE["centre"], np.float64) + d * r[:, None]).astype(np.float32)
    return xyz, tris.astype(np.uint32), d


def radial(xyz):
    """distance of every vertex from the sphere's centre, in fp64"""
    return np.linalg.norm(np.asarray(xyz, np.float64) - np.array(SPHERE["centre"], np.float64), axis=1)


def renumber(xyz, tris, seed):
    """the same mesh numbered another way: vertices permuted, triangles shuffled, each triangle's corners rotated.  Returns
    (xyz', tris', perm) with xyz'[perm[v]] = xyz[v]."""
    rng = np.random.default_rng(seed)
    n = len(xyz)
    perm = rng.permutation(n)
    xyz2 = np.empty_like(xyz)
    xyz2[perm] = xyz
    t = perm[np.asarray(tris, np.int64)]
    t = t[rng.permutation(len(t))]
    rot = (rng.integers(0, 3, size=len(t))[:, None] + np.arange(3)[None, :]) % 3
    t = np.take_along_axis(t, rot, axis=1)
    return xyz2, np.ascontiguousarray(t.astype(np.uint32)), perm


def _pts(*rows):
    return np.array(rows, np.float32)


def _tri(*rows):
    return np.array(rows, np.uint32).reshape(-1, 3)


def small_shape(name):
    """(xyz f32 [V,3], tris u32 [T,3])"""
    sq = _pts((0.1, 0.2, 1.0), (0.6, 0.25, 1.1), (0.15, 0.7, 0.9), (0.7, 0.8, 1.3), (0.4, 0.45, 1.6))
    if name == "no triangle":
        return sq, _tri()
    if name == "one triangle":
        return sq[:3], _tri((0, 1, 2))
    if name == "isolated vertex":                                   # vertex 3 is in no triangle, vertex 4 only in a degenerate one
        return sq, _tri((0, 1, 2), (4, 4, 4))
    if name == "two triangles on one edge":                         # the edge (1, 2) counts once
        return sq[:4], _tri((0, 1, 2), (2, 1, 3))
    if name == "tetrahedron":
        return sq[[0, 1, 2, 4]], _tri((0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3))
    if name == "bow-tie":                                           # two triangles that share vertex 2 only
        return sq, _tri((0, 1, 2), (2, 3, 4))
    if name == "twice and reversed":                                # (A, B, C) twice plus (A, C, B): the normals partly cancel
        return sq[:3], _tri((0, 1, 2), (0, 1, 2), (0, 2, 1))
    if name == "pair that cancels":                                 # (A, B, C), (A, C, B): zero normals
        return sq[:3], _tri((0, 1, 2), (0, 2, 1))
    if name == "(a, a, b)":                                         # a and b are neighbours; F = 0
        return sq[:3], _tri((0, 0, 1), (1, 2, 2))
    if name == "(a, a, b) beside a triangle":
        return sq[:4], _tri((0, 1, 2), (3, 3, 0))
    raise KeyError(name)


SMALL_SHAPES = ("no triangle", "one triangle", "isolated vertex", "two triangles on one edge", "tetrahedron", "bow-tie",
                "twice and reversed", "pair that cancels", "(a, a, b)", "(a, a, b) beside a triangle")


def fan(k=4096, seed=3):
    """a closed fan of k triangles around one vertex of valence k (a noisy cone), numbering shuffled"""
    rng = np.random.default_rng(seed)
    a = np.arange(k) * (2.0 * np.pi / k)
    r = 0.5 + 0.01 * rng.standard_normal(k)
    rim = np.stack([r * np.cos(a), r * np.sin(a), 1.0 + 0.01 * rng.standard_normal(k)], axis=1)
    xyz = np.concatenate([[[0.02, -0.01, 1.2]], rim]).astype(np.float32)
    i = np.arange(k)
    tris = np.stack([np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % k], axis=1)
    xyz, tris, _ = renumber(xyz, tris, seed)
    return xyz, tris


def sheet(n_vert, n_tri, seed=4):
    """a noisy height field of exactly n_vert vertices, row by row, and the first n_tri triangles of its quads"""
    w = 45
    rows = -(-n_vert // w)
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(rows), np.arange(w), indexing="ij"), axis=-1).reshape(-1, 2)[:n_vert].astype(np.float64)
    xyz = np.concatenate([g * 0.01, 0.8 + 0.002 * rng.standard_normal((n_vert, 1))], axis=1).astype(np.float32)
    a = np.arange(n_vert - w - 1)
    a = a[a % w != w - 1]
    tris = np.concatenate([np.stack([a, a + 1, a + w], axis=1), np.stack([a + 1, a + w + 1, a + w], axis=1)], axis=1).reshape(-1, 3)
    assert len(tris) >= n_tri and int(tris[:n_tri].max()) < n_vert
    return xyz, np.ascontiguousarray(tris[:n_tri].astype(np.uint32))


# n_vert and 3 n_tri one below, at and one above a multiple of the chunk.  3 n_tri = 2048 m - 1 has n_tri = 1365 (4095 = 2 * 2048 - 1)
# and 3413 (10239 = 5 * 2048 - 1), 3 n_tri = 2048 m has 2048 (6144) and 4096 (12288), 3 n_tri = 2048 m + 1 has 683 (2049) and
# 2731 (8193 = 4 * 2048 + 1); every vertex count meets a corner count of another kind too
SHEETS = [(CHUNK - 1, 1365), (CHUNK, 2048), (CHUNK + 1, 683), (2 * CHUNK - 1, 3413), (2 * CHUNK, 4096), (2 * CHUNK + 1, 2731),
          (CHUNK - 1, 683), (CHUNK, 1365), (CHUNK + 1, 2048), (2 * CHUNK - 1, 4096), (2 * CHUNK, 2731), (2 * CHUNK + 1, 3413)]
assert sorted({3 * t % CHUNK for _, t in SHEETS}) == [0, 1, CHUNK - 1] and sorted({v % CHUNK for v, _ in SHEETS}) == [0, 1, CHUNK - 1]


def soup(seed=23):
    """2^16 vertices with random ids, 2^17 triangles among the vertices of one box (long probe chains, valences far from 6)"""
    rng = np.random.default_rng(seed)
    n, t = 1 << 16, 1 << 17
    xyz = rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
    box = np.floor((xyz.astype(np.float64) + 1.0) * 4.0).clip(0, 7).astype(np.int64)
    order = np.lexsort((rng.random(n), box[:, 2], box[:, 1], box[:, 0]))
    per = n // 512
    base = rng.integers(0, n, size=t)
    lo = np.minimum(base // per * per, n - per)
    tris = np.stack([order[base], order[lo + rng.integers(0, per, size=t)], order[lo + rng.integers(0, per, size=t)]], axis=1)
    return xyz, np.ascontiguousarray(tris.astype(np.uint32))


def extremes():
    """two sheets that no triangle joins: one in the plane x = 2^20 m (Q at its largest; 41 m between its vertices, so face
    products near 2^70) and one whose coordinates all lie below 2^-10 m (Q of a few thousand steps)"""
    big = 1048576.0
    xyz, tris = sheet(400, 600, seed=6)
    xyz = xyz.astype(np.float64)
    far = np.stack([np.full(len(xyz), big), -3.0e5 + xyz[:, 0] * 4096.0, 2.0e5 + xyz[:, 1] * 4096.0 + xyz[:, 2] * 10.0], axis=1)
    near = xyz * (2.0 ** -12)
    out = np.concatenate([far, near]).astype(np.float32)
    assert np.abs(out).max() == big and np.abs(out[400:]).max() < 2.0 ** -10
    return out, np.ascontiguousarray(np.concatenate([tris, tris.astype(np.int64) + 400]).astype(np.uint32))


WIDE_FAN_K = 270000


def wide_fan(k=WIDE_FAN_K, seed=8):
    """a fan whose hub lies 2^21 m from its k rim vertices along x: the hub's D_x = k * 2^45 passes 2^63 from k = 2^18, and the
    face vectors reach 2^90, their sum 2^108.  One iteration keeps every coordinate in range."""
    big = 1048576.0
    rng = np.random.default_rng(seed)
    a = np.arange(k) * (2.0 * np.pi / k)
    rim = np.stack([np.full(k, big), 5.0e5 * np.cos(a), 5.0e5 * np.sin(a) + rng.standard_normal(k)], axis=1)
    xyz = np.concatenate([[[-big, 10.0, -20.0]], rim]).astype(np.float32)
    i = np.arange(k)
    tris = np.stack([np.zeros(k, np.int64), 1 + i, 1 + (i + 1) % k], axis=1)
    xyz, tris, _ = renumber(xyz, tris, seed)
    return xyz, tris


def spiky():
    """a tetrahedron 100 km across: with lambda = 1 and mu = -2 every vertex's offset from the centroid grows by 11 / 9 per
    iteration (the lambda step takes it to -1/3 of itself, the mu step multiplies by 11/3), past 2^20 m within a dozen iterations"""
    xyz, tris = small_shape("tetrahedron")
    return (xyz.astype(np.float64) * 2.0e5).astype(np.float32), tris


_CACHE = {}


def reference(name, build, iterations, lam=0.5, mu=-0.53):
    """(xyz, tris, smoothed, info, normals, n_zero) of a named mesh, computed once and shared (read-only)"""
    import mesh_smooth_reference as ref
    key = (name, iterations, lam, mu)
    if key not in _CACHE:
        xyz, tris = build()
        out, info = ref.smooth(xyz, tris, iterations, lam, mu)
        nrm, nz = ref.normals(xyz, tris)
        for a in (xyz, tris, out, info["valence"], nrm):
            a.setflags(write=False)
        _CACHE[key] = (xyz, tris, out, info, nrm, nz)
    return _CACHE[key]
