"""Shared by the global-registration tests (CPU and GPU): the "four solids" scene and the crafted cases, all from seeds, with their
reference answers (tests/cloud_global_reference.py) computed once per process and left unchanged."""
import functools

import numpy as np

import cloud_global_reference as gr

# the scene: (kind, centre, half-extents or radius, samples)
SOLIDS = (("box", (0.0, 0.0, 0.0), (0.5, 0.4, 0.3), 1400), ("box", (0.35, 0.1, 0.45), (0.15, 0.2, 0.15), 500),
          ("sphere", (-0.3, -0.2, 0.4), 0.18, 400), ("box", (-0.6, 0.25, -0.1), (0.1, 0.08, 0.2), 300))
PLANT_AXIS, PLANT_DEG, PLANT_T = (1.0, 2.0, 3.0), 130.0, (0.7, -0.4, 1.1)
K, RADIUS, HYPOTHESES, MAX_DIST = 48, 0.15, 20_000, 0.03
FPFH_KS = (8, 32, 33, 48, 64)


def _box(n, c, h, rng):
    c, h = np.array(c, float), np.array(h, float)
    areas = np.array([h[1] * h[2], h[0] * h[2], h[0] * h[1]])
    face = rng.choice(6, n, p=np.repeat(areas / areas.sum() / 2, 2))
    u = rng.uniform(-1, 1, (n, 3)) * h
    ax, sg = face // 2, (face % 2) * 2.0 - 1
    u[np.arange(n), ax] = sg * h[ax]
    nr = np.zeros((n, 3))
    nr[np.arange(n), ax] = sg
    return u + c, nr


def _sphere(n, c, r, rng):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return np.array(c) + r * v, v


def four_solids(seed, scale=1.0):
    """(points, outward normals) float32: surface samples by area, 1400 / 500 / 400 / 300 x scale per solid"""
    rng = np.random.default_rng(seed)
    parts = [(_box if kind == "box" else _sphere)(int(n * scale), c, size, rng) for kind, c, size, n in SOLIDS]
    return (np.concatenate([a for a, _ in parts]).astype(np.float32), np.concatenate([b for _, b in parts]).astype(np.float32))


def rotation(axis, deg):
    a = np.array(axis, float)
    a /= np.linalg.norm(a)
    th = np.radians(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def planted_pose():
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rotation(PLANT_AXIS, PLANT_DEG), PLANT_T
    return T


@functools.lru_cache(maxsize=None)
def scene(noise=0.0, scale=1.0):
    """dict: tgt, tgt_normals (seed 1), src, src_normals (seed 2, un-moved by the planted pose; `noise` metres of Gaussian noise),
    T (source to target).  Both normal sets are turned towards their own cloud's centroid.  No point is shared."""
    tg, tn = four_solids(1, scale)
    sp, sn = four_solids(2, scale)
    T = planted_pose()
    R0, t0 = T[:3, :3], T[:3, 3]
    src = ((sp.astype(np.float64) - t0) @ R0).astype(np.float32)
    srcn = (sn.astype(np.float64) @ R0).astype(np.float32)
    if noise:
        src = src + np.random.default_rng(3).normal(0, noise, src.shape).astype(np.float32)
    out = dict(tgt=tg, tgt_normals=gr.orient_to_centroid(tg, tn), src=src, src_normals=gr.orient_to_centroid(src, srcn), T=T)
    for v in out.values():
        v.setflags(write=False)
    return out


def displacement(T, T_true, points):
    """the largest distance between where T and T_true put a point of `points`"""
    p = np.asarray(points, np.float64)
    return float(np.linalg.norm((p @ T[:3, :3].T + T[:3, 3]) - (p @ T_true[:3, :3].T + T_true[:3, 3]), axis=1).max())


@functools.lru_cache(maxsize=None)
def scene_recipe(noise=0.0, mutual=True):
    s = scene(noise)
    return gr.recipe(s["src"], s["src_normals"], s["tgt"], s["tgt_normals"], K, RADIUS, HYPOTHESES, MAX_DIST, seed=0, mutual=mutual)


# ---- subsample cases: name -> (points, voxel) -------------------------------------------------------------------------------------
SUB_CASES = ("random", "faces", "one_voxel", "duplicates", "cell_limit", "n255", "n256", "n257")


@functools.lru_cache(maxsize=None)
def sub_case(name):
    rng = np.random.default_rng(SUB_CASES.index(name) + 11)
    if name == "random":
        return (rng.uniform(-1, 1, (3000, 3)) * (1.0, 0.7, 0.4)).astype(np.float32), 0.05
    if name == "faces":                         # dyadic voxel: lattice coordinates are exact, points ON cell faces, negative ones too
        g = rng.integers(-6, 7, (1500, 3)).astype(np.float32) * 0.125
        g[::3] += (rng.uniform(0, 0.24, (500, 3))).astype(np.float32)
        return g, 0.25
    if name == "one_voxel":
        return (rng.uniform(0.01, 0.99, (700, 3)) * 0.5).astype(np.float32), 0.5
    if name == "duplicates":
        base = (rng.uniform(-1, 1, (300, 3))).astype(np.float32)
        return base[rng.integers(0, 300, 1200)], 0.1
    if name == "cell_limit":                    # |cell| = 2^20 - 1 on both sides, voxel 2^-4: coordinates are exact in f32
        lim = (1 << 20) - 1
        p = np.array([[lim / 16.0, 0, 0], [-lim / 16.0, 0, 0], [0, lim / 16.0 + 0.03, 0], [0, 0, -lim / 16.0], [lim / 16.0, 0.01, 0.02]], np.float32)
        return p, 1.0 / 16
    n = int(name[1:])
    return (rng.uniform(-1, 1, (n, 3))).astype(np.float32), 0.3


# ---- FPFH cases: name -> dict(xyz, normals, k, radius) ----------------------------------------------------------------------------
FPFH_CASES = tuple(f"scene_k{k}" for k in FPFH_KS) + ("lattice_ties", "duplicates", "zero_normals", "parallel", "isolated", "k_gt_n")


@functools.lru_cache(maxsize=None)
def fpfh_case(name):
    rng = np.random.default_rng(FPFH_CASES.index(name) + 101)
    if name.startswith("scene_k"):
        s = scene()
        return dict(xyz=s["src"][::2], normals=s["src_normals"][::2], k=int(name[7:]), radius=RADIUS)

    def unit(v):
        return (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)
    if name == "lattice_ties":                  # a dyadic lattice: every k-NN list is full of exact ties
        g = np.stack(np.meshgrid(np.arange(7), np.arange(6), np.arange(5), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 0.125
        return dict(xyz=g, normals=unit(rng.normal(size=g.shape)), k=12, radius=0.3)
    if name == "duplicates":
        base = rng.uniform(-0.3, 0.3, (150, 3)).astype(np.float32)
        pick = rng.integers(0, 150, 400)
        return dict(xyz=base[pick], normals=unit(rng.normal(size=(400, 3))), k=16, radius=0.25)
    if name == "zero_normals":
        p = rng.uniform(-0.3, 0.3, (400, 3)).astype(np.float32)
        nr = unit(rng.normal(size=p.shape))
        nr[::5] = 0
        return dict(xyz=p, normals=nr, k=10, radius=0.3)
    if name == "parallel":                      # d parallel to ns for the pairs along x: |v| == 0, the pair is skipped
        p = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0, 0.25, 0], [0.25, 0.5, 0.125]], np.float32)
        nr = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
        return dict(xyz=p, normals=nr, k=4, radius=0.0)
    if name == "isolated":
        p = rng.uniform(-0.2, 0.2, (200, 3)).astype(np.float32)
        p[77] = (3.0, 3.0, 3.0)
        return dict(xyz=p, normals=unit(rng.normal(size=p.shape)), k=8, radius=0.2)
    if name == "k_gt_n":
        p = rng.uniform(-0.2, 0.2, (6, 3)).astype(np.float32)
        return dict(xyz=p, normals=unit(rng.normal(size=p.shape)), k=20, radius=0.0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def fpfh_ref(name):
    c = fpfh_case(name)
    return gr.fpfh(c["xyz"], c["normals"], c["k"], c["radius"])


# ---- match cases: name -> (a, b) -------------------------------------------------------------------------------------------------
MATCH_CASES = ("scene", "ties", "dim1", "dim33", "dim34", "dim64", "nb1", "nb63", "nb64", "nb65")


@functools.lru_cache(maxsize=None)
def match_case(name):
    rng = np.random.default_rng(MATCH_CASES.index(name) + 201)
    if name == "scene":
        r = scene_recipe()
        return r["fs"]["fpfh"], r["ft"]["fpfh"]
    if name == "ties":                          # duplicated rows of b: the smaller index wins; small integers: every d2 is exact
        b = rng.integers(0, 4, (40, 33)).astype(np.float32)
        b = np.concatenate([b, b[::-1], b])
        return rng.integers(0, 4, (300, 33)).astype(np.float32), b
    if name.startswith("dim"):
        d = int(name[3:])
        return rng.normal(size=(300, d)).astype(np.float32), rng.normal(size=(200, d)).astype(np.float32)
    nb = int(name[2:])
    return rng.normal(size=(257, 33)).astype(np.float32), rng.normal(size=(nb, 33)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def match_ref(name):
    return gr.match_features(*match_case(name))


# ---- RANSAC cases: name -> dict(src, tgt, corr, hypotheses, max_dist, edge_ratio, seed) -------------------------------------------
RANSAC_CASES = ("scene", "scene_all", "m3", "all_fail", "threshold")


@functools.lru_cache(maxsize=None)
def ransac_case(name):
    if name in ("scene", "scene_all"):
        s, r = scene(), scene_recipe(mutual=name == "scene")
        return dict(src=s["src"], tgt=s["tgt"], corr=r["corr"], hypotheses=HYPOTHESES, max_dist=MAX_DIST, edge_ratio=0.9, seed=0)
    if name == "m3":                            # three correspondences: a hypothesis passes when its draws are a permutation
        src = np.array([[0, 0, 0], [1, 0, 0], [0, 0.5, 0], [0.25, 0.25, 1]], np.float32)
        tgt = (src.astype(np.float64) @ rotation((0, 0, 1), 90).T + (2, 0, 0)).astype(np.float32)
        return dict(src=src, tgt=tgt, corr=np.array([[0, 0], [1, 1], [2, 2]], np.int32), hypotheses=64, max_dist=0.01, edge_ratio=0.9, seed=7)
    if name == "all_fail":                      # the target is the source at twice the size: every edge pair has ratio 0.5
        src = np.random.default_rng(5).uniform(-1, 1, (50, 3)).astype(np.float32)
        return dict(src=src, tgt=(2 * src).astype(np.float32), corr=np.stack([np.arange(50)] * 2, 1).astype(np.int32), hypotheses=500,
                    max_dist=0.05, edge_ratio=0.9, seed=1)
    if name == "threshold":
        # Dyadic coordinates and a pure translation: a hypothesis that draws the pairs 0, 1, 2 or 0, 2, 1 in that order builds its
        # triads from axis-aligned unit edges, so its pose is EXACT (R = I, t = (4, 0, 0)): the residual of the fourth pair is exactly
        # its planted offset 0.25 = max_dist (it counts) and the fifth's is 0.5 (it does not).  The reference reports on_threshold.
        src = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 2], [2, 2, 0.5]], np.float32)
        tgt = src + np.float32([4, 0, 0])
        tgt[3] += np.float32([0, 0, 0.25])
        tgt[4] += np.float32([0, 0.5, 0])
        return dict(src=src, tgt=tgt, corr=np.stack([np.arange(5)] * 2, 1).astype(np.int32), hypotheses=256, max_dist=0.25, edge_ratio=0.9, seed=3)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ransac_ref(name):
    c = ransac_case(name)
    return gr.ransac(c["src"], c["tgt"], c["corr"], c["hypotheses"], c["max_dist"], c["edge_ratio"], c["seed"])
