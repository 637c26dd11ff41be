"""Shared by the cloud-registration tests (CPU and GPU): the clouds at the edges of tl3d_cloud_evaluate / tl3d_cloud_register
(kernels_cloudicp.hip; the contract is in include/tl3d.h and DESIGN.md section 14), generated from seeds, and the references of
tests/cloud_register_reference.py on them, each computed once per process."""
import functools
import math

import numpy as np

import cloud_register_reference as cr

PARITY = 1e-4            # the project's ICP parity bar (README): pose and scale against the reference
REDUCE_THREADS = 512 * 256      # the reduce pass's grid x block at its cap (kernels_cloudicp.hip: CLOUD_MEMBERS_CAP workgroups of 256)


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def pose(axis, deg, t):
    T = np.eye(4)
    T[:3, :3] = rot(axis, deg)
    T[:3, 3] = t
    return T


def unmove(points, T, scale=1.0):
    """The float32 source that (T, scale) maps onto `points`: p = R^T (x - t) / scale."""
    x = np.asarray(points, np.float64)
    return (((x - T[:3, 3]) @ T[:3, :3]) / scale).astype(np.float32)


def move(points, T, scale=1.0):
    """scale * R p + t in fp64, rounded to float32 (what metrics.align_clouds does on the host)."""
    p = np.asarray(points, np.float32).astype(np.float64)
    return (scale * (p @ T[:3, :3].T) + T[:3, 3]).astype(np.float32)


# ---- surfaces -----------------------------------------------------------------------------------------------------------------
BOX_C, BOX_H = np.array([2.0, 1.0, 3.0]), np.array([0.5, 0.4, 0.3])


def box_samples(n, seed, centre=BOX_C, half=BOX_H):
    """n points on the surface of the box, by area, with the outward face normals (float32 both)."""
    rng = np.random.default_rng(seed)
    areas = np.array([half[1] * half[2], half[0] * half[2], half[0] * half[1]])
    face = rng.choice(6, n, p=np.repeat(areas / areas.sum() / 2, 2))
    u = rng.uniform(-1, 1, (n, 3)) * half
    axis, sign = face // 2, (face % 2) * 2.0 - 1.0
    u[np.arange(n), axis] = sign * half[axis]
    nrm = np.zeros((n, 3))
    nrm[np.arange(n), axis] = sign
    return (u + centre).astype(np.float32), nrm.astype(np.float32)


def plane_samples(n, seed, z=0.5, half=1.0):
    rng = np.random.default_rng(seed)
    p = np.column_stack([rng.uniform(-half, half, n), rng.uniform(-half, half, n), np.full(n, z)])
    return p.astype(np.float32), np.tile(np.array([0, 0, 1], np.float32), (n, 1))


def default_cell(tgt):
    """tl3d_nearest_points' default cell: (V / (4 n))^(1/k) over the box's k non-zero extents."""
    t = np.asarray(tgt, np.float32).astype(np.float64)
    ext = t.max(axis=0) - t.min(axis=0)
    ext = ext[ext > 0]
    return 1.0 if len(ext) == 0 else float(np.prod(ext) / (4.0 * len(t))) ** (1.0 / len(ext))


# ---- tl3d_cloud_evaluate: one dict per case: src, tgt, normals (or None), and the call's keywords --------------------------------
T_BOX = pose((1, 2, 3), 3.0, (0.02, -0.015, 0.01))


def _box(n_src=500, n_tgt=700, **kw):
    tgt, nrm = box_samples(n_tgt, 11)
    pts, _ = box_samples(n_src, 12)
    return dict(dict(src=unmove(pts, T_BOX, 1.03), tgt=tgt, normals=nrm, T=T_BOX, scale=1.03, max_dist=0.2), **kw)


def _ties():
    # an 8 x 8 x 8 lattice of spacing 1/4; the moved sources sit on edge midpoints (2 nearest), face centres (4) and cell centres
    # (8).  T is exact in fp64: 90 degrees about z and a dyadic translation, so q and every d2 are exact and the ties are ties.
    g = np.arange(8) * 0.25
    tgt = np.array([(x, y, z) for z in g for y in g for x in g], np.float32)
    rng = np.random.default_rng(5)
    base = rng.integers(0, 7, (90, 3)) * 0.25
    off = np.array([(0.125, 0, 0), (0, 0.125, 0), (0, 0, 0.125), (0.125, 0.125, 0), (0.125, 0, 0.125), (0, 0.125, 0.125),
                    (0.125, 0.125, 0.125)])
    q = base + off[np.arange(90) % 7]
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = (0.5, -0.25, 1.0)
    src = unmove(q, T)
    assert np.array_equal(cr.transform(src, T, 1.0)[1], q)
    nrm = np.tile(np.array([0.0, 0.6, 0.8], np.float32), (len(tgt), 1))
    return dict(src=src, tgt=tgt, normals=nrm, T=T, scale=1.0, max_dist=1.0)


def _gate_edge():
    # the target's point 0 at the origin, the rest far away; sources at exactly max_dist = 1/4 along an axis (kept) and one float32
    # step beyond (dropped)
    tgt = np.array([(0, 0, 0), (8, 8, 8), (-8, 8, 8), (8, -8, 8), (8, 8, -8), (-8, -8, -8), (16, 0, 0)], np.float32)
    up = np.nextafter(np.float32(0.25), np.float32(1))
    src = np.array([(0.25, 0, 0), (up, 0, 0), (0, -0.25, 0), (0, -up, 0), (0, 0, 0.25), (0, 0, up), (0, 0, 0), (0.125, 0, 0)], np.float32)
    nrm = np.tile(np.array([0.6, 0.0, 0.8], np.float32), (len(tgt), 1))
    return dict(src=src, tgt=tgt, normals=nrm, T=np.eye(4), scale=1.0, max_dist=0.25, expect_index=[0, -1, 0, -1, 0, -1, 0, 0])


def _outside(max_dist):
    c = _box(n_src=200)
    diag = 2 * np.linalg.norm(BOX_H)
    T = c["T"].copy()
    T[:3, 3] += 100 * diag * np.array([0.6, 0.0, 0.8])
    return dict(c, T=T, max_dist=max_dist)


def _zero_normals():
    c = _box()
    nrm = c["normals"].copy()
    nrm[::3] = 0.0
    return dict(c, normals=nrm)


def _big():
    # just above the reduce pass's grid x block: its stride loop runs twice in the first threads
    tgt, nrm = box_samples(1000, 21)
    rng = np.random.default_rng(22)
    n = REDUCE_THREADS + 37
    src = (BOX_C + rng.uniform(-1, 1, (n, 3)) * (BOX_H + 0.05)).astype(np.float32)
    return dict(src=src, tgt=tgt, normals=nrm, T=pose((0, 0, 1), 1.0, (0.01, 0, 0)), scale=1.0, max_dist=0.1, nearest="kdtree")


EVAL_CASES = {
    "box_plane": lambda: _box(),
    "box_plane_scale": lambda: _box(with_scale=True),
    "box_point": lambda: _box(normals=None),
    "box_point_scale": lambda: _box(normals=None, with_scale=True),
    "ties": _ties,
    "ties_point": lambda: dict(_ties(), normals=None, with_scale=True),
    "gate_edge": _gate_edge,
    "outside_gated": lambda: _outside(0.2),
    "outside_ungated": lambda: _outside(0.0),
    "zero_normals": _zero_normals,
    "one_target": lambda: dict(_box(n_tgt=1), max_dist=0.0),
    "stride": lambda: _box(stride=3, with_scale=True),
    "n255": lambda: _box(n_src=255),
    "n256": lambda: _box(n_src=256, normals=None),
    "n257": lambda: _box(n_src=257, with_scale=True),
    "big": _big,
}


@functools.lru_cache(maxsize=None)
def eval_case(name):
    return EVAL_CASES[name]()


def eval_kwargs(case):
    return {k: case[k] for k in ("T", "scale", "stride", "max_dist", "with_scale") if k in case}


@functools.lru_cache(maxsize=None)
def eval_ref(name):
    c = eval_case(name)
    near = cr.nearest_kdtree if c.get("nearest") == "kdtree" else cr.nearest_brute
    return cr.evaluate(c["src"], c["tgt"], c["normals"], nearest=near, **eval_kwargs(c))


# ---- tl3d_cloud_register: the planted poses ------------------------------------------------------------------------------------
T_TRUE = pose((1, 2, 3), 3.0, (0.02, -0.015, 0.01))        # 3 degrees and 2.7 cm


def _closed_box(sigma, plane):
    tgt, nrm = box_samples(4000, 1)
    pts, _ = box_samples(800, 2)
    return dict(src=unmove(pts, T_TRUE, sigma), tgt=tgt, normals=nrm if plane else None, truth=(T_TRUE, sigma),
                kw=dict(estimate_scale=sigma != 1.0))


def _moved_subset(plane):
    tgt, nrm = box_samples(4000, 1)
    return dict(src=unmove(tgt[::5], T_TRUE), tgt=tgt, normals=nrm if plane else None, truth=(T_TRUE, 1.0),
                kw=dict(levels=(dict(iters=10, stride=4, max_dist=0.20), dict(iters=30, stride=1, max_dist=0.05))))


def _single_plane():
    tgt, nrm = plane_samples(500, 3)
    pts, _ = plane_samples(300, 4, half=0.9)
    return dict(src=pts + np.array([0, 0, 0.01], np.float32), tgt=tgt, normals=nrm, truth=None, kw={})


REG_CASES = {f"box_{'plane' if pl else 'point'}_{s}": functools.partial(_closed_box, s, pl) for pl in (True, False) for s in (1.0, 1.05, 0.95)}
REG_CASES.update(subset_plane=lambda: _moved_subset(True), subset_point=lambda: _moved_subset(False), single_plane=_single_plane)


@functools.lru_cache(maxsize=None)
def reg_case(name):
    return REG_CASES[name]()


@functools.lru_cache(maxsize=None)
def reg_ref(name):
    c = reg_case(name)
    return cr.register(c["src"], c["tgt"], c["normals"], **c["kw"])


def truth_distance(res, truth):
    """(Frobenius distance of the 4 x 4 pose to the truth's, |scale - truth's|)."""
    return float(np.linalg.norm(np.asarray(res["T"]) - truth[0])), abs(res["scale"] - truth[1])
