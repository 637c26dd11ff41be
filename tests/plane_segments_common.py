"""Shared by the plane segmentation tests (CPU and GPU): the crafted clouds of tl3d_segment_planes (kernels_planes.hip; the definition
is in include/tl3d.h), their parameters and known answers, and the bar of the plane parameters.  No GPU imports.  Not a test.

THE BAR (derived, not measured).  The kernel forms C_ab = fl(S_ab) - fl(fl(s_a s_b) / c) in fp64 from the exact integers S_ab = sum
e_a e_b, s_a = sum e_a and the count c.  Counting roundings of relative size u = 2^-53 along that sequence:
    S_ab -> fp64   two (the high and the low 64 bits are converted apart and added)     <= 2 u |S_ab|
    s_a, s_b -> fp64, their product, the division by c: four                           <= 4 u |s_a s_b| / c  (first order)
    the subtraction: one                                                               <= u |C_ab| <= u (|S_ab| + |s_a s_b| / c)
By Cauchy-Schwarz |S_ab| <= sqrt(S_aa S_bb) and s_a^2 <= c S_aa, so |s_a s_b| / c <= sqrt(S_aa S_bb) too and every entry is off by
at most 8 u sqrt(S_aa S_bb); the Frobenius norm of the perturbation, hence its 2-norm, is at most 8 u sum_a S_aa:
    |dC| <= 8 * 2^-53 * trace(sum e e^T).
The Jacobi sweeps are backward stable: 8 sweeps of 3 rotations, each touching an entry with at most 8 roundings, stay within
192 u |C|_2 <= 256 * 2^-53 * lambda2 (the allowance of cloud_normals_common.py, which grants 1024 * 2^-52 for sums and solver
together).  Davis-Kahan turns both into an angle, Weyl into an eigenvalue:
    sin(angle) <= 2 (|dC| + |dJ|) / (lambda1 - lambda0) + 4 u        (4 u: the final normalisation)
    |d lambda0| <= |dC| + |dJ|,  so  |d rms| <= sqrt((|dC| + |dJ|) / c) * 2^-20 + 4 u rms      (|sqrt a - sqrt b| <= sqrt |a - b|)
    |d centroid_a| <= 4 u (|Q(seed_a)| + |m_a|) * 2^-20          (conversion, division, sum; the scale is a power of two)
    |d d| <= |centroid| * sin-bar + sum_a |d centroid_a| + 4 u |centroid|
with lambda and the sums taken from the extended-precision evaluation of the exact integer sums (plane_segments_reference.
plane_extended)."""
import functools
import math

import numpy as np

import plane_segments_reference as pr

U = 2.0 ** -53


# ---- the bar -------------------------------------------------------------------------------------------------------------------------
def plane_bars(sums, qseed, lam):
    """(sin bar, rms bar, centroid bars [3], d bar) of one plane from its exact sums and extended-precision eigenvalues"""
    cnt, se, see, _ = sums
    dc = 8 * U * float(see[0] + see[1] + see[2]) + 256 * U * float(lam[2])
    gap = float(lam[1] - lam[0])
    sin_bar = 2 * dc / gap + 4 * U if gap > 0 else math.inf
    rms = math.sqrt(max(float(lam[0]), 0.0) / cnt) / pr.Q
    rms_bar = math.sqrt(dc / cnt) / pr.Q + 4 * U * rms
    cen = [(float(qseed[a]) + se[a] / cnt) / pr.Q for a in range(3)]
    cen_bar = [4 * U * (abs(float(qseed[a])) + abs(se[a] / cnt)) / pr.Q for a in range(3)]
    norm = math.sqrt(sum(c * c for c in cen))
    return sin_bar, rms_bar, cen_bar, norm * sin_bar + sum(cen_bar) + 4 * U * norm


def check_planes(got, res, p32, what):
    """Holds plane records to the extended-precision answer of the exact sums of the reference result `res`; prints the largest
    fraction of each bar first.  Returns that fraction."""
    q = pr.quantise(p32)
    worst = dict(sin=0.0, rms=0.0, centroid=0.0, d=0.0)
    fails = []
    assert len(got) == len(res.planes), f"{what}: {len(got)} planes, reference {len(res.planes)}"
    for k, (g, sums) in enumerate(zip(got, res.sums)):
        seed = int(res.planes["seed"][k])
        nv, d, cen, rms, lam = pr.plane_extended(sums, q[seed])
        sin_bar, rms_bar, cen_bar, d_bar = plane_bars(sums, q[seed], lam)
        gn = np.asarray(g["normal"], np.float64)
        fr = dict(sin=float(np.linalg.norm(np.cross(gn, nv))) / sin_bar if math.isfinite(sin_bar) else 0.0,
                  rms=abs(float(g["rms"]) - rms) / rms_bar if rms_bar > 0 else float(float(g["rms"]) != rms),
                  centroid=max((abs(float(g["centroid"][a]) - cen[a]) / cen_bar[a] if cen_bar[a] > 0 else float(g["centroid"][a] != cen[a]))
                               for a in range(3)),
                  d=abs(float(g["d"]) - d) / d_bar if math.isfinite(d_bar) and d_bar > 0 else 0.0)
        if math.isfinite(sin_bar) and float(gn @ nv) <= 0:
            fails.append((k, "the normal points the other way"))
        if abs(float(np.linalg.norm(gn)) - 1.0) > 4 * U:
            fails.append((k, "the normal is not unit"))
        for key, v in fr.items():
            worst[key] = max(worst[key], v)
            if v > 1.0:
                fails.append((k, f"{key} at {v:.3g} of its bar"))
    print(f"{what}: {len(got)} planes, largest fraction of the bar: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not fails, f"{what}: {fails[:5]}"
    return max(worst.values())


# ---- box corner ----------------------------------------------------------------------------------------------------------------------
STEP = 0.005                       # the sampling: 5 mm, the "voxel" of the parameters below
# min_points: the k = 30 neighbourhood of a point on the step's outermost ring is a half disc of about 4.4 samples = 22 mm, which
# reaches the face 20 mm beneath, so that ring (60 of the 256 points) and up to three more points per corner carry blended normals and
# fall to the curvature bound; 14 x 14 - 12 = 184 are left at the least.  150 keeps the step a candidate with room for noise.
BOX_PARAMS = pr.Params(radius=2.5 * STEP, min_cos=math.cos(math.radians(10.0)), max_offset=STEP, max_curvature=0.05, min_points=150,
                       max_rms=0.5 * STEP)
BOX_VIEWPOINT = np.array([[0.3, 0.3, 0.3]])


def _grid(nu, nv):
    g = np.stack(np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij"), axis=-1).reshape(-1, 2)
    return (g + 0.5) * STEP


@functools.lru_cache(maxsize=None)
def box_corner(noise_mm=0.0):
    """(points f32, normals f32, curvature f32): three 40 x 40 faces of a box corner at 5 mm, a 16 x 16 step plane 2 cm above the
    face z = 0, and a quarter cylinder of 0.3 m radius that faces the corner; seeded depth noise along z, x, y; normals and
    curvature from the normal tests' fp64 k = 30 PCA reference, turned towards a viewpoint inside the corner."""
    import cloud_normals_common as cn
    f = _grid(40, 40)
    z0 = np.zeros((len(f), 1))
    faces = [np.concatenate([f, z0], axis=1), np.concatenate([z0, f], axis=1), np.concatenate([f[:, :1], z0, f[:, 1:]], axis=1)]
    s = _grid(16, 16) + 10 * STEP
    step = np.concatenate([s, np.full((len(s), 1), 0.02)], axis=1)
    a = np.pi + (np.arange(94) + 0.5) * (0.5 * np.pi / 94)
    aa, zz = np.meshgrid(a, (np.arange(40) + 0.5) * STEP, indexing="ij")
    cyl = np.stack([0.75 + 0.3 * np.cos(aa), 0.75 + 0.3 * np.sin(aa), zz], axis=-1).reshape(-1, 3)
    p = np.concatenate(faces + [step, cyl])
    if noise_mm > 0:
        p = p + np.random.default_rng(5).normal(0.0, noise_mm * 1e-3, p.shape)
    p32 = np.ascontiguousarray(p, np.float32)
    r = cn.ref(p32, 30, viewpoints=BOX_VIEWPOINT)
    out = (p32, np.ascontiguousarray(r.normals, np.float32), np.ascontiguousarray(r.curvature, np.float32))
    for arr in out:
        arr.setflags(write=False)
    return out


BOX_PARTS = dict(face_z=(0, 1600), face_x=(1600, 3200), face_y=(3200, 4800), step=(4800, 5056), cylinder=(5056, 5056 + 94 * 40))


@functools.lru_cache(maxsize=None)
def box_reference(noise_mm=0.0):
    return pr.segment_tree(*box_corner(noise_mm), BOX_PARAMS)


# ---- decision edges: exactly representable coordinates, one f32 ulp beyond each edge -----------------------------------------------
def _up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def _down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


Z = (0.0, 0.0, 1.0)
C06 = float(np.float32(0.6))           # the fp64 value of f32 0.6
CURV = float(np.float32(0.05))


def _chain(xs, nrm=Z):
    """points (x, 0, 0) with one normal"""
    return np.float32([[x, 0, 0] for x in xs]), np.float32([nrm] * len(xs))


def _lattice_zigzag(h):
    """a 4 x 4 lattice at spacing 0.25 whose z alternates +-h like a chess board: the plane z = 0 with rms h"""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 2)
    z = np.where((g[:, 0] + g[:, 1]) % 2 == 0, h, -h)
    return np.float32(np.concatenate([g * 0.25, z[:, None]], axis=1)), np.float32([Z] * 16)


def _edge_cases():
    """name -> (points, normals, curvature or None, Params, (eligible, regions, candidates, planes))"""
    base = pr.Params(radius=0.5, min_cos=0.5, max_offset=0.125, min_points=3)
    cases = {}
    # d^2 == radius^2 links; one ulp further does not
    p, n = _chain([0.0, 0.5, 1.0])
    cases["d2 on the radius"] = (p, n, None, base, (3, 1, 1, 1))
    p, n = _chain([0.0, 0.5, _up(1.0)])
    cases["d2 one ulp beyond"] = (p, n, None, base, (3, 2, 0, 0))
    p, n = _chain([0.0, 0.5, _down(1.0)])
    cases["d2 one ulp inside"] = (p, n, None, base, (3, 1, 1, 1))
    # s == min_cos links: normals (1,0,0) and (0.6,0.8,0), min_cos the fp64 value of f32 0.6; the points lie along z (offsets 0)
    pz = np.float32([[0, 0, -0.25], [0, 0, 0], [0, 0, 0.25]])
    prm = base.replace(min_cos=C06)
    cases["s on min_cos"] = (pz, np.float32([[1, 0, 0], [1, 0, 0], [0.6, 0.8, 0]]), None, prm, (3, 1, 1, 1))
    cases["s one ulp below"] = (pz, np.float32([[1, 0, 0], [1, 0, 0], [_down(0.6), 0.8, 0]]), None, prm, (3, 2, 0, 0))
    cases["s one ulp above"] = (pz, np.float32([[1, 0, 0], [1, 0, 0], [_up(0.6), 0.8, 0]]), None, prm, (3, 1, 1, 1))
    # the offset: exactly max_offset on both sides, on one side only (the other normal sees offset 0), beyond on one side
    prm = base.replace(min_cos=0.0)
    po = lambda z: np.float32([[-0.25, 0, 0], [0, 0, 0], [0.25, 0, z]])
    cases["offset on the bound, both sides"] = (po(0.125), np.float32([Z, Z, Z]), None, prm, (3, 1, 1, 1))
    cases["offset one ulp beyond, both sides"] = (po(_up(0.125)), np.float32([Z, Z, Z]), None, prm, (3, 2, 0, 0))
    cases["offset on the bound, one side"] = (po(0.125), np.float32([Z, Z, [0, 1, 0]]), None, prm, (3, 1, 1, 1))
    cases["offset one ulp beyond, one side"] = (po(_up(0.125)), np.float32([Z, Z, [0, 1, 0]]), None, prm, (3, 2, 0, 0))
    cases["offset beyond on the other side only"] = (po(0.0625), np.float32([Z, Z, [1, 0, 0]]), None, prm, (3, 2, 0, 0))
    # curvature exactly max_curvature is eligible; one ulp more, a NaN, a zero / NaN / infinite normal are not
    p, n = _chain([0.0, 0.5, 1.0, 1.5])
    prm = base.replace(max_curvature=CURV)
    cases["curvature on the bound"] = (p, n, np.float32([0, CURV, 0, 0]), prm, (4, 1, 1, 1))
    cases["curvature one ulp beyond"] = (p, n, np.float32([0, _up(CURV), 0, 0]), prm, (3, 2, 0, 0))
    cases["curvature NaN"] = (p, n, np.float32([0, np.nan, 0, 0]), prm, (3, 2, 0, 0))
    cases["curvature ignored at max_curvature 0"] = (p, n, np.float32([0, np.nan, 9, 0]), base, (4, 1, 1, 1))
    for name, bad in (("zero normal", [0, 0, 0]), ("NaN normal", [0, np.nan, 1]), ("infinite normal", [0, np.inf, 1])):
        nb = n.copy()
        nb[1] = bad
        cases[name] = (p, nb, None, base, (3, 2, 0, 0))
    # count == min_points is a candidate; one point fewer is not
    p, n = _chain([0.0, 0.5, 1.0, 1.5, 2.0])
    cases["count on min_points"] = (p, n, None, base.replace(min_points=5), (5, 1, 1, 1))
    cases["count one below min_points"] = (p, n, None, base.replace(min_points=6), (5, 1, 0, 0))
    # rms on both sides of max_rms, and max_rms = 0 (no bound); a zig-zag of +-2^-6 has rms 2^-6 about z = 0
    p, n = _lattice_zigzag(2.0 ** -6)
    prm = base.replace(radius=0.375)
    cases["rms below max_rms"] = (p, n, None, prm.replace(max_rms=2.0 ** -5), (16, 1, 1, 1))
    cases["rms above max_rms"] = (p, n, None, prm.replace(max_rms=2.0 ** -7), (16, 1, 1, 0))
    cases["max_rms 0"] = (p, n, None, prm, (16, 1, 1, 1))
    # all points coincide: a candidate whose lambda2 is 0 is no plane
    cases["coincident points"] = (np.float32([[1, 2, 3]] * 4), np.float32([Z] * 4), None, base, (4, 1, 1, 0))
    return cases


EDGE_CASES = _edge_cases()
EDGES = tuple(EDGE_CASES)


# ---- signed / unsigned ---------------------------------------------------------------------------------------------------------------
SHEET_PARAMS = pr.Params(radius=2.5 * STEP, min_cos=math.cos(math.radians(10.0)), max_offset=STEP, min_points=200)


def two_sheets():
    """a 20 x 20 sheet at z = 0 with normals +z and a 20 x 19 sheet 1 mm above it with normals -z"""
    a, b = _grid(20, 20), _grid(20, 19)
    p = np.concatenate([np.concatenate([a, np.zeros((400, 1))], axis=1), np.concatenate([b, np.full((380, 1), 0.001)], axis=1)])
    n = np.concatenate([np.tile([[0, 0, 1.0]], (400, 1)), np.tile([[0, 0, -1.0]], (380, 1))])
    return np.float32(p), np.float32(n)


# ---- union-find topologies, as points ------------------------------------------------------------------------------------------------
TOPO_PARAMS = pr.Params(radius=0.5, min_cos=0.5, max_offset=0.0625, min_points=64)
TOPOLOGIES = ("strip ascending", "strip descending", "strip permuted", "4096 strips interleaved", "hub")


@functools.lru_cache(maxsize=None)
def topology(name, strips=4096):
    """(points, normals): every coordinate is a short binary fraction, exact in f32"""
    n = 1 << 18
    if name.startswith("strip"):                                # 2^18 points 0.75 radius apart: only neighbours in the strip link
        order = dict(ascending=np.arange(n), descending=np.arange(n)[::-1], permuted=np.random.default_rng(11).permutation(n))[name.split()[1]]
        p = np.zeros((n, 3), np.float32)
        p[:, 0] = order * 0.375
    elif name == "4096 strips interleaved":                     # point j of strip s has index j * strips + s; strips 0.125 apart in z:
        j, s = np.divmod(np.arange(64 * strips), strips)        # closer than the radius, further than max_offset
        p = np.stack([j * 0.375, np.zeros(len(j)), s * 0.125], axis=1).astype(np.float32)
    elif name == "hub":                                         # 65 536 points of a 256 x 256 lattice 0.25 across: every pair within 0.354
        g = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), axis=-1).reshape(-1, 2)
        p = np.concatenate([g * 2.0 ** -10, np.zeros((len(g), 1))], axis=1).astype(np.float32)
    else:
        raise KeyError(name)
    nrm = np.tile(np.float32([Z]), (len(p), 1))
    p.setflags(write=False)
    nrm.setflags(write=False)
    return p, nrm


def topology_answer(name, strips=4096):
    """(plane_id, counts, [(count, seed)]) by reasoning: the hub's pair list (2^31) and the 4096 strips' plane list are too long for
    a reference in a test that takes seconds; test_plane_segments_reference_cpu.py holds the reasoning to the references on the
    three strips and on 128 interleaved strips."""
    n = len(topology(name, strips)[0])
    if name.startswith("strip") or name == "hub":               # one region: its label is index 0
        return np.zeros(n, np.int32), (n, 1, 1, 1), [(n, 0)]
    return (np.arange(n) % strips).astype(np.int32), (n, strips, strips, strips), [(64, s) for s in range(strips)]
