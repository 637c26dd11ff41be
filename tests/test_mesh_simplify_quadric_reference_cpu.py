"""CPU: the restatement of the quadric placement rules (tests/mesh_simplify_quadric_reference.py) against
an exact rational solve, on meshes with known answers (a roof's crease, a cube's corner, a tilted plane) and on the edge rules;
the C-ABI call is exported, bound and refuses bad arguments without a GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import mesh_simplify_quadric_reference as mqr
import mesh_simplify_reference as msr
from mesh_simplify_quadric_common import (CARRY_FILL, CARRY_TRIS, CORNER, NO_TRIS, PLANE, ROOFS, reference, roof_crease_clusters, roof_distance)
from tl3d import _cabi as abi

LATTICE = tuple(f"roof {k}" for k in range(len(ROOFS))) + ("corner", "plane", "crease outside", "spans")
EXACT_TOL = 1e-9            # steps: 1024 eps / reg = 2.3e-10 at reg = 2^-10, times 5


def _exact(s, S, n, reg):
    """x of (M + reg I) x = reg m - g in Fractions, from the integer sums: multiplied through by T = A00 + A11 + A22,
    (A + reg T I) x = reg T m - b, by Gaussian elimination"""
    A00, A01, A02, A11, A12, A22, b0, b1, b2 = (Fraction(v) for v in s)
    reg = Fraction(reg)
    T = A00 + A11 + A22
    m = [Fraction(int(S[a]), int(n) * 16384) for a in range(3)]
    rows = [[A00 + reg * T, A01, A02, reg * T * m[0] - b0], [A01, A11 + reg * T, A12, reg * T * m[1] - b1],
            [A02, A12, A22 + reg * T, reg * T * m[2] - b2]]
    for c in range(3):
        p = next(r for r in range(c, 3) if rows[r][c] != 0)
        rows[c], rows[p] = rows[p], rows[c]
        rows[c] = [v / rows[c][c] for v in rows[c]]
        for r in range(3):
            if r != c:
                rows[r] = [v - rows[r][c] * w for v, w in zip(rows[r], rows[c])]
    return [rows[a][3] for a in range(3)], m


def _placed(info):
    return np.flatnonzero(~np.isnan(info["x"][:, 0]))


@pytest.mark.parametrize("name", LATTICE)
def test_solve_agrees_with_the_exact_rational_solve(name):
    """The fp64 solve of the reference against Fractions on the same integer sums, on the lattice of 1/1024 cell: rank 3 (corner),
    rank 2 (roofs, crease outside) and rank 1 (plane, one triangle).  Bound: 1e-9 steps = 1024 eps / reg with a margin of 5.
    Measured: roofs 1.2e-13, 1.1e-13, 5.7e-14, corner 3.4e-14, crease outside 2.5e-14, one triangle 8.3e-12, plane 2.6e-11 steps.
    The adjugate WITHOUT its refinement step gives 6.4e-10 on the one triangle and 2.5e-9 on the plane (at rank 1 the cofactors
    cancel to O(reg) and det to O(reg^2)), which is why the rules have the step."""
    _, want, _ = reference(name)
    info = want[3]
    worst = 0.0
    assert len(_placed(info))
    for c in _placed(info):
        exact, _ = _exact(info["sums"][c], info["S"][c], info["n"][c], mqr.REG)
        worst = max(worst, max(abs(float(Fraction(float(info["x"][c, a])) - exact[a])) for a in range(3)))
    print(f"{name}: {len(_placed(info))} clusters, largest |x - exact| = {worst:.3g} steps")
    assert worst <= EXACT_TOL


@pytest.mark.parametrize("k", range(len(ROOFS)))
def test_roof_crease_is_kept_by_the_quadric_and_rounded_by_the_mean(k):
    (xyz, _, _, _, _), want, mean = reference(f"roof {k}")
    crease = roof_crease_clusters(xyz, want[3]["vert_map"])
    assert len(crease) >= 3 and want[3]["corners_skipped"] == 0
    dq, dm = roof_distance(want[0][crease]), roof_distance(mean[0][crease])
    print(f"roof {ROOFS[k]}: quadric {dq.min():.4f}..{dq.max():.4f} cell, mean {dm.min():.4f}..{dm.max():.4f} cell from the crease")
    assert dq.max() <= 0.005 and dm.min() >= 0.05


def test_cube_corner_is_kept_by_the_quadric_and_rounded_by_the_mean():
    (xyz, _, _, _, _), want, mean = reference("corner")
    c = np.unique(want[3]["vert_map"][(xyz == np.array(CORNER, np.float32)).all(axis=1)])
    assert len(c) == 1
    dq = np.linalg.norm(want[0][c[0]].astype(np.float64) - CORNER)
    dm = np.linalg.norm(mean[0][c[0]].astype(np.float64) - CORNER)
    print(f"corner: quadric {dq:.4f} cell, mean {dm:.4f} cell from the corner")
    assert dq <= 0.005 and dm >= 0.1


def test_single_plane_stays_on_the_plane_and_at_the_mean_within_it():
    """One plane with unit normal u and offset e: M = u u^T, g = e u, so x = m - u (u.m + e) / (1 + reg) exactly: the in-plane part
    is the mean's, and the distance to the plane is the mean's times reg / (1 + reg).  Asserted on the rational solve (whose
    agreement with the reference is the test above), in integers: N = (-a, -b, 1) scaled."""
    (xyz, _, tris, cell, _), want, mean = reference("plane")
    info = want[3]
    assert info["quadric_placed"] == info["clusters"] and info["clamped"] == 0 and info["corners_skipped"] == 0
    nrm = [Fraction(-PLANE[0]), Fraction(-PLANE[1]), Fraction(1)]
    n2 = sum(v * v for v in nrm)
    for c in range(info["clusters"]):
        x, m = _exact(info["sums"][c], info["S"][c], info["n"][c], mqr.REG)
        # the plane seen from the cluster's cell, in steps: nrm . (p + 1024 i) = 1024 * PLANE[2]
        e = sum(nrm[a] * 1024 * int(info["cell_index"][c, a]) for a in range(3)) - Fraction(PLANE[2]) * 1024
        dist_m, dist_x = sum(nrm[a] * m[a] for a in range(3)) + e, sum(nrm[a] * x[a] for a in range(3)) + e
        assert dist_x == dist_m * Fraction(mqr.REG) / (1 + Fraction(mqr.REG))
        assert dist_m == 0 and dist_x == 0                              # the members lie on the plane, so does their mean
        assert all(x[a] - m[a] == -nrm[a] * (dist_m - dist_x) / n2 for a in range(3))         # no in-plane component
    # and in f32: both positions round one point of the lattice (the two paths differ by 1e-11 cell before that): one ulp at most
    assert (np.abs(want[0] - mean[0]) <= np.spacing(np.abs(mean[0]))).all()


def test_span_rule_is_per_corner():
    (xyz, _, tris, cell, _), want, mean = reference("spans")
    info = want[3]
    assert info["corners_skipped"] == 2 and info["quadric_placed"] == 1 and info["clusters"] == 3
    assert np.isnan(info["x"][0]).all() and np.isnan(info["x"][2]).all() and not np.isnan(info["x"][1]).any()
    assert info["sums"][0] == [0] * 9 and info["sums"][2] == [0] * 9
    for c in (0, 2):                                                    # skipped corners: the mean's bytes
        assert np.array_equal(want[0][c].view(np.uint8), mean[0][c].view(np.uint8))
    # the middle corner by hand: p seen from cell 3
    p = [np.array(v, dtype=object) for v in ((-3 * 1024 + 512, 256, 512), (512, 768, 512), (1024 + 512, 256, 768))]
    e1, e2 = p[1] - p[0], p[2] - p[0]
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    d = -sum(n[a] * p[0][a] for a in range(3))
    assert info["sums"][1] == [n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2], d * n[0], d * n[1], d * n[2]]
    # one cell further apart and nothing contributes; one cell closer and every corner does
    far = xyz.copy(); far[0, 0] -= 1.0
    near = xyz.copy(); near[0, 0] += 1.0
    assert mqr.simplify(far, None, tris, cell)[3]["corners_skipped"] == 3 and mqr.simplify(far, None, tris, cell)[3]["quadric_placed"] == 0
    assert mqr.simplify(near, None, tris, cell)[3]["corners_skipped"] == 0 and mqr.simplify(near, None, tris, cell)[3]["quadric_placed"] == 3


def test_steps_are_the_floor_division_also_below_zero_and_above_the_cell():
    """h = (q + 8192) >> 14 on values q cannot quite reach (the fp64 rounding of r leaves |q| within a step of [0, 2^24]) and
    on the ones it does"""
    q = np.array([-16385, -8193, -8192, -1, 0, 8191, 8192, (1 << 24) - 8193, (1 << 24) - 8192, 1 << 24, (1 << 24) + 8191, (1 << 24) + 8192])
    assert [int(v) for v in mqr.steps(q)] == [(int(v) + 8192) // 16384 for v in q] == [-1, -1, 0, 0, 0, 0, 1, 1023, 1024, 1024, 1024, 1025]


@pytest.mark.parametrize("name", ["axis lines 0.25", "axis lines 0.1", "axis lines 0.005", "axis lines 0.1 shifted"])
def test_vertices_one_f32_step_beside_a_cell_face(name):
    """the vertices on o + k * cell and one f32 step beside it: q = 0, q just above 0, and q just below 2^24 or 2^24 itself, which
    all round to h = 0 or h = 1024, the far face of the vertex's own cell"""
    (xyz, rgb, tris, cell, origin), want, mean = reference(name)
    i, q = msr.cells(xyz, cell, origin)
    h = mqr.steps(q)
    assert q.min() >= 0 and q.max() <= 1 << 24 and h.min() >= 0 and h.max() <= 1024
    if not name.endswith("shifted"):
        assert (q == 0).any() and ((q > (1 << 24) - 8192) & (h == 1024)).any() and ((q > 0) & (q < 8192) & (h == 0)).any()
    for a, b in zip(want[1:3], mean[1:3]):                             # colours and triangles are the mean call's
        assert np.array_equal(a, b)
    lo = np.asarray(origin or (0, 0, 0), np.float64) + want[3]["cell_index"] * float(cell)
    assert (want[0] >= np.nextafter(lo.astype(np.float32), np.float32(-np.inf))).all()
    assert (want[0] <= np.nextafter((lo + float(cell)).astype(np.float32), np.float32(np.inf))).all()


def test_clusters_without_area_follow_the_mean_rule():
    (xyz, rgb, tris, cell, _), want, mean = reference("without area")
    assert want[3]["quadric_placed"] == 0 and want[3]["clamped"] == 0 and want[3]["corners_skipped"] == 0
    for a, b in zip(want[:3], mean[:3]):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    no_tris = mqr.simplify(xyz, rgb, NO_TRIS, cell)
    assert no_tris[3]["quadric_placed"] == 0 and np.array_equal(no_tris[0].view(np.uint8), mean[0].view(np.uint8))


def test_crease_outside_the_cell_is_clamped_and_counted():
    (xyz, _, tris, cell, _), want, mean = reference("crease outside")
    info = want[3]
    c = info["vert_map"][0]
    assert info["vert_map"][3] == c and info["clamped"] == 1 and info["quadric_placed"] == info["clusters"]
    # the planes meet at x = -0.5, z = 0.25, at 27 degrees: the pull towards the mean, 1.1 cells away, is visible but small
    assert info["x"][c, 0] < -400.0 and abs(info["x"][c, 2] - 256.0) < 50.0
    assert want[0][c, 0] == 0.0 and 0.0 <= want[0][c, 1] <= 1.0 and abs(want[0][c, 2] - 0.25) < 0.05
    assert (want[0] >= info["cell_index"]).all() and (want[0] <= info["cell_index"] + 1).all()


def test_reg_outside_its_range_is_rejected():
    (xyz, _, tris, cell, _), _, _ = reference("spans")
    for reg in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mqr.simplify(xyz, None, tris, cell, reg=reg)
    assert mqr.simplify(xyz, None, tris, cell, reg=1.0)[3]["quadric_placed"] == 1


def test_carry_case_wraps_the_low_words_and_changes_sign():
    """what makes the GPU's carry case a carry case: on the one hot record the terms d N_a, in input order, wrap a 64-bit low word
    thousands of times and take every running sum below zero and back"""
    (xyz, rgb, tris, cell, _), want, _ = reference("carry")
    info = want[3]
    assert len(tris) == CARRY_TRIS and len(xyz) == 3 * CARRY_TRIS + CARRY_FILL
    hot = info["vert_map"][-1]
    assert info["n"][hot] == CARRY_FILL + CARRY_TRIS
    i, q = msr.cells(xyz, cell)
    h = mqr.steps(q)
    running, wraps, changes, biggest = [0, 0, 0], 0, [0, 0, 0], 0
    for t in tris.astype(np.int64):
        k = [j for j in range(3) if info["vert_map"][t[j]] == hot]
        assert len(k) == 1
        p = [[int((i[t[j], a] - i[t[k[0]], a]) * 1024 + h[t[j], a]) for a in range(3)] for j in range(3)]
        e1, e2 = [p[1][a] - p[0][a] for a in range(3)], [p[2][a] - p[0][a] for a in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        d = -sum(n[a] * p[0][a] for a in range(3))
        for a in range(3):
            lo_before = running[a] & 0xFFFFFFFFFFFFFFFF
            running[a] += d * n[a]
            wraps += 1 if (lo_before + ((d * n[a]) & 0xFFFFFFFFFFFFFFFF)) >> 64 else 0
            changes[a] += 1 if (running[a] < 0) != (running[a] - d * n[a] < 0) else 0
            biggest = max(biggest, abs(d * n[a]))
    print(f"carry: {wraps} wraps, sign changes {changes}, largest term 2^{np.log2(float(biggest)):.1f}")
    assert running == info["sums"][hot][6:] and wraps >= 1000 and min(changes) >= 4 and biggest >= 1 << 56
    assert info["corners_skipped"] == 0 and info["quadric_placed"] > 1


# ---- the C-ABI without a GPU --------------------------------------------------------------------------------------------------
def test_call_is_exported_and_bound():
    lib = abi.load()
    assert "tl3d_mesh_simplify_quadric" in abi.SYMBOLS and hasattr(lib, "tl3d_mesh_simplify_quadric")
    assert len(lib.tl3d_mesh_simplify_quadric.argtypes) == 22 and lib.tl3d_mesh_simplify_quadric.restype is C.c_int
    assert lib.tl3d_mesh_simplify_quadric.argtypes[8] is C.c_double                  # reg, behind the origin
    assert len(lib.tl3d_mesh_simplify_clusters.argtypes) == 18


def test_argument_validation_needs_no_gpu():
    """every check but the two scans is decided before the first device call: made with a null context, which is refused last"""
    lib = abi.load()
    tris = np.array([[0, 1, 2], [2, 3, 4]], np.uint32)
    xyz, rgb = np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8)
    oxyz, orgb, otri, vmap = np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8), np.zeros((2, 3), np.uint32), np.zeros(5, np.uint32)
    counts = [C.c_int64(-7) for _ in range(7)]

    def call(**kw):
        a = dict(xyz=xyz, n_vert=5, tri=tris, n_tri=2, cell=0.5, origin=None, reg=2.0 ** -10, oxyz=oxyz, vcap=5, otri=otri, tcap=2,
                 vmap=vmap, counts=[C.byref(c) for c in counts])
        a.update(kw)
        o = None if a["origin"] is None else (C.c_double * 3)(*a["origin"])
        rc = lib.tl3d_mesh_simplify_quadric(None, abi.ptr(a["xyz"]), abi.ptr(rgb), a["n_vert"], abi.ptr(a["tri"]), a["n_tri"], a["cell"], o,
                                            a["reg"], abi.ptr(a["oxyz"]), abi.ptr(orgb), a["vcap"], abi.ptr(a["otri"]), a["tcap"],
                                            abi.ptr(a["vmap"]), *a["counts"])
        return rc, lib.tl3d_last_error()
    short = [C.byref(c) for c in counts[:6]] + [None]
    for kw, msg in ((dict(n_tri=-2), b"negative size"), (dict(n_vert=1 << 31), b"2^31"), (dict(vcap=-1), b"negative capacity"),
                    (dict(counts=short), b"null argument"), (dict(cell=0.0), b"cell size"), (dict(origin=(0.0, float("nan"), 0.0)), b"origin"),
                    (dict(reg=0.0), b"reg"), (dict(reg=-1.0), b"reg"), (dict(reg=1.5), b"reg"), (dict(reg=float("nan")), b"reg"),
                    (dict(reg=float("inf")), b"reg"), (dict(xyz=None), b"null vertex list"), (dict(tri=None), b"null triangle list"),
                    (dict(oxyz=None), b"null output"), (dict(oxyz=xyz), b"aliases"), (dict(otri=tris), b"aliases"),
                    (dict(vmap=tris.reshape(-1)[1:]), b"aliases"), (dict(), b"null ctx"), (dict(reg=1.0), b"null ctx"),
                    (dict(reg=5e-324), b"null ctx")):
        rc, err = call(**kw)
        assert rc == abi.E_INVALID and msg in err, (kw.keys(), err)
    assert [c.value for c in counts] == [-7] * 7 and not oxyz.any() and not otri.any() and not vmap.any()       # nothing written
