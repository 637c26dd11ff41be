"""CPU: the numpy reference of the cloud registration (tests/cloud_register_reference.py) held to things that do not share its code:
central finite differences of the residual (the Jacobian and its sign, the scale column included), scipy's cKDTree (the neighbour),
and planted poses (the whole run).  tests/test_gpu_cloud_register.py compares the GPU with this reference on the same cases.

Measured here (printed by the tests; Frobenius distance of the 4 x 4 pose to the planted one, |scale - planted|):
    closed box, point-to-plane   sigma 1: 1.4e-3          1.05: 3.6e-3, 8.8e-4      0.95: 3.6e-3, 8.0e-4     (status 1, 4-6 iterations)
    closed box, point-to-point   sigma 1: 9.3e-3          1.05: 1.0e-2, 4.0e-4      0.95: 9.9e-3, 1.2e-3     (status 0 after 15)
    moved subset                 plane 5.4e-8, point 3.1e-8 (the float32 rounding of the source), status 1 after 2 iterations
    single plane                 three directions kept in each of 4 solves; in-plane translation 6.4e-12 m, rotation about the
                                 normal 1.6e-19 rad
The box's 800 source samples pair with the nearest of 4000 OTHER samples (spacing 2.8 cm), so neither mode ends at the planted pose:
point-to-plane is millimetres away (near an edge the nearest sample lies on the next face), point-to-point a centimetre (it slides
along the faces slowly and is still moving when the default levels end)."""
import math

import numpy as np
import pytest

import cloud_register_common as cc
import cloud_register_reference as cr


@pytest.mark.parametrize("plane", [True, False])
def test_jacobian_matches_finite_differences(plane):
    """r(exp(x) T, sigma exp(x6)) of fixed correspondences against J: dr/dx_k = J_k at x = 0, all seven columns."""
    c = cc.eval_case("box_plane_scale")
    src, T, s = c["src"][:40], c["T"], c["scale"]
    w, q = cr.transform(src, T, s)
    _, idx = cr.nearest_brute(q, c["tgt"])
    y = c["tgt"][idx].astype(np.float64)
    worst = 0.0
    for n in ([c["normals"][idx].astype(np.float64)] if plane else [np.tile(np.eye(3)[a], (len(src), 1)) for a in range(3)]):
        _, J = cr.rows(n, q - y, q, w, True)
        for k in range(7):
            h = 1e-6
            x = np.zeros(7)
            x[k] = h
            fd = (cr.residuals(x, src, y, n, T, s) - cr.residuals(-x, src, y, n, T, s)) / (2 * h)
            worst = max(worst, np.abs(fd - J[:, k]).max())
    print(f"largest |finite difference - J|: {worst:.3g}")
    # central differences: h^2 / 6 times a third derivative of order |q| (1e-12) plus rounding eps |r| / h (1e-10)
    assert worst < 1e-8


@pytest.mark.parametrize("name", ["box_plane", "box_point_scale", "zero_normals", "stride", "outside_ungated", "n257"])
def test_brute_force_neighbour_is_the_kd_trees(name):
    c = cc.eval_case(name)
    a = cc.eval_ref(name)
    b = cr.evaluate(c["src"], c["tgt"], c["normals"], nearest=cr.nearest_kdtree, **cc.eval_kwargs(c))
    assert np.array_equal(a["index"], b["index"])
    for k in ("A", "b", "e", "n_corr", "n_src", "n_no_normal"):
        assert np.array_equal(a[k], b[k]), k


def test_ties_go_to_the_smaller_index_and_the_gate_is_inclusive():
    c, ref = cc.eval_case("ties"), cc.eval_ref("ties")
    w, q = cr.transform(c["src"], c["T"], 1.0)
    t = c["tgt"].astype(np.float64)
    d2 = ((t[None] - q[:, None]) ** 2).sum(axis=2)
    ties = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
    assert sorted(set(ties.tolist())) == [2, 4, 8]
    assert np.array_equal(ref["index"], np.argmax(d2 == d2.min(axis=1, keepdims=True), axis=1))
    g = cc.eval_case("gate_edge")
    assert cc.eval_ref("gate_edge")["index"].tolist() == g["expect_index"]
    assert cc.eval_ref("outside_gated")["n_corr"] == 0 and cc.eval_ref("outside_ungated")["n_corr"] == 200
    z = cc.eval_ref("zero_normals")
    assert z["n_no_normal"] > 50 and z["n_corr"] + z["n_no_normal"] == int((z["index"] >= 0).sum())
    assert cc.eval_ref("stride")["n_src"] == 167 and np.all(cc.eval_ref("stride")["index"][np.arange(500) % 3 != 0] == -1)


@pytest.mark.parametrize("name", [n for n in cc.REG_CASES if n.startswith("box_")])
def test_closed_box_recovers_pose_and_scale(name):
    c, res = cc.reg_case(name), cc.reg_ref(name)
    dT, ds = cc.truth_distance(res, c["truth"])
    print(f"{name}: pose {dT:.3g}, scale {ds:.3g}, status {res['status']}, iters {res['iters_run']}, rmse {res['rmse']:.3g}, kept {set(res['kept'])}")
    # the target's spacing is sqrt(area / n) = 2.8 cm: a few of the 800 samples fall into a hole wider than the 5 cm gate
    assert res["status"] in (0, 1) and res["fitness"] > 0.99
    # 800 samples pair with the nearest of 4000 OTHER samples (near an edge: one of the next face, with that face's normal), so the
    # run ends where those pairs balance, not at the planted pose, and a pair says nothing finer than the target's spacing about the
    # directions along the surface (point-to-point slides along the faces a fraction of the spacing per iteration, and the default
    # levels end after 15).  Bound: half the spacing for the pose, and half the spacing over the box's half diagonal (0.71 m) for
    # the scale.
    assert dT < 0.014 and ds < 0.014 / 0.71
    assert set(res["kept"]) == {7 if c["kw"]["estimate_scale"] else 6}


@pytest.mark.parametrize("name", ["subset_plane", "subset_point"])
def test_moved_subset_ends_at_the_truth(name):
    c, res = cc.reg_case(name), cc.reg_ref(name)
    dT, _ = cc.truth_distance(res, c["truth"])
    print(f"{name}: pose {dT:.3g}, status {res['status']}, iters {res['iters_run']}, rmse {res['rmse']:.3g}")
    # the source is the float32 rounding of the exactly moved points: 2^-24 relative of coordinates up to 3.5 m, 2e-7 per point
    assert res["status"] == 1 and dT < 1e-6 and res["rmse"] < 2e-7 * math.sqrt(3)


def test_single_plane_leaves_three_directions_alone():
    res = cc.reg_ref("single_plane")
    T = res["T"]
    inplane = float(np.hypot(T[0, 3], T[1, 3]))
    about_normal = abs(T[1, 0] - T[0, 1]) / 2
    print(f"single plane: kept {res['kept']}, in-plane translation {inplane:.3g} m, rotation about the normal {about_normal:.3g} rad, "
          f"t_z {T[2, 3]:.12g}, status {res['status']}")
    assert res["kept"] and set(res["kept"]) == {3}
    # below the run's own stop threshold (eps = 1e-9) a pose component has not moved by the run's own measure
    assert inplane < 1e-9 and about_normal < 1e-9
    assert abs(T[2, 3] + 0.01) < 1e-8 and res["rmse"] < 1e-8


def test_abi_struct_matches_the_header():
    import ctypes as C
    import os
    import re

    from tl3d import _cabi as abi
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tl3d.h")) as f:
        body = re.search(r"typedef struct tl3d_cloud_eval \{(.*?)\} tl3d_cloud_eval;", f.read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"[\*\[\]0-9 ]", "", d.split(None, 1)[1]) for d in (x.strip() for x in body.split(";")) if d]
    assert names == [f for f, _ in abi.CloudEval._fields_] and C.sizeof(abi.CloudEval) == (28 + 7 + 1 + 3) * 8
    assert "tl3d_cloud_evaluate" in abi.SYMBOLS and "tl3d_cloud_register" in abi.SYMBOLS
