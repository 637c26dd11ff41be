"""CPU: the numpy reference of the joint point-to-plane + photometric registration (tests/rgbd_reference.py) against things that
do not depend on it: a per-pixel loop for the intensity maps, central differences for the photometric Jacobian, the C oracle for
the geometric half, and the planted motions of the degenerate scenes for the registration as a whole."""
import numpy as np
import pytest

import icp_degenerate_common as idc
import rgbd_common as rc
import rgbd_reference as ref
import track_reference as tr


@pytest.fixture(scope="module")
def orc():
    return idc.oracle()


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_intensity_map_equals_the_per_pixel_loop(radius):
    d, bgr = rc.crafted()
    a, b = ref.intensity_map(d, bgr, radius, rc.JUMP), ref.intensity_map_brute(d, bgr, radius, rc.JUMP)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    flag = a[..., 3]
    assert set(np.unique(flag)) == {0.0, 1.0, 2.0}
    assert (a[flag == 0] == 0).all() and (a[flag == 1][:, 1:3] == 0).all()
    # the step beyond the jump separates: a pixel beside it is flagged 1, its S averages its own side only (radius 0: itself)
    assert flag[7, 11] == 1 and flag[7, 12] == 1 and flag[14, 5] == 2 and flag[14, 6] == 2
    assert (a[..., 0] >= 0).all() and (a[..., 0] <= 255 * 256 / 65280.0).all()


def _jacobian_check(s0, plus, minus, h, J):
    """per twist component k: (share of the photometric correspondences whose association is stable under +-h, worst
    |central difference - J[k]| / |J| over them)"""
    out = []
    norm = np.linalg.norm(J, axis=0)
    for k in range(6):
        stable = s0["photo"]
        for s in (plus[k], minus[k]):
            stable = stable & s["qualified"] & (s["ut"] == s0["ut"]) & (s["vt"] == s0["vt"])
        cd = (plus[k]["ri"] - minus[k]["ri"]) / (2 * h)
        out.append((stable.sum() / s0["photo"].sum(), float((np.abs(cd - J[k])[stable] / norm[stable]).max())))
    return out


def test_photometric_jacobian_is_the_derivative_of_the_residual(orc):
    """fixes the sign and the [omega, v] order of J_I: T <- exp(x) T moves r_I by J_I . x"""
    h = 1e-4
    f = rc.pairs()["control"]
    m = rc.maps(orc, "control", 0)
    kw = dict(stride=2, max_dist=0.1, photo_gate=rc.GATE, dtype=ref.F64, detail=True)
    T = f["T_init"]
    s0 = ref.sums(rc.CAM, *m, T, **kw)
    assert s0["n_photo"] > 500
    plus = [ref.sums(rc.CAM, *m, tr.se3_apply(h * e, T), **kw) for e in np.eye(6)]
    minus = [ref.sums(rc.CAM, *m, tr.se3_apply(-h * e, T), **kw) for e in np.eye(6)]
    J = s0["J_p"]
    for share, worst in _jacobian_check(s0, plus, minus, h, J):
        assert share >= 0.9
        assert worst <= 1e-5
    # mutants: rotation and translation swapped, the sign flipped
    for mutant in (np.concatenate([J[3:], J[:3]]), -J):
        assert max(w for _, w in _jacobian_check(s0, plus, minus, h, mutant)) > 1e-2


@pytest.mark.parametrize("name", rc.NAMES)
def test_geometric_half_is_the_oracles_pass(orc, name):
    f = rc.pairs()[name]
    for stride, radius in ((1, 0), (2, 1), (3, 0)):
        m = rc.maps(orc, name, radius)
        for T in (f["T_true"], f["T_init"]):
            s = ref.sums(rc.CAM, *m, T, stride=stride, max_dist=0.1)
            so, cnt, nsrc = orc.icp_sums(m[0], m[1], T, stride=stride, max_dist=0.1)
            assert (s["n_corr"], s["n_src"]) == (cnt, nsrc)
            got = np.concatenate([s["A"], s["b"], [s["e"]]])
            assert (np.abs(got - so[:28]) <= s["n_corr"] * idc.EPS * s["abs"]).all()
            assert s["n_photo"] > 500 and s["n_photo"] <= s["n_qualified"] <= s["n_corr"]


def test_known_answers_tube_and_plane(orc):
    """the joint run recovers the motion point-to-plane cannot see; the same reference without the photometric term does not"""
    tube, plane = rc.pairs()["tube"], rc.pairs()["plane"]
    j_tube, j_plane = rc.reference_run(orc, "tube"), rc.reference_run(orc, "plane")
    g_tube, g_plane = rc.reference_run(orc, "tube", 0.0), rc.reference_run(orc, "plane", 0.0)
    e_tube, e_plane = rc.trans_err(j_tube["T"], tube)[0], rc.trans_err(j_plane["T"], plane)[0]
    print(f"joint: tube {e_tube * 1e3:.3f} mm ({j_tube['kept']} kept), plane {e_plane * 1e3:.3f} mm ({j_plane['kept']} kept); geometry only: tube "
          f"{rc.trans_err(g_tube['T'], tube)[1] * 1e3:.1f} mm along the axis ({g_tube['kept']} kept), plane {rc.trans_err(g_plane['T'], plane)[0] * 1e3:.2f} mm")
    assert e_tube <= rc.JOINT_BAR["tube"] and e_plane <= rc.JOINT_BAR["plane"]
    assert max(rc.JOINT_BAR.values()) <= 2e-3
    # the recorded reference values (rgbd_common.py) are what the reference reaches
    assert abs(e_tube - rc.REF_TUBE) <= 0.1 * rc.REF_TUBE and abs(e_plane - rc.REF_PLANE) <= 0.1 * rc.REF_PLANE
    assert j_tube["kept"] == 6 and j_plane["kept"] == 6
    assert rc.trans_err(g_tube["T"], tube)[1] >= rc.TUBE_GEO_AXIS_MIN
    assert rc.trans_err(g_plane["T"], plane)[0] > rc.PLANE_GEO_MIN
    assert g_tube["kept"] == idc.EXPECTED_KEPT["tube"] and g_plane["kept"] == idc.EXPECTED_KEPT["plane"]


def test_control_is_not_disturbed(orc):
    f = rc.pairs()["control"]
    assert rc.trans_err(rc.reference_run(orc, "control")["T"], f)[0] < 1e-4
    assert rc.trans_err(rc.reference_run(orc, "control", 0.0)["T"], f)[0] < 1e-4


def test_weight_and_cutoff_interact(orc):
    """weight 0.01 leaves the slide's eigenvalue under eig_rel * the largest: 5 directions kept, the slide stays"""
    r = rc.reference_run(orc, "tube", 0.01)
    assert r["kept"] == 5
    assert rc.trans_err(r["T"], rc.pairs()["tube"])[1] >= rc.TUBE_GEO_AXIS_MIN
