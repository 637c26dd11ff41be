"""CPU: the conditions that keep tests/test_gpu_icp_degenerate.py honest, checked with the references alone (the C oracle and the
numpy solve of tests/track_reference.py; tests/icp_degenerate_common.py): every case has a hole around the eigenvalue cutoff, the
spectra have the shape the cases are named for, the bound of a step is a small fraction of the step, four wrong solves miss it by
more than 100 times, the C oracle keeps it, and the count gates gate."""
import numpy as np
import pytest

import icp_degenerate_common as dc
import track_reference as tr


@pytest.fixture(scope="module")
def orc():
    return dc.oracle()


@pytest.fixture(scope="module")
def steps(orc):
    """every reference step, once: (name, stride, radius, sim3) -> reference_step; (track name, stride) -> track_reference_step"""
    out = {c: dc.reference_step(orc, *c) for c in dc.combos()}
    for stride in dc.STRIDES:
        out[("pixels6", stride, 0, False)] = dc.reference_step(orc, "pixels6", stride, 0)
        for name in dc.LEAK_START:
            out[("leak", name, stride)] = dc.reference_step(orc, name, stride, 0, T=dc.pair_frames()[name]["T_leak"])
        for name in dc.TRACK_CASES:
            out[(name, stride)] = dc.track_reference_step(name, stride)
    out[("track_pixels8", 2)] = dc.track_reference_step("track_plane", 2, dc.track_pixel_depth(8))
    return out


def _prm(key):
    return dc.TRACK_PRM if str(key[0]).startswith("track") else dc.PRM


def test_no_eigenvalue_lies_near_the_cutoff(steps):
    """within a factor 2 of eig_rel * lmax, on either side: the device's sums differ from the reference's by ~1e-12 relative, so
    both keep the same directions"""
    for key, r in steps.items():
        lam, _, keep = dc.spectrum(r["M"], _prm(key)["damping"], _prm(key)["eig_rel"])
        cut = _prm(key)["eig_rel"] * lam.max()
        near = (lam > 0.5 * cut) & (lam < 2.0 * cut)
        print(key, "eigenvalues / largest:", " ".join(f"{v:.2e}" for v in lam / lam.max()), "kept", int(keep.sum()))
        assert not near.any(), (key, lam / lam.max())


def test_the_spectra_have_the_shape_the_cases_are_named_for(steps):
    for key, r in steps.items():
        lam, _, keep = dc.spectrum(r["M"])
        if key[0] in dc.PAIR_CASES:
            name, _, _, sim3 = key
            assert int(keep.sum()) == (dc.EXPECTED_KEPT_SIM3 if sim3 else dc.EXPECTED_KEPT)[name], (key, lam / lam.max())
            if name == "corridor":                                       # sliding is seen through the far wall only: kept, and weak
                assert lam.min() < 1e-2 * lam.max()
        elif key[0] == "leak":
            assert int(keep.sum()) == dc.EXPECTED_KEPT[key[1]], (key, lam / lam.max())
        elif key[0] in dc.TRACK_KEPT:
            assert int(keep.sum()) == dc.TRACK_KEPT[key[0]], (key, lam / lam.max())
        elif key[0] == "track_pixels8":
            assert int(keep.sum()) == 3, (key, lam / lam.max())


def test_the_bound_is_a_small_fraction_of_the_step(steps):
    for key, r in steps.items():
        xn = float(np.linalg.norm(r["x"]))
        print(key, f"|x| {xn:.3e}, step_bound {r['bound']:.3e} = {r['bound'] / xn:.1e} |x|, n_corr {r['n_corr']}")
        assert xn > 1e-3, key
        assert r["bound"] <= 1e-3 * xn, key
        assert r["status"] == 0 and r["iters_run"] == 1


def _mutants(r, prm):
    M, b, x = r["M"], r["b"], r["x"]
    n = len(M)
    swapped = x.copy()
    swapped[:3], swapped[3:6] = x[3:6], x[:3]
    return dict(no_cutoff=dc.solve_n(M, b, prm["damping"], prm["eig_rel"], keep=np.ones(n, bool)),
                cutoff_x100=dc.solve_n(M, b, prm["damping"], 100.0 * prm["eig_rel"]),
                sign=-x, halves_swapped=swapped)


# the cases each mutant is meant to be caught on: what it changes must matter there
MUTANT_TARGETS = dict(no_cutoff=("sphere", "cylinder", "tube"), cutoff_x100=("cylinder", "tube", "corridor"), sign=dc.PAIR_CASES,
                      halves_swapped=dc.PAIR_CASES)


def test_four_wrong_solves_miss_the_bound_by_more_than_100_times(steps):
    for mutant, targets in MUTANT_TARGETS.items():
        ratios = {key: float(np.linalg.norm(_mutants(r, _prm(key))[mutant] - r["x"])) / r["bound"] for key, r in steps.items() if key[0] in targets}
        worst = min(ratios, key=ratios.get)
        print(f"{mutant}: |x_mutant - x| / step_bound >= {ratios[worst]:.3e} (on {worst}) over {len(ratios)} cases")
        assert ratios[worst] > 100.0, (mutant, worst)
    # and on the tracking cases, the two that need nothing dropped to differ
    for name in dc.TRACK_CASES:
        for stride in dc.STRIDES:
            r = steps[(name, stride)]
            for mutant in ("sign", "halves_swapped"):
                assert np.linalg.norm(_mutants(r, dc.TRACK_PRM)[mutant] - r["x"]) > 100.0 * r["bound"], (mutant, name)


def test_the_c_oracle_keeps_the_bound(orc, steps):
    """its icp(iters=1) -- cyclic Jacobi, or LDL^T where nothing can be dropped -- against the numpy eigh solve, 6 and 7 unknowns"""
    for key in dc.combos() + [("pixels6", s, 0, False) for s in dc.STRIDES]:
        name, stride, radius, sim3 = key
        r = steps[key]
        f = dc.pair_frames()[name] if name in dc.PAIR_CASES else dc.pixel_frames()[name]
        src, nmap = dc.maps(orc, name, radius)
        o = orc.icp(src, nmap, T_init=f["T_init"], iters=1, stride=stride, estimate_scale=sim3, **dc.PRM)
        d = float(np.linalg.norm(o["T"] - r["T"]))
        ds = abs(o["scale"] - r["scale"])
        print(f"{key}: |T_oracle - T_ref| / bound = {d / r['pose_bound']:.3e}, |scale_oracle - scale_ref| / bound = {ds / dc.scale_bound(r):.3e}")
        assert d <= r["pose_bound"] and ds <= dc.scale_bound(r), key
        assert (o["status"], o["iters_run"]) == (r["status"], r["iters_run"]), key
    # tracking: track() with one iteration is the step with the camera moved by -x
    for name in dc.TRACK_CASES:
        c = dc.track_cases()[name]
        for stride in dc.STRIDES:
            r = steps[(name, stride)]
            res = tr.track(c["rec"], *dc.T_SPEC, dc.CAM, c["depth"], c["start"], [dict(dc.TRACK_PRM, iters=1, stride=stride)])
            assert np.linalg.norm(res["T"] - r["T"]) <= r["pose_bound"] and (res["status"], res["iters_run"]) == (0, 1)


def test_the_count_gates_gate(orc, steps):
    for stride in dc.STRIDES:
        for n in (5, 6):
            r = dc.reference_step(orc, f"pixels{n}", stride, 0)
            assert r["n_corr"] == n and r["n_src"] == n
            assert (r["x"] is None) == (n < 6)
    for n in (7, 8):
        r = dc.track_reference_step("track_plane", 2, dc.track_pixel_depth(n))
        assert r["n_corr"] == n and r["n_src"] == n
        assert (r["x"] is None) == (n < 8)
    assert len(set(dc.track_pixels())) == 8 and all(u % 2 == 0 and v % 2 == 0 for u, v in dc.track_pixels())


def test_the_reference_leaves_unobserved_directions_at_the_prior(orc, steps):
    """the leak bars of the GPU test: 1e-4 |x| on a plane (the bar of tests/test_track_reference_cpu.py), twice the reference's own
    leak elsewhere, which must itself be a small fraction of the step"""
    for name in dc.LEAK_CASES:
        f = dc.pair_frames()[name]
        for stride in dc.STRIDES:
            for radius in dc.RADII:
                r, bar = dc.leak_reference(orc, name, stride, radius)
                print(f"{name} stride {stride} radius {radius}: |x| {np.linalg.norm(r['x']):.3e}, reference leak {dc.leak(dc.unobserved(name, f['T_tgt']), r['x']):.3e}, "
                      f"bar {bar:.3e}")
                assert np.linalg.norm(r["x"]) > 1e-3
                assert bar < 1e-3, (name, stride, radius)
                if "plane" in name:
                    assert dc.leak(dc.unobserved(name, f["T_tgt"]), r["x"]) < bar == dc.PLANE_LEAK
    for name in dc.TRACK_CASES:
        for stride in dc.STRIDES:
            r, bar = dc.track_leak_reference(name, stride)
            print(f"{name} stride {stride}: reference leak {dc.leak(dc.track_cases()[name]['Q'], r['x']):.3e}, bar {bar:.3e}")
            assert bar < 1e-3
            if name == "track_plane":
                assert dc.leak(dc.track_cases()[name]["Q"], r["x"]) < bar == dc.PLANE_LEAK


def test_no_step_of_the_few_iteration_runs_comes_near_eps(orc):
    """every step of every run the GPU test makes (both radii, 6 and 7 unknowns, tracking) is more than 10 times FEW_EPS, so none stops
    early; and the iterated numpy reference ends where the C oracle does, far inside the parity bar the GPU test uses (1e-4)"""
    for name in dc.PAIR_CASES:
        for radius in dc.RADII:
            for sim3 in ((False, True) if name in dc.SIM3_CASES else (False,)):
                sizes, T, scale = dc.few_reference(orc, name, 2, radius, sim3)
                src, nmap = dc.maps(orc, name, radius)
                o = orc.icp(src, nmap, T_init=dc.pair_frames()[name]["T_init"], iters=dc.FEW_ITERS, stride=2, estimate_scale=sim3,
                            **dict(dc.PRM, eps=dc.FEW_EPS))
                print(name, radius, "sim3" if sim3 else "", "steps", " ".join(f"{s:.1e}" for s in sizes), f"|T_ref - T_oracle| {np.linalg.norm(T - o['T']):.2e}")
                assert all(s > 10.0 * dc.FEW_EPS for s in sizes), (name, radius, sim3)
                assert (o["status"], o["iters_run"]) == (0, dc.FEW_ITERS)
                assert np.linalg.norm(T - o["T"]) < 1e-6 and abs(scale - o["scale"]) < 1e-6
    for name in dc.TRACK_CASES:
        sizes = dc.track_few_sizes(name, 2)
        print(name, "steps", " ".join(f"{s:.1e}" for s in sizes))
        assert all(s > 10.0 * dc.FEW_EPS for s in sizes), name
        ref = dc.track_few_reference(name, 2)
        assert (ref["status"], ref["iters_run"]) == (0, dc.FEW_ITERS)
