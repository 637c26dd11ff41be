"""GPU: registration of two unorganised point clouds (kernels_cloudicp.hip: tl3d_cloud_evaluate, tl3d_cloud_register; DESIGN.md
section 14) against the numpy restatement of its contract (tests/cloud_register_reference.py, held to finite differences, cKDTree and
planted poses in tests/test_cloud_register_reference_cpu.py) on the cases of tests/cloud_register_common.py.

One pass.  The indices and the counts are exact.  Every TERM of a sum is bit-identical by contract (fp64, one rounding per
operation, a stated order), so a sum differs from the reference's correctly rounded one by the order of its additions alone:
|got - ref| <= n_rows * 2^-52 * sum |term| per entry of A, b and e.
The run.  Pose (Frobenius norm of the 4 x 4 difference) and scale within the project's ICP parity bar of 1e-4 of the reference;
iters_run and status equal; the distance to a planted pose at most the reference's own plus that bar.
Measured on an MI355X: see DESIGN.md section 14 and profiles/cloud_register.txt."""
import ctypes as C

import numpy as np
import pytest

import cloud_register_common as cc
import cloud_register_reference as cr
import tl3d
from tl3d import _cabi as abi
from tl3d import metrics, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as c:
        yield c


def _evaluate(ctx, c, **over):
    kw = dict(cc.eval_kwargs(c), indices=True)
    kw.update(over)
    return ctx.cloud_evaluate(c["src"], c["tgt"], c["normals"], **kw)


def _assert_eval(got, ref, what):
    assert got["index"].dtype == np.int32 and np.array_equal(got["index"], ref["index"]), f"{what}: indices differ"
    for k in ("n_corr", "n_src", "n_no_normal"):
        assert got[k] == ref[k], f"{what}: {k} {got[k]} != {ref[k]}"
    n = ref["n_rows"]
    A = got["A"][np.triu_indices(7)]
    assert np.array_equal(got["A"], got["A"].T)
    worst = 0.0
    for name, g, r, a in (("A", A, ref["A"], ref["A_abs"]), ("b", got["b"], ref["b"], ref["b_abs"]),
                          ("e", np.array([got["e"]]), np.array([ref["e"]]), np.array([ref["e_abs"]]))):
        bound = n * 2.0 ** -52 * a
        err = np.abs(g - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert np.all(err <= bound), f"{what}: {name} off by {err.max():.3g} (bound {bound[np.argmax(err)]:.3g})"
    print(f"{what}: n_corr {got['n_corr']} of {got['n_src']}, rows {n}, largest error / bound {worst:.3g}")


# ---- one pass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.EVAL_CASES)
def test_evaluate_matches_the_reference(ctx, name):
    c, ref = cc.eval_case(name), cc.eval_ref(name)
    _assert_eval(_evaluate(ctx, c), ref, name)
    if not c.get("with_scale"):
        A = _evaluate(ctx, c)["A"]
        assert np.all(A[6] == 0) and np.all(A[:, 6] == 0)


def test_evaluate_edges_are_what_they_are_for(ctx):
    assert _evaluate(ctx, cc.eval_case("gate_edge"))["index"].tolist() == cc.eval_case("gate_edge")["expect_index"]
    assert _evaluate(ctx, cc.eval_case("outside_gated"))["n_corr"] == 0
    out = _evaluate(ctx, cc.eval_case("outside_ungated"))
    assert out["n_corr"] == 200 and np.all(out["index"] >= 0)
    z = _evaluate(ctx, cc.eval_case("zero_normals"))
    assert z["n_no_normal"] > 50
    one = _evaluate(ctx, cc.eval_case("one_target"))
    assert np.all(one["index"] == 0) and one["n_corr"] == 500
    s = _evaluate(ctx, cc.eval_case("stride"))
    assert s["n_src"] == 167 and np.all(s["index"][np.arange(500) % 3 != 0] == -1)
    big = _evaluate(ctx, cc.eval_case("big"))
    assert big["n_src"] == cc.REDUCE_THREADS + 37


def test_evaluate_empty_sets(ctx):
    c = cc.eval_case("box_plane")
    none = np.zeros((0, 3), np.float32)
    out = ctx.cloud_evaluate(c["src"], none, None, indices=True)
    assert out["n_corr"] == 0 and out["n_src"] == 500 and out["e"] == 0 and not out["A"].any() and not out["b"].any()
    assert np.all(out["index"] == -1) and len(out["index"]) == 500
    out = ctx.cloud_evaluate(none, c["tgt"], c["normals"], indices=True)
    assert out["n_corr"] == 0 and out["n_src"] == 0 and not out["A"].any() and len(out["index"]) == 0
    res = ctx.register_clouds(none, c["tgt"], c["normals"], T_init=c["T"], scale_init=1.5)
    assert res["status"] == 2 and np.array_equal(res["T"], c["T"]) and res["scale"] == 1.5 and res["n_corr"] == 0
    res = ctx.register_clouds(c["src"], none, T_init=c["T"])
    assert res["status"] == 2 and np.array_equal(res["T"], c["T"]) and res["iters_run"] == 0


# ---- against tested code -------------------------------------------------------------------------------------------------------
def test_evaluate_agrees_with_nearest_points_and_distance_summary(ctx):
    c = cc.eval_case("box_point")
    src = cc.move(c["src"], c["T"], c["scale"])               # near the target, and the pose of the call is the identity
    for max_dist in (0.03, None):
        out = ctx.cloud_evaluate(src, c["tgt"], None, max_dist=max_dist, indices=True)
        d, i = ctx.nearest_points(src, c["tgt"], max_dist=max_dist)
        assert np.array_equal(out["index"], i)
        s = ctx.distance_summary(d)
        assert s["within"] == out["n_corr"] and 0 < out["n_corr"] <= 500
        # both are sums of n_corr squared distances whose terms agree to a few roundings: the summation-order bound over n_corr terms
        assert abs(out["e"] - s["sum_sq"]) <= out["n_corr"] * 2.0 ** -52 * s["sum_sq"]


# ---- the same bytes ------------------------------------------------------------------------------------------------------------
def _variants(ctx, tgt):
    cell = cc.default_cell(tgt)
    for order in (True, False):
        ctx.set_nearest_query_order(order)
        for cs in (None, 0.5 * cell, 4 * cell):
            yield f"cell {cs}, cell order {order}", cs
    ctx.set_nearest_query_order(True)


@pytest.mark.parametrize("name", ["box_plane_scale", "box_point", "ties", "stride", "outside_ungated"])
def test_evaluate_gives_the_same_bytes(ctx, name):
    import torch
    c = cc.eval_case(name)
    first = _evaluate(ctx, c)
    again = _evaluate(ctx, c)
    assert again["raw"] == first["raw"] and np.array_equal(again["index"], first["index"]), "a second run differs"
    try:
        for what, cs in _variants(ctx, c["tgt"]):
            got = _evaluate(ctx, c, cell_size=cs)
            assert got["raw"] == first["raw"] and np.array_equal(got["index"], first["index"]), what
    finally:
        ctx.set_nearest_query_order(True)
    dev = [None if a is None else torch.from_numpy(a).cuda() for a in (c["src"], c["tgt"], c["normals"])]
    got = ctx.cloud_evaluate(*dev, **dict(cc.eval_kwargs(c), indices=True))
    assert got["raw"] == first["raw"] and got["index"].is_cuda and np.array_equal(got["index"].cpu().numpy(), first["index"])


def _result_bytes(r):
    return (np.asarray(r["T"]).tobytes(), r["scale"], r["fitness"], r["rmse"], r["n_corr"], r["n_src"], r["iters_run"], r["status"])


@pytest.mark.parametrize("name", ["box_plane_1.05", "box_point_1.0"])
def test_register_gives_the_same_bytes(ctx, name):
    import torch
    c = cc.reg_case(name)
    first = _result_bytes(ctx.register_clouds(c["src"], c["tgt"], c["normals"], **c["kw"]))
    assert _result_bytes(ctx.register_clouds(c["src"], c["tgt"], c["normals"], **c["kw"])) == first, "a second run differs"
    try:
        for what, cs in _variants(ctx, c["tgt"]):
            assert _result_bytes(ctx.register_clouds(c["src"], c["tgt"], c["normals"], cell_size=cs, **c["kw"])) == first, what
    finally:
        ctx.set_nearest_query_order(True)
    dev = [None if a is None else torch.from_numpy(a).cuda() for a in (c["src"], c["tgt"], c["normals"])]
    assert _result_bytes(ctx.register_clouds(*dev, **c["kw"])) == first


# ---- the run -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.REG_CASES)
def test_register_matches_the_reference(ctx, name):
    c, ref = cc.reg_case(name), cc.reg_ref(name)
    got = ctx.register_clouds(c["src"], c["tgt"], c["normals"], **c["kw"])
    dT, ds = float(np.linalg.norm(got["T"] - ref["T"])), abs(got["scale"] - ref["scale"])
    print(f"{name}: |T - T_ref|_F {dT:.3g}, |scale - scale_ref| {ds:.3g}, status {got['status']}, iters {got['iters_run']}, "
          f"n_corr {got['n_corr']} (ref {ref['n_corr']}), rmse {got['rmse']:.6g} (ref {ref['rmse']:.6g})")
    assert dT <= cc.PARITY and ds <= cc.PARITY
    assert got["iters_run"] == ref["iters_run"] and got["status"] == ref["status"]
    assert got["n_corr"] == ref["n_corr"] and got["n_src"] == ref["n_src"]
    assert abs(got["rmse"] - ref["rmse"]) <= cc.PARITY and abs(got["fitness"] - ref["fitness"]) <= 1e-12
    if c["truth"] is not None:
        (gT, gs), (rT, rs) = cc.truth_distance(got, c["truth"]), cc.truth_distance(ref, c["truth"])
        assert gT <= rT + cc.PARITY and gs <= rs + cc.PARITY
    if name.startswith("subset"):
        assert got["status"] == 1, "the moved subset converges early"
    if name == "single_plane":
        T = got["T"]
        rin, rab = float(np.hypot(ref["T"][0, 3], ref["T"][1, 3])), abs(ref["T"][1, 0] - ref["T"][0, 1]) / 2
        assert np.hypot(T[0, 3], T[1, 3]) <= rin + cc.PARITY and abs(T[1, 0] - T[0, 1]) / 2 <= rab + cc.PARITY


def test_register_status_paths(ctx):
    c = cc.reg_case("box_plane_1.0")
    T0 = cc.pose((0, 0, 1), 1.0, (0.3, 0.0, 0.0))              # 30 cm off: nothing within a millimetre
    tight = dict(iters=5, stride=1, max_dist=1e-3)
    res = ctx.register_clouds(c["src"], c["tgt"], c["normals"], T_init=T0, levels=[tight])
    ref = cr.register(c["src"], c["tgt"], c["normals"], T_init=T0, levels=[tight])
    assert ref["status"] == 2 and ref["n_corr"] < 6
    assert res["status"] == 2 and np.array_equal(res["T"], T0) and res["iters_run"] == 0 and res["n_corr"] == ref["n_corr"]
    # two levels, the first fails: the second never runs
    res = ctx.register_clouds(c["src"], c["tgt"], c["normals"], T_init=T0, levels=[tight, dict(iters=5, stride=1, max_dist=1.0)])
    assert res["status"] == 2 and np.array_equal(res["T"], T0) and res["iters_run"] == 0 and res["n_src"] == 800
    # ... and where the first level does its work the second starts from its pose
    lv = [dict(iters=3, stride=4, max_dist=0.2), dict(iters=2, stride=1, max_dist=0.05)]
    res = ctx.register_clouds(c["src"], c["tgt"], c["normals"], levels=lv)
    ref = cr.register(c["src"], c["tgt"], c["normals"], levels=lv)
    assert res["status"] == ref["status"] and res["iters_run"] == ref["iters_run"] <= 2 and res["n_src"] == 800
    assert np.linalg.norm(res["T"] - ref["T"]) <= cc.PARITY


def test_align_clouds_moves_the_cloud(ctx):
    c = cc.reg_case("subset_plane")
    res, moved = metrics.align_clouds(ctx, c["src"], c["tgt"], c["normals"], **c["kw"])
    assert moved.dtype == np.float32 and np.array_equal(moved, cc.move(c["src"], res["T"], res["scale"]))
    assert np.abs(moved - c["tgt"][::5]).max() < 1e-6


# ---- what the calls refuse -------------------------------------------------------------------------------------------------------
def _raw_evaluate(ctx, h, src, n_src, tgt, n_tgt, nrm, T, scale, stride, out, index):
    return ctx._lib.tl3d_cloud_evaluate(h, abi.ptr(src), n_src, abi.ptr(tgt), n_tgt, abi.ptr(nrm), abi.ptr(T), scale, stride, 0.05, 0.0, 0,
                                        None if out is None else C.byref(out), abi.ptr(index))


def _raw_register(ctx, h, src, n_src, tgt, n_tgt, nrm, T, scale, levels, n_levels, out):
    lv = (abi.IcpParams * 8)()
    for i, kw in enumerate(levels or ()):
        lv[i] = abi.IcpParams(int(kw.get("iters", 3)), int(kw.get("stride", 1)), float(kw.get("max_dist", 0.05)), 1e-6, 1e-9, 1e-4, 0, 0)
    return ctx._lib.tl3d_cloud_register(h, abi.ptr(src), n_src, abi.ptr(tgt), n_tgt, abi.ptr(nrm), abi.ptr(T), scale,
                                        lv if levels is not None else None, n_levels, 0.0, None if out is None else C.byref(out))


def test_argument_validation(ctx):
    c = cc.eval_case("box_plane")
    src, tgt, nrm, T = c["src"], c["tgt"], c["normals"], np.ascontiguousarray(c["T"])
    ev, rs = abi.CloudEval(), abi.IcpResult()
    C.memset(C.byref(ev), 0xAB, C.sizeof(ev))
    C.memset(C.byref(rs), 0xAB, C.sizeof(rs))
    ev0, rs0 = bytes(ev), bytes(rs)
    index = np.full(len(src), -7, np.int32)
    h = ctx._h
    bad_T = T.copy()
    bad_T[1, 2] = np.nan
    one = [dict()]
    e = lambda **k: _raw_evaluate(ctx, **dict(dict(h=h, src=src, n_src=len(src), tgt=tgt, n_tgt=len(tgt), nrm=nrm, T=T, scale=1.0, stride=1,
                                                   out=ev, index=index), **k))
    r = lambda **k: _raw_register(ctx, **dict(dict(h=h, src=src, n_src=len(src), tgt=tgt, n_tgt=len(tgt), nrm=nrm, T=T, scale=1.0, levels=one,
                                                   n_levels=1, out=rs), **k))
    for what, kw in (("null ctx", dict(h=None)), ("null source", dict(src=None)), ("null target", dict(tgt=None)), ("null pose", dict(T=None)),
                     ("null out", dict(out=None)), ("negative n_src", dict(n_src=-1)), ("negative n_tgt", dict(n_tgt=-1)),
                     ("n_tgt 2^31", dict(n_tgt=1 << 31)), ("a NaN in T", dict(T=bad_T)), ("an infinite scale", dict(scale=float("inf")))):
        assert e(**kw) == abi.E_INVALID, f"evaluate, {what}"
        assert r(**kw) == abi.E_INVALID, f"register, {what}"
    assert e(stride=0) == abi.E_INVALID
    for what, kw in (("stride 0", dict(levels=[dict(stride=0)])), ("n_levels 0", dict(n_levels=0)), ("n_levels 5", dict(levels=[dict()] * 5, n_levels=5)),
                     ("null levels", dict(levels=None)), ("iters -1", dict(levels=[dict(iters=-1)])), ("max_dist 0", dict(levels=[dict(max_dist=0.0)]))):
        assert r(**kw) == abi.E_INVALID, f"register, {what}"
    # a non-finite coordinate: found by the bounds pass on the device, nothing written
    for which in ("src", "tgt"):
        a = (src if which == "src" else tgt).copy()
        a[len(a) // 2, 1] = np.inf
        assert e(**{which: a}) == abi.E_INVALID and b"non-finite" in ctx._lib.tl3d_last_error()
        assert r(**{which: a}) == abi.E_INVALID
    assert bytes(ev) == ev0 and bytes(rs) == rs0 and np.all(index == -7), "a refused call wrote something"
    assert e() == abi.OK and ev.n_src == len(src) and r() == abi.OK and rs.status in (0, 1)


def test_refused_while_a_batch_is_uncollected():
    cam = dict(width=64, height=48, fx=56.0, fy=56.0, cx=31.5, cy=23.5)
    scene = synth.object_scene()
    frames = [synth.render(scene, p, **cam) for p in synth.orbit_poses(2, 1.0, 1.5)]
    c = cc.eval_case("box_plane")
    with tl3d.FusionContext(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], n_slots=2) as fc:
        for i, (d, col) in enumerate(frames):
            fc.upload(i, d, col)
            fc.build_normals(i)
        fc.icp_batch_enqueue([(0, 1)], [dict(iters=2, stride=2, max_dist=0.1)])
        for call in (lambda: fc.cloud_evaluate(c["src"], c["tgt"], c["normals"]), lambda: fc.register_clouds(c["src"], c["tgt"], c["normals"]),
                     lambda: fc.cloud_evaluate(c["src"], np.zeros((0, 3), np.float32))):
            with pytest.raises(abi.Tl3dError) as err:
                call()
            assert err.value.code == abi.E_STATE
        fc.icp_batch_collect()
        assert fc.cloud_evaluate(c["src"], c["tgt"], c["normals"])["n_src"] == 500
