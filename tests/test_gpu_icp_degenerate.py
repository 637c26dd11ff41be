"""GPU: the solve at the end of every registration -- solve6_direct, the cross-lane Jacobi solve6_wave, the one-lane Sim(3) solve
(reg_solve.h), reached through icp, icp_batch and track -- on geometry that leaves some motion unobserved: planes, a sphere,
a cylinder, an open tube, a corridor, six pixels.  Single update steps against the fp64 reference of
tests/icp_degenerate_common.py within the bound derived there (tests/test_icp_degenerate_reference_cpu.py checks, with the
references alone, the conditions under which that bound means something); unobserved directions; a few iterations against the
existing parity bar; the count gates; repeatability.  Every comparison prints measured / bound."""
import numpy as np
import pytest

import icp_degenerate_common as dc
import tl3d

pytestmark = pytest.mark.gpu

SLOT = {name: (2 * i, 2 * i + 1) for i, name in enumerate(dc.PAIR_CASES)}        # (source, target)
SLOT["pixels5"] = (2 * len(dc.PAIR_CASES), SLOT["control"][1])
SLOT["pixels6"] = (2 * len(dc.PAIR_CASES) + 1, SLOT["control"][1])
N_SLOTS = 2 * len(dc.PAIR_CASES) + 2


@pytest.fixture(scope="module")
def orc():
    return dc.oracle()


@pytest.fixture(scope="module")
def ctxs():
    """smoothing radius -> a context that holds every pair's frames and their normal maps"""
    out = {}
    frames = dict(dc.pair_frames(), **dc.pixel_frames())
    for radius in dc.RADII:
        ctx = tl3d.FusionContext(dc.W, dc.H, dc.CAM["fx"], dc.CAM["fy"], dc.CAM["cx"], dc.CAM["cy"], n_slots=N_SLOTS, grid=None)
        ctx.set_normal_smoothing(radius)
        for name, (s, t) in SLOT.items():
            ctx.upload(s, frames[name]["src"], None)
            if name in dc.PAIR_CASES:
                ctx.upload(t, frames[name]["tgt"], None)
        for slot in range(N_SLOTS):
            ctx.build_normals(slot)
        out[radius] = ctx
    yield out
    for ctx in out.values():
        ctx.close()


def _level(stride, sim3=False):
    return dict(dc.PRM, iters=1, stride=stride, estimate_scale=sim3)


def _both_routes(ctx, name, T_init, level):
    """the per-iteration kernel and the batched one, from the same start"""
    s, t = SLOT[name]
    one = ctx.icp(s, t, T_init=T_init, scale_src=1.0, **level)
    batch = ctx.icp_batch([(s, t)], [level], T_init=[T_init], scales=[1.0])[0]
    return (("icp", one), ("icp_batch", batch))


def _check_step(ctx, name, stride, res, ref, what):
    d = float(np.linalg.norm(res["T"] - ref["T"]))
    ds = abs(res["scale"] - ref["scale"])
    print(f"{what}: |T - T_ref| {d:.3e} / {ref['pose_bound']:.3e} = {d / ref['pose_bound']:.3e}; |scale - scale_ref| {ds:.3e} / "
          f"{dc.scale_bound(ref):.3e} = {ds / dc.scale_bound(ref):.3e}; n_corr {ref['n_corr']}")
    assert d <= ref["pose_bound"], what
    assert ds <= dc.scale_bound(ref), what
    assert (res["status"], res["iters_run"]) == (ref["status"], ref["iters_run"]), what
    s, t = SLOT[name]
    ev = ctx.icp_evaluate([(s, t)], [res["T"]], stride=stride, max_dist=dc.PRM["max_dist"], scales=[res["scale"]])[0]
    assert (res["n_corr"], res["n_src"]) == (ev["n_corr"], ev["n_src"]), what


@pytest.mark.parametrize("radius", dc.RADII)
def test_one_step_matches_the_reference_on_every_pairwise_route(ctxs, orc, radius):
    ctx = ctxs[radius]
    for name, stride, r, sim3 in dc.combos():
        if r != radius:
            continue
        ref = dc.reference_step(orc, name, stride, radius, sim3)
        assert ref["status"] == 0 and np.linalg.norm(ref["x"]) > 1e-3
        for route, res in _both_routes(ctx, name, dc.pair_frames()[name]["T_init"], _level(stride, sim3)):
            _check_step(ctx, name, stride, res, ref, f"{route} {name} stride {stride} radius {radius}{' Sim(3)' if sim3 else ''}")
            if not sim3:
                assert res["scale"] == 1.0


def _track_ctx(sparse, n_slots=1):
    spec = tl3d.GridSpec(dc.T_DIMS, dc.T_ORIGIN, dc.T_VOXEL, dc.T_TRUNC, tl3d.CH_TSDF, pool_tsdf=dc.T_DIMS[0] * dc.T_DIMS[1] * dc.T_DIMS[2] // 512 if sparse else 0)
    return tl3d.FusionContext(dc.W, dc.H, dc.CAM["fx"], dc.CAM["fy"], dc.CAM["cx"], dc.CAM["cy"], n_slots=n_slots, grid=spec)


def _track_level(stride):
    return dict(dc.TRACK_PRM, iters=1, stride=stride)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("name", dc.TRACK_CASES)
def test_one_tracking_step_matches_the_reference(name, sparse):
    c = dc.track_cases()[name]
    with _track_ctx(sparse) as ctx:
        ctx.upload_grid(tl3d.CH_TSDF, c["rec"])
        ctx.upload(0, c["depth"], None)
        for stride in dc.STRIDES:
            ref = dc.track_reference_step(name, stride)
            assert ref["status"] == 0 and np.linalg.norm(ref["x"]) > 1e-3
            res = ctx.track(0, c["start"], [_track_level(stride)])
            d = float(np.linalg.norm(res["T"] - ref["T"]))
            print(f"track {name} stride {stride}: |T - T_ref| {d:.3e} / {ref['pose_bound']:.3e} = {d / ref['pose_bound']:.3e}; n_corr {ref['n_corr']}")
            assert d <= ref["pose_bound"]
            assert (res["status"], res["iters_run"]) == (ref["status"], ref["iters_run"])
            ev = ctx.track_evaluate(0, res["pose"], stride=stride, max_dist=dc.TRACK_PRM["max_dist"])
            assert (res["n_corr"], res["n_src"]) == (ev["n_corr"], ev["n_src"])
            # the update's components along what the volume does not observe (camera frame of the start; the camera moved by -x)
            _, bar = dc.track_leak_reference(name, stride)
            leak = dc.leak(c["Q"], dc.step_of(res["T"], c["T0"]))
            print(f"track {name} stride {stride}: leak {leak:.3e} / {bar:.3e} = {leak / bar:.3e}")
            assert leak <= bar


def test_unobserved_directions_stay_at_the_prior(ctxs, orc):
    """plane: in-plane translations, rotation about the normal; sphere: rotations about its centre; cylinder: spin about and slide
    along its axis; tube: slide along its axis.  The bars are the reference's (icp_degenerate_common.leak_reference)."""
    for name in dc.LEAK_CASES:
        f = dc.pair_frames()[name]
        Q = dc.unobserved(name, f["T_tgt"])
        for stride in dc.STRIDES:
            for radius in dc.RADII:
                ref, bar = dc.leak_reference(orc, name, stride, radius)
                for route, res in _both_routes(ctxs[radius], name, f["T_leak"], _level(stride)):
                    x = dc.step_of(res["T"], f["T_leak"])
                    leak = dc.leak(Q, x)
                    print(f"{route} {name} stride {stride} radius {radius}: |x| {np.linalg.norm(x):.3e}, leak {leak:.3e} / {bar:.3e} = {leak / bar:.3e}")
                    assert res["status"] == 0 and np.linalg.norm(x) > 1e-3
                    assert leak <= bar
                    assert np.linalg.norm(res["T"] - ref["T"]) <= ref["pose_bound"]


def test_a_few_iterations_end_within_the_parity_bar(ctxs, orc):
    """five iterations, eps = FEW_EPS (no step of a reference run comes within 10 times of it: tests/test_icp_degenerate_reference_cpu.py,
    so status and iters_run are compared), against the C
    oracle and track_reference.track at the bar every registration test uses: 1e-4 Frobenius"""
    for name in dc.PAIR_CASES:
        for radius in dc.RADII:
            for sim3 in ((False, True) if name in dc.SIM3_CASES else (False,)):
                src, nmap = dc.maps(orc, name, radius)
                T0 = dc.pair_frames()[name]["T_init"]
                o = orc.icp(src, nmap, T_init=T0, iters=dc.FEW_ITERS, stride=2, estimate_scale=sim3, **dict(dc.PRM, eps=dc.FEW_EPS))
                assert (o["status"], o["iters_run"]) == (0, dc.FEW_ITERS)
                for route, res in _both_routes(ctxs[radius], name, T0, dict(_level(2, sim3), iters=dc.FEW_ITERS, eps=dc.FEW_EPS)):
                    d = float(np.linalg.norm(res["T"] - o["T"]))
                    print(f"{route} {name} radius {radius}{' Sim(3)' if sim3 else ''}, {dc.FEW_ITERS} iterations: |T - T_oracle| {d:.3e} / 1e-4 = {d / 1e-4:.3e}; "
                          f"|scale - scale_oracle| {abs(res['scale'] - o['scale']):.3e}")
                    assert d < 1e-4
                    assert (res["status"], res["iters_run"]) == (o["status"], o["iters_run"])
    for name in dc.TRACK_CASES:
        c = dc.track_cases()[name]
        ref = dc.track_few_reference(name, 2)
        assert (ref["status"], ref["iters_run"]) == (0, dc.FEW_ITERS)
        with _track_ctx(False) as ctx:
            ctx.upload_grid(tl3d.CH_TSDF, c["rec"])
            ctx.upload(0, c["depth"], None)
            res = ctx.track(0, c["start"], [dict(_track_level(2), iters=dc.FEW_ITERS, eps=dc.FEW_EPS)])
        d = float(np.linalg.norm(res["T"] - ref["T"]))
        print(f"track {name}, {dc.FEW_ITERS} iterations: |T - T_ref| {d:.3e} / 1e-4 = {d / 1e-4:.3e}")
        assert d < 1e-4
        assert (res["status"], res["iters_run"]) == (ref["status"], ref["iters_run"])


def test_count_gates(ctxs, orc):
    """5 matched pixels (7 for tracking): status 2, no update, the start pose bit for bit; 6 (8): the solve runs"""
    ctx = ctxs[0]
    T0 = dc.pixel_frames()["pixels5"]["T_init"]
    for stride in dc.STRIDES:
        assert dc.reference_step(orc, "pixels5", stride, 0)["n_corr"] == 5
        for route, res in _both_routes(ctx, "pixels5", T0, _level(stride)):
            assert (res["status"], res["iters_run"], res["n_corr"], res["n_src"]) == (2, 0, 5, 5), route
            assert np.array_equal(res["T"], T0), route
        ref = dc.reference_step(orc, "pixels6", stride, 0)
        assert ref["n_corr"] == 6 and ref["status"] == 0
        for route, res in _both_routes(ctx, "pixels6", T0, _level(stride)):
            _check_step(ctx, "pixels6", stride, res, ref, f"{route} six pixels stride {stride}")
    c = dc.track_cases()["track_plane"]
    with _track_ctx(False, n_slots=2) as tctx:
        tctx.upload_grid(tl3d.CH_TSDF, c["rec"])
        tctx.upload(0, dc.track_pixel_depth(7), None)
        tctx.upload(1, dc.track_pixel_depth(8), None)
        res = tctx.track(0, c["start"], [_track_level(2)])
        assert (res["status"], res["iters_run"], res["n_corr"], res["n_src"]) == (2, 0, 7, 7)
        assert np.array_equal(res["T"], c["T0"])
        ref = dc.track_reference_step("track_plane", 2, dc.track_pixel_depth(8))
        assert ref["n_corr"] == 8 and ref["status"] == 0
        res = tctx.track(1, c["start"], [_track_level(2)])
        d = float(np.linalg.norm(res["T"] - ref["T"]))
        print(f"track eight pixels: |T - T_ref| {d:.3e} / {ref['pose_bound']:.3e} = {d / ref['pose_bound']:.3e}")
        assert d <= ref["pose_bound"] and (res["status"], res["iters_run"]) == (0, 1)


def _same(a, b):
    return np.array_equal(a["T"], b["T"]) and all(a[k] == b[k] for k in ("scale", "rmse", "fitness", "n_corr", "n_src", "iters_run", "status"))


def test_degenerate_steps_repeat_bit_for_bit(ctxs):
    """across two calls, and across two positions inside a batch of 20 mixed pairs"""
    ctx = ctxs[1]
    names = [dc.PAIR_CASES[i % len(dc.PAIR_CASES)] for i in range(20)]
    for probe in ("plane", "sphere", "cylinder", "tube"):
        mixed = list(names)
        mixed[3] = mixed[17] = probe
        pairs = [SLOT[n] for n in mixed]
        Ts = [dc.pair_frames()[n]["T_init"] for n in mixed]
        level = _level(2)
        batch = ctx.icp_batch(pairs, [level], T_init=Ts)
        again = ctx.icp_batch(pairs, [level], T_init=Ts)
        assert batch[3]["status"] == 0 and batch[3]["iters_run"] == 1
        assert _same(batch[3], batch[17]), probe
        assert all(_same(a, b) for a, b in zip(batch, again)), probe
        s, t = SLOT[probe]
        one = ctx.icp(s, t, T_init=dc.pair_frames()[probe]["T_init"], **level)
        two = ctx.icp(s, t, T_init=dc.pair_frames()[probe]["T_init"], **level)
        assert _same(one, two), probe
    for name in dc.TRACK_CASES:
        c = dc.track_cases()[name]
        with _track_ctx(False) as tctx:
            tctx.upload_grid(tl3d.CH_TSDF, c["rec"])
            tctx.upload(0, c["depth"], None)
            a, b = tctx.track(0, c["start"], [_track_level(2)]), tctx.track(0, c["start"], [_track_level(2)])
            assert _same(a, b), name
