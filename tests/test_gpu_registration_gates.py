"""GPU: the two count thresholds of the step behind a pass of tracking, colour and cloud registration (csrc/kernels_regstep.hip: one
routine for the three) on the scenes of tests/registration_gates_common.py, against the three numpy references.

An iteration needs 6 correspondences in the colour and the cloud step (tracking's 8 is pinned by test_gpu_icp_degenerate.py::
test_count_gates): with 5 the run fails -- status 2, no update, the start pose bit for bit --, with 6 the solve runs.  A level that
ends with fewer than 8 is the run's last, for all three: with 6 or 7 the two-level run IS the one-level run, bit for bit; with 8 the
second level runs.  Every scene's counts are asserted of its reference first (check_schedule_refs, hole_around_cutoff), so a scene
that drifts off its edge fails here instead of passing on the other side.  Status, iters_run and the counts are exact; a pose that
moved is held to the project's ICP parity bar of 1e-4 (Frobenius) of the reference's, as every registration test does.  Every
comparison prints what it measured."""
import numpy as np
import pytest

import icp_degenerate_common as dc
import registration_gates_common as gc
import rgbd_common as rc
import tl3d

pytestmark = pytest.mark.gpu


def _assert_run(got, ref, what):
    dT = float(np.linalg.norm(got["T"] - ref["T"]))
    ds = abs(got["scale"] - ref.get("scale", 1.0))
    print(f"{what}: |T - T_ref|_F {dT:.3e}, |scale - scale_ref| {ds:.3e} (bar {gc.PARITY:g}); status {got['status']} / {ref['status']}, iterations "
          f"{got['iters_run']} / {ref['iters_run']}, n_corr {got['n_corr']} / {ref['n_corr']} of {got['n_src']} / {ref['n_src']}")
    assert (got["status"], got["iters_run"], got["n_corr"], got["n_src"]) == (ref["status"], ref["iters_run"], ref["n_corr"], ref["n_src"]), what
    assert dT <= gc.PARITY and ds <= gc.PARITY, what


def _assert_failed_at_start(got, T0, n, what):
    print(f"{what}: status {got['status']}, iterations {got['iters_run']}, n_corr {got['n_corr']} of {got['n_src']}, |T - T0| {np.linalg.norm(got['T'] - T0):.3e}")
    assert (got["status"], got["iters_run"], got["n_corr"], got["n_src"]) == (2, 0, n, n), what
    assert np.array_equal(got["T"], T0) and got["scale"] == 1.0, what


def _assert_schedule(one, two, one_ref, two_ref, n, what):
    """the one-level and the two-level run of a scene whose first level ends with n correspondences"""
    _assert_run(one, one_ref, f"{what}, level one alone")
    _assert_run(two, two_ref, f"{what}, both levels")
    if n < 8:
        assert gc.same_result(one, two), f"{what}: the second level ran"
    else:
        assert two["iters_run"] == gc.LEVEL2_ITERS and not np.array_equal(two["T"], one["T"]), f"{what}: the second level did not run"


# ---- cloud -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud_ctx():
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as c:
        yield c


def _cloud(ctx, n, kind, iters):
    c = gc.cloud_case(n, kind)
    return ctx.register_clouds(c["src"], c["tgt"], c["normals"], levels=gc.cloud_levels(iters), estimate_scale=c["estimate_scale"])


@pytest.mark.parametrize("kind", gc.CLOUD_KINDS)
def test_cloud_iteration_needs_six(cloud_ctx, kind):
    ref5 = gc.cloud_ref(5, kind, (1,))
    assert (ref5["status"], ref5["iters_run"], ref5["n_corr"], ref5["n_src"]) == (2, 0, 5, 5)
    _assert_failed_at_start(_cloud(cloud_ctx, 5, kind, (1,)), np.eye(4), 5, f"cloud {kind}, 5 points")
    M, n_corr = gc.cloud_first_system(6, kind)
    ref6 = gc.cloud_ref(6, kind, (1,))
    assert n_corr == 6 and gc.hole_around_cutoff(M, gc.CLOUD_LV["damping"], gc.CLOUD_LV["eig_rel"])
    assert (ref6["status"], ref6["iters_run"], ref6["n_corr"]) == (0, 1, 6) and np.linalg.norm(ref6["T"] - np.eye(4)) > 100 * gc.PARITY
    _assert_run(_cloud(cloud_ctx, 6, kind, (1,)), ref6, f"cloud {kind}, 6 points")


@pytest.mark.parametrize("n", gc.COUNTS)
@pytest.mark.parametrize("kind", gc.CLOUD_KINDS)
def test_cloud_level_that_ends_below_eight_is_the_last(cloud_ctx, kind, n):
    one_ref, two_ref = gc.cloud_ref(n, kind, (1,)), gc.cloud_ref(n, kind, (1, gc.LEVEL2_ITERS))
    gc.check_schedule_refs(one_ref, two_ref, n, 1)
    assert gc.hole_around_cutoff(gc.cloud_first_system(n, kind)[0], gc.CLOUD_LV["damping"], gc.CLOUD_LV["eig_rel"])
    _assert_schedule(_cloud(cloud_ctx, n, kind, (1,)), _cloud(cloud_ctx, n, kind, (1, gc.LEVEL2_ITERS)), one_ref, two_ref, n, f"cloud {kind}, {n} points")


# ---- colour ------------------------------------------------------------------------------------------------------------------------
RGBD_N = (5,) + gc.COUNTS                                       # slot 0: the target; slot 1 + i: the source with RGBD_N[i] pixels


@pytest.fixture(scope="module")
def rgbd_ctx():
    f = rc.pairs()["control"]
    with tl3d.FusionContext(rc.W, rc.H, rc.CAM["fx"], rc.CAM["fy"], rc.CAM["cx"], rc.CAM["cy"], n_slots=1 + len(RGBD_N), grid=None) as ctx:
        ctx.set_normal_smoothing(0)
        ctx.upload(0, f["tgt"], f["tgt_bgr"])
        for i, n in enumerate(RGBD_N):
            ctx.upload(1 + i, *gc.rgbd_frame(n))
        ctx.build_normals_many(list(range(1 + len(RGBD_N))))
        ctx.build_intensity(list(range(1 + len(RGBD_N))), rc.RADIUS, rc.JUMP)
        yield ctx


def _rgbd(ctx, n, iters, weight):
    return ctx.rgbd_register([(1 + RGBD_N.index(n), 0)], gc.rgbd_levels(iters, weight), T_init=[gc.rgbd_T0()])[0]


def _assert_photo(got, ref, what):
    print(f"{what}: n_photo {got['n_photo']} / {ref['n_photo']}, n_qualified {got['n_qualified']} / {ref['n_qualified']}")
    assert (got["n_photo"], got["n_qualified"]) == (ref["n_photo"], ref["n_qualified"]), what


@pytest.mark.parametrize("weight", gc.RGBD_WEIGHTS)
def test_colour_iteration_needs_six_not_eight(rgbd_ctx, weight):
    ref5 = gc.rgbd_ref(5, (1,), weight)
    assert (ref5["status"], ref5["iters_run"], ref5["n_corr"], ref5["n_src"]) == (2, 0, 5, 5)
    _assert_failed_at_start(_rgbd(rgbd_ctx, 5, (1,), weight), gc.rgbd_T0(), 5, f"colour weight {weight}, 5 pixels")
    M, s = gc.rgbd_first_system(6, weight)
    ref6 = gc.rgbd_ref(6, (1,), weight)
    assert s["n_corr"] == 6 and s["n_photo"] > 0 and gc.hole_around_cutoff(M, gc.RGBD_LV["damping"], gc.RGBD_LV["eig_rel"])
    assert (ref6["status"], ref6["iters_run"], ref6["n_corr"]) == (0, 1, 6) and np.linalg.norm(ref6["T"] - gc.rgbd_T0()) > 100 * gc.PARITY
    got = _rgbd(rgbd_ctx, 6, (1,), weight)
    _assert_run(got, ref6, f"colour weight {weight}, 6 pixels")
    _assert_photo(got, ref6, f"colour weight {weight}, 6 pixels")
    if weight:                                              # the weight reaches the solve: the two references are apart
        assert np.linalg.norm(ref6["T"] - gc.rgbd_ref(6, (1,), 0.0)["T"]) > 2.0 * gc.PARITY


@pytest.mark.parametrize("n", gc.COUNTS)
@pytest.mark.parametrize("weight", gc.RGBD_WEIGHTS)
def test_colour_level_that_ends_below_eight_is_the_last(rgbd_ctx, weight, n):
    one_ref, two_ref = gc.rgbd_ref(n, (1,), weight), gc.rgbd_ref(n, (1, gc.LEVEL2_ITERS), weight)
    gc.check_schedule_refs(one_ref, two_ref, n, 1)
    assert gc.hole_around_cutoff(gc.rgbd_first_system(n, weight)[0], gc.RGBD_LV["damping"], gc.RGBD_LV["eig_rel"])
    one, two = _rgbd(rgbd_ctx, n, (1,), weight), _rgbd(rgbd_ctx, n, (1, gc.LEVEL2_ITERS), weight)
    _assert_schedule(one, two, one_ref, two_ref, n, f"colour weight {weight}, {n} pixels")
    _assert_photo(two, two_ref, f"colour weight {weight}, {n} pixels")
    if n < 8:
        assert (one["n_photo"], one["n_qualified"], one["photo_rmse"]) == (two["n_photo"], two["n_qualified"], two["photo_rmse"])


# ---- tracking ----------------------------------------------------------------------------------------------------------------------
def test_tracking_level_that_ends_below_eight_is_the_last():
    c = dc.track_cases()["track_plane"]
    spec = tl3d.GridSpec(dc.T_DIMS, dc.T_ORIGIN, dc.T_VOXEL, dc.T_TRUNC, tl3d.CH_TSDF)
    with tl3d.FusionContext(dc.W, dc.H, dc.CAM["fx"], dc.CAM["fy"], dc.CAM["cx"], dc.CAM["cy"], n_slots=len(gc.COUNTS), grid=spec) as ctx:
        ctx.upload_grid(tl3d.CH_TSDF, c["rec"])
        for slot, n in enumerate(gc.COUNTS):
            ctx.upload(slot, dc.track_pixel_depth(n), None)
            one_ref, two_ref = gc.track_ref(n, (0,)), gc.track_ref(n, (0, gc.LEVEL2_ITERS))
            gc.check_schedule_refs(one_ref, two_ref, n, 0)
            one, two = ctx.track(slot, c["start"], gc.track_levels((0,))), ctx.track(slot, c["start"], gc.track_levels((0, gc.LEVEL2_ITERS)))
            _assert_schedule(one, two, one_ref, two_ref, n, f"tracking, {n} pixels")
            assert np.array_equal(one["T"], c["T0"])            # a level without updates leaves the start pose
