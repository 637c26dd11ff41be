"""CPU: the scenes of tests/registration_gates_common.py sit where tests/test_gpu_registration_gates.py needs them -- shown with the
numpy references alone, so that a scene that drifts off a threshold fails without a GPU too."""
import numpy as np
import pytest

import icp_degenerate_common as dc
import registration_gates_common as gc


@pytest.mark.parametrize("kind", gc.CLOUD_KINDS)
def test_cloud_scenes(kind):
    ref5, ref6 = gc.cloud_ref(5, kind, (1,)), gc.cloud_ref(6, kind, (1,))
    assert (ref5["status"], ref5["iters_run"], ref5["n_corr"], ref5["n_src"]) == (2, 0, 5, 5) and np.array_equal(ref5["T"], np.eye(4))
    assert (ref6["status"], ref6["iters_run"], ref6["n_corr"]) == (0, 1, 6) and np.linalg.norm(ref6["T"] - np.eye(4)) > 100 * gc.PARITY
    for n in gc.COUNTS:
        M, n_corr = gc.cloud_first_system(n, kind)
        assert n_corr == n and gc.hole_around_cutoff(M, gc.CLOUD_LV["damping"], gc.CLOUD_LV["eig_rel"])
        gc.check_schedule_refs(gc.cloud_ref(n, kind, (1,)), gc.cloud_ref(n, kind, (1, gc.LEVEL2_ITERS)), n, 1)


@pytest.mark.parametrize("weight", gc.RGBD_WEIGHTS)
def test_colour_scenes(weight):
    ref5, ref6 = gc.rgbd_ref(5, (1,), weight), gc.rgbd_ref(6, (1,), weight)
    assert (ref5["status"], ref5["iters_run"], ref5["n_corr"], ref5["n_src"]) == (2, 0, 5, 5) and np.array_equal(ref5["T"], gc.rgbd_T0())
    assert (ref6["status"], ref6["iters_run"], ref6["n_corr"]) == (0, 1, 6) and np.linalg.norm(ref6["T"] - gc.rgbd_T0()) > 100 * gc.PARITY
    if weight:
        assert np.linalg.norm(ref6["T"] - gc.rgbd_ref(6, (1,), 0.0)["T"]) > 2.0 * gc.PARITY
    for n in gc.COUNTS:
        M, s = gc.rgbd_first_system(n, weight)
        assert s["n_corr"] == n and s["n_photo"] > 0 and gc.hole_around_cutoff(M, gc.RGBD_LV["damping"], gc.RGBD_LV["eig_rel"])
        gc.check_schedule_refs(gc.rgbd_ref(n, (1,), weight), gc.rgbd_ref(n, (1, gc.LEVEL2_ITERS), weight), n, 1)


def test_tracking_scenes():
    T0 = dc.track_cases()["track_plane"]["T0"]
    for n in gc.COUNTS:
        one = gc.track_ref(n, (0,))
        gc.check_schedule_refs(one, gc.track_ref(n, (0, gc.LEVEL2_ITERS)), n, 0)
        assert np.array_equal(one["T"], T0)
