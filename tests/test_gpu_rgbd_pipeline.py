"""GPU: config.photometric through the pipeline and the command line.  Six frames of a camera moving 3 cm
and 0.5 degrees of yaw per frame down an open rectangular tube, whose ends lie beyond max_depth: point-to-plane ICP cannot see the
motion along the axis and the camera "stands still"; with the photometric term the chain follows it.  The refusals raise before any
device work."""
import numpy as np
import pytest

import tl3d
import track_reference as tr
from helpers import SMALL
from tl3d import synth
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu

CAM = {k: SMALL[k] for k in ("fx", "fy", "cx", "cy")}
BASE = dict(**CAM, voxel_size=0.04, subsample_factor=2, grid_dim=128)
N = 6


@pytest.fixture(scope="module")
def dolly():
    scene = synth.Scene(room=((-1, -1.2, -50), (1, 1.2, 200)))
    poses = synth.dolly_poses(N, (0.1, -0.1, 0), (0, 0, 0.03), 0.5)
    return poses, [synth.render(scene, p, **SMALL) for p in poses]


def _centre(pose):
    R, t = np.asarray(pose[0], float).reshape(3, 3), np.asarray(pose[1], float).reshape(3)
    return -R.T @ t


def _centre_error(pipe, poses):
    """distance between the last kept camera's centre and the true one, in the first camera's frame"""
    last = pipe.frame_index[-1]
    T_true = tr.pose_matrix(poses[last]) @ np.linalg.inv(tr.pose_matrix(poses[0]))
    return float(np.linalg.norm(_centre(pipe.camera_poses[-1]) - _centre((T_true[:3, :3], T_true[:3, 3]))))


def _run(frames, **kw):
    pipe = DepthToReconstructionPipeline(ReconstructionConfig(**BASE, **kw))
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    return pipe, pipe.reconstruct()


@pytest.fixture(scope="module")
def runs(dolly):
    poses, frames = dolly
    return _run(frames, photometric=True), _run(frames)


def test_the_chain_follows_the_tube_only_with_colour(dolly, runs):
    poses, _frames = dolly
    (on, out_on), (off, out_off) = runs
    assert out_on[0] is not None and out_off[0] is not None
    assert on.frame_index == list(range(N)) and off.frame_index == list(range(N))
    e_on, e_off = _centre_error(on, poses), _centre_error(off, poses)
    print(f"last camera centre off by {e_on * 1e3:.2f} mm with photometric, {e_off * 1e3:.1f} mm without, over {0.03 * (N - 1) * 1e3:.0f} mm of travel")
    assert e_on <= 0.005
    assert e_off > 0.100
    st = on.stats["photometric"]
    assert st["frames"] == N - 1 and st["n_photo"] > 500 * (N - 1) and 0 < st["mean_photo_rmse"] < 0.05
    assert (st["weight"], st["gate"], st["smooth_radius"], st["depth_jump"]) == (0.1, 0.2, 1, 0.05)
    assert len(on.icp_log) == N - 1 and all(e["n_photo"] > 500 and e["photo_rmse"] > 0 for e in on.icp_log)
    assert "photometric" not in off.stats and all("n_photo" not in e for e in off.icp_log)
    assert set(on.stats) - set(off.stats) == {"photometric"}


def test_off_makes_no_call(dolly, monkeypatch):
    _poses, frames = dolly
    calls = []
    for name in ("build_intensity", "rgbd_register"):
        real = getattr(tl3d.FusionContext, name)
        monkeypatch.setattr(tl3d.FusionContext, name, lambda self, *a, _r=real, _n=name, **kw: (calls.append(_n), _r(self, *a, **kw))[1])
    _run(frames[:3], photo_weight=0.5, photo_smooth_radius=2)          # the parameters alone do nothing
    assert calls == []
    _run(frames[:3], photometric=True)
    assert calls == ["build_intensity", "rgbd_register"]               # one map build, one batch


def test_the_command_line_gives_the_same_poses(dolly, runs, tmp_path, monkeypatch, capsys):
    from PIL import Image
    import depth_to_reconstruction as d2r
    _poses, frames = dolly
    rgb_dir, depth_dir = tmp_path / "rgb", tmp_path / "depth"
    rgb_dir.mkdir()
    depth_dir.mkdir()
    for i, (d, c) in enumerate(frames):
        Image.fromarray(c[..., ::-1]).save(rgb_dir / f"frame_{i:04d}.png")
        np.save(depth_dir / f"frame_{i:04d}_depth.npy", d)
    seen = []
    real = DepthToReconstructionPipeline.reconstruct
    monkeypatch.setattr(DepthToReconstructionPipeline, "reconstruct", lambda self, *a, **kw: (seen.append(self), real(self, *a, **kw))[1])
    cam = ["--fx", str(SMALL["fx"]), "--fy", str(SMALL["fy"]), "--cx", str(SMALL["cx"]), "--cy", str(SMALL["cy"])]
    tail = ["--no-vis", "--voxel-size", "0.04", "--grid", "128", *cam]
    out = tmp_path / "a.ply"
    assert d2r.main(["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--output", str(out), "--photometric", "--photo-weight", "0.1",
                     "--photo-gate", "0.2", "--photo-smooth-radius", "1", *tail]) == 0
    assert out.stat().st_size > 1000 and len(seen) == 1 and seen[0].config.photometric
    (on, _out), _off = runs
    assert len(seen[0].camera_poses) == len(on.camera_poses) == N
    for (ra, ta), (rb, tb) in zip(seen[0].camera_poses, on.camera_poses):
        assert np.asarray(ra).tobytes() == np.asarray(rb).tobytes() and np.asarray(ta).tobytes() == np.asarray(tb).tobytes()
    capsys.readouterr()
    for extra, msg in ((["--gpus", "2"], "single GPU"), (["--estimate-scale"], "estimate_scale"), (["--loop-closure"], "loop_closure"),
                       (["--photo-weight", "-1"], "photo_weight"), (["--photo-smooth-radius", "8"], "photo_smooth_radius")):
        with pytest.raises(SystemExit):                      # refused before any process is started
            d2r.main(["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--output", str(tmp_path / "x.ply"), "--photometric", *extra, *tail])
        assert msg in capsys.readouterr().err and not (tmp_path / "x.ply").exists()


def test_refusals_come_before_any_device_work(dolly, monkeypatch):
    _poses, frames = dolly

    def no_device(*a, **kw):
        raise AssertionError("a context was created")
    monkeypatch.setattr("tl3d.pipeline.FusionContext", no_device)

    def pipe(images=None, **kw):
        p = DepthToReconstructionPipeline(ReconstructionConfig(**BASE, photometric=True, **kw))
        p.set_frames([c for d, c in frames] if images is None else images, [d for d, c in frames])
        return p
    with pytest.raises(ValueError, match="colour"):
        pipe(images=[c if i != 2 else None for i, (d, c) in enumerate(frames)]).reconstruct()
    with pytest.raises(ValueError, match="estimate_scale"):
        pipe().reconstruct(estimate_scale=True)
    with pytest.raises(ValueError, match="loop_closure"):
        pipe(loop_closure=True).reconstruct()
    with pytest.raises(ValueError, match="single GPU"):
        pipe().reconstruct_sharded(dist=None)
    for bad in (dict(photo_weight=-0.1), dict(photo_gate=0.0), dict(photo_smooth_radius=8), dict(photo_depth_jump=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            pipe(**bad).reconstruct()
