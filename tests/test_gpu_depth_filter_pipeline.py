"""GPU: config.depth_filter through the pipeline and both command lines, on the SMALL scene of
tests/helpers.py with every depth frame passed through a 3 x 3 box blur (what a depth network or a sensor's interpolation does to
an occlusion edge).  On: points, colours and poses are, bit for bit, those of a run with the option off on frames the numpy
reference filtered beforehand -- from host arrays and from files through the streaming loader -- and stats["depth_filter"] holds the
reference's totals.  Off: no key, no call.  The effect: fewer fused points away from every true surface of the analytic scene."""
import numpy as np
import pytest

import depth_filter_common as dc
import depth_filter_reference as dr
import tl3d
from helpers import SMALL, small_scene_frames
from tl3d import synth
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu

CAM = {k: SMALL[k] for k in ("fx", "fy", "cx", "cy")}
VOXEL = 0.02
BASE = dict(**CAM, voxel_size=VOXEL, subsample_factor=1, grid_dim=128)
PRM = dc.prm()                                          # the defaults: jump 0.05, radius 1, min_support 4, no region stage
REGION = dc.prm(min_region=40)


def box3(d):
    """3 x 3 box blur with the border repeated"""
    p = np.pad(d.astype(np.float64), 1, mode="edge")
    h, w = d.shape
    return (sum(p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0).astype(np.float32)


@pytest.fixture(scope="module")
def scene():
    """(poses, blurred frames, {params: (reference-filtered frames, total counts)})"""
    poses, frames = small_scene_frames(n=3)
    blurred = [(box3(d), c) for d, c in frames]
    ref = {}
    for key, prm in (("default", PRM), ("region", REGION)):
        res = [dr.filter_shifted(d, **prm) for d, _c in blurred]
        ref[key] = ([(r[0], c) for r, (_d, c) in zip(res, blurred)], np.sum([r[1] for r in res], axis=0))
    assert ref["default"][1][1] > 1500                  # (659 in frame 0: DESIGN.md section 4.7)
    return poses, blurred, ref


def _run(frames, poses=None, **kw):
    pipe = DepthToReconstructionPipeline(ReconstructionConfig(**BASE, **kw))
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    return pipe, pipe.reconstruct(poses=poses)


def _same(a, b):
    (xa, ca, pa), (xb, cb, pb) = a, b
    assert len(xa) > 1000
    assert xa.tobytes() == xb.tobytes() and np.asarray(ca).tobytes() == np.asarray(cb).tobytes()
    assert len(pa) == len(pb)
    for (ra, ta), (rb, tb) in zip(pa, pb):
        assert np.asarray(ra).tobytes() == np.asarray(rb).tobytes() and np.asarray(ta).tobytes() == np.asarray(tb).tobytes()


def _flags(prm):
    return dict(depth_filter=True, depth_filter_jump=prm["jump_rel"], depth_filter_radius=prm["radius"],
                depth_filter_min_support=prm["min_support"], depth_filter_min_region=prm["min_region"])


@pytest.mark.parametrize("key,prm", [("default", PRM), ("region", REGION)])
def test_on_equals_off_on_prefiltered_frames(scene, key, prm):
    _poses, blurred, ref = scene
    pre, totals = ref[key]
    on, out_on = _run(blurred, **_flags(prm))           # registered, not given: the poses come out of the filtered frames too
    off, out_off = _run(pre)
    _same(out_on, out_off)
    st = on.stats["depth_filter"]
    assert [st[k] for k in ("valid", "removed_flying", "regions", "removed_regions")] == totals.tolist()
    assert st["frames"] == 3 and {k: st[k] for k in prm} == prm
    assert set(on.stats) - set(off.stats) == {"depth_filter"}
    assert set(on.timings) - set(off.timings) == {"depth_filter_s"} and on.timings["depth_filter_s"] >= 0


def test_off_makes_no_call_and_leaves_no_key(scene, monkeypatch):
    _poses, blurred, _ref = scene
    calls = []
    real = tl3d.FusionContext.filter_depth_slots

    def counting(self, *a, **kw):
        calls.append(1)
        return real(self, *a, **kw)
    monkeypatch.setattr(tl3d.FusionContext, "filter_depth_slots", counting)
    off, (xyz, _rgb, _p) = _run(blurred, depth_filter_radius=2, depth_filter_min_region=99)     # the parameters alone do nothing
    assert calls == [] and len(xyz) > 1000
    assert not any("depth_filter" in k for k in off.stats) and not any("depth_filter" in k for k in off.timings)
    on, _out = _run(blurred, depth_filter=True)
    assert calls == [1]                                 # once over all slots


def _write(tmp, name, frames):
    from PIL import Image
    rgb_dir, depth_dir = tmp / f"{name}_rgb", tmp / f"{name}_depth"
    rgb_dir.mkdir()
    depth_dir.mkdir()
    for i, (d, c) in enumerate(frames):
        Image.fromarray(c[..., ::-1]).save(rgb_dir / f"frame_{i:04d}.png")
        np.save(depth_dir / f"frame_{i:04d}_depth.npy", d)
    return rgb_dir, depth_dir


def test_streaming_loader_and_both_command_lines(scene, tmp_path, capsys):
    import depth_enhanced_reconstruction as der
    import depth_to_reconstruction as d2r
    _poses, blurred, ref = scene
    pre, totals = ref["default"]
    raw_rgb, raw_depth = _write(tmp_path, "raw", blurred)
    pre_rgb, pre_depth = _write(tmp_path, "pre", pre)
    # the streaming loader
    on = DepthToReconstructionPipeline(ReconstructionConfig(**BASE, depth_filter=True))
    assert on.load_data_streaming(str(raw_rgb), str(raw_depth)) == 3
    out_on = on.reconstruct()
    off = DepthToReconstructionPipeline(ReconstructionConfig(**BASE))
    assert off.load_data_streaming(str(pre_rgb), str(pre_depth)) == 3
    _same(out_on, off.reconstruct())
    assert [on.stats["depth_filter"][k] for k in ("valid", "removed_flying", "regions", "removed_regions")] == totals.tolist()
    assert "depth_filter" not in off.stats
    # both command lines: the flag on the blurred files writes the file that the plain run writes from the pre-filtered files
    cam = ["--fx", str(SMALL["fx"]), "--fy", str(SMALL["fy"]), "--cx", str(SMALL["cx"]), "--cy", str(SMALL["cy"])]
    tail = ["--no-vis", "--voxel-size", "0.025", "--grid", "128", *cam]
    a, b = tmp_path / "a.ply", tmp_path / "b.ply"
    assert d2r.main(["--rgb-folder", str(raw_rgb), "--depth-folder", str(raw_depth), "--output", str(a), "--depth-filter", *tail]) == 0
    assert "Depth filter:" in capsys.readouterr().out
    assert d2r.main(["--rgb-folder", str(pre_rgb), "--depth-folder", str(pre_depth), "--output", str(b), *tail]) == 0
    assert "Depth filter:" not in capsys.readouterr().out
    assert a.stat().st_size > 10000 and a.read_bytes() == b.read_bytes()
    c = tmp_path / "c.ply"                               # the options' defaults spelled out
    assert d2r.main(["--rgb-folder", str(raw_rgb), "--depth-folder", str(raw_depth), "--output", str(c), "--depth-filter", "--depth-filter-jump", "0.05",
                     "--depth-filter-radius", "1", "--depth-filter-min-support", "4", "--depth-filter-min-region", "0", *tail]) == 0
    assert c.read_bytes() == a.read_bytes()
    assert der.main(["--input", str(raw_rgb), "--depth-folder", str(raw_depth), "--output", str(tmp_path / "der_on"), "--depth-filter", *cam]) == 0
    assert der.main(["--input", str(pre_rgb), "--depth-folder", str(pre_depth), "--output", str(tmp_path / "der_off"), *cam]) == 0
    on_bytes = (tmp_path / "der_on" / "reconstruction.ply").read_bytes()
    assert len(on_bytes) > 10000 and on_bytes == (tmp_path / "der_off" / "reconstruction.ply").read_bytes()
    capsys.readouterr()
    with pytest.raises(SystemExit):                      # refused before any process is started
        d2r.main(["--rgb-folder", str(raw_rgb), "--depth-folder", str(raw_depth), "--output", str(tmp_path / "x.ply"), "--gpus", "2", "--depth-filter", *tail])
    assert "--depth-filter needs a single GPU" in capsys.readouterr().err and not (tmp_path / "x.ply").exists()


def surface_distance(scene, pts):
    """distance of every point to the nearest true surface of an analytic scene of spheres inside a room (a box seen from inside)"""
    pts = np.asarray(pts, np.float64)
    d = np.full(len(pts), np.inf)
    for c, r in scene.spheres:
        d = np.minimum(d, np.abs(np.linalg.norm(pts - np.asarray(c, np.float64), axis=1) - r))
    lo, hi = (np.asarray(v, np.float64) for v in scene.room)
    inside = np.minimum(pts - lo, hi - pts)                                  # per axis, negative outside
    outside = np.linalg.norm(np.maximum(np.maximum(lo - pts, pts - hi), 0.0), axis=1)
    box = np.where((inside >= 0).all(axis=1), inside.min(axis=1), outside)
    return np.minimum(d, box)


def test_the_effect_fewer_points_off_every_surface(scene):
    """With the true poses, the fused points farther than 3 voxels from every true surface: the blurred frames must give at least 100 of
    them (the condition on the input), and the filtered run fewer.  Measured pair: DESIGN.md section 4.7."""
    poses, blurred, _ref = scene
    world = synth.object_scene()
    assert not world.planes and not world.cylinders and world.room is not None
    _p0, (xyz0, _c0, _) = _run(blurred, poses=poses)
    _p1, (xyz1, _c1, _) = _run(blurred, poses=poses, depth_filter=True)
    far0 = int((surface_distance(world, xyz0) > 3 * VOXEL).sum())
    far1 = int((surface_distance(world, xyz1) > 3 * VOXEL).sum())
    print(f"points farther than 3 voxels from every surface: {far0} of {len(xyz0)} unfiltered, {far1} of {len(xyz1)} filtered")
    assert far0 >= 100
    assert far1 < far0
