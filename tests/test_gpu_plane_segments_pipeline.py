"""GPU: config.cloud_planes through the pipeline, the saved files and both command lines, on the SMALL scene
of tests/helpers.py and on a short run down the corridor of config 3: off by default with no trace and the file's bytes as ever;
on, the arrays of a direct FusionContext.segment_planes call on the pipeline's own cloud, which are those of the numpy / scipy
reference of tests/plane_segments_reference.py; the same partition from a blocked run; the `plane` property and the JSON report."""
import json
import math

import numpy as np
import pytest

import plane_segments_reference as pr
import tl3d
from helpers import SMALL, small_scene_frames
from tl3d import pipeline as pl
from tl3d import synth
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu

CAM = {k: SMALL[k] for k in ("fx", "fy", "cx", "cy")}
VOXEL = 0.02
BASE = dict(**CAM, voxel_size=VOXEL, subsample_factor=1, grid_dim=128)
ON = dict(cloud_normals=True, cloud_planes=True)
COUNT_KEYS = ("eligible", "regions", "candidates", "planes")


@pytest.fixture(scope="module")
def scene():
    return small_scene_frames(n=3, noise=0.002)          # (the noise: see test_gpu_cloud_normals_pipeline.py)


def _run(scene, limit=None, base=BASE, **kw):
    poses, frames = scene
    old = pl.MAX_BLOCK_VOXELS
    try:
        if limit is not None:
            pl.MAX_BLOCK_VOXELS = limit
        pipe = DepthToReconstructionPipeline(ReconstructionConfig(**base, **kw))
        pipe.set_frames([c for d, c in frames], [d for d, c in frames])
        out = pipe.reconstruct(poses=poses)
    finally:
        pl.MAX_BLOCK_VOXELS = old
    return pipe, out


@pytest.fixture(scope="module")
def runs(scene):
    return _run(scene), _run(scene, **ON)


def _centres(poses):
    return np.array([-np.asarray(R, np.float64).T @ np.asarray(t, np.float64).reshape(3) for R, t in poses])


def _parse(path):
    """(property names, structured vertex array) of a binary PLY cloud"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    props = [ln.split()[1:] for ln in head if ln.startswith("property")]
    types = {"double": "<f8", "float": "<f4", "uchar": "u1", "int": "<i4"}
    nv = int(next(ln for ln in head if ln.startswith("element vertex")).split()[-1])
    rec = np.frombuffer(data, np.dtype([(nm, types[t]) for t, nm in props]), nv, end)
    assert len(data) == end + nv * rec.dtype.itemsize
    return [nm for _, nm in props], rec


def _reference(xyz, normals, curvature, voxel, **kw):
    prm = dict(radius=2.5 * voxel, min_cos=math.cos(math.radians(10.0)), max_offset=voxel, max_curvature=0.05, min_points=200, max_rms=0.5 * voxel)
    prm.update(kw)
    return pr.segment_tree(xyz.astype(np.float32), normals, curvature, pr.Params(**prm))


def _direct(xyz, poses, voxel, **kw):
    """normals, curvature and the direct segment_planes call on a pipeline's cloud, with the pipeline's parameters"""
    p32 = xyz.astype(np.float32)
    prm = dict(radius=2.5 * voxel, max_angle_deg=10.0, max_offset=voxel, max_curvature=0.05, min_points=200, max_rms=0.5 * voxel)
    prm.update(kw)
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as ctx:
        dn, dc = ctx.estimate_normals(p32, 30, viewpoints=_centres(poses), cell_size=2 * voxel, curvature=True)
        return dn, dc, ctx.segment_planes(p32, dn, dc, **prm), prm


def test_off_by_default_leaves_no_trace(runs, tmp_path):
    (off, (xyz, rgb, _)), _ = runs
    assert off.cloud_plane_ids is None and off.cloud_planes is None
    assert not any("cloud_planes" in k for k in off.stats) and not any("cloud_planes" in k for k in off.timings)
    off.save_reconstruction(xyz, rgb, str(tmp_path / "off.ply"))
    rec = np.empty(len(xyz), dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    for a, col in zip("xyz", xyz.T):
        rec[a] = col
    for a, col in zip("rgb", np.asarray(rgb).T):
        rec[a] = col
    head = ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {len(xyz)}\n" + "property double x\nproperty double y\nproperty double z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert len(xyz) > 1000 and (tmp_path / "off.ply").read_bytes() == head.encode("ascii") + rec.tobytes()


def test_on_gives_the_direct_calls_arrays_and_the_references(runs, tmp_path):
    (off, (xyz0, rgb0, _)), (on, (xyz, rgb, poses)) = runs
    assert xyz.tobytes() == xyz0.tobytes() and np.asarray(rgb).tobytes() == np.asarray(rgb0).tobytes()
    n = len(xyz)
    assert on.cloud_plane_ids.shape == (n,) and on.cloud_plane_ids.dtype == np.int32
    assert on.cloud_curvature is None and on.cloud_normals.shape == (n, 3)          # computed for the planes, kept only when asked for
    dn, dc, (ids, planes, counts), prm = _direct(xyz, poses, VOXEL)
    assert on.cloud_normals.tobytes() == dn.tobytes()
    assert on.cloud_plane_ids.tobytes() == ids.tobytes() and on.cloud_planes.tobytes() == planes.tobytes()
    st = on.stats["cloud_planes"]
    assert {k: st[k] for k in COUNT_KEYS} == counts and {k: st[k] for k in prm} == prm
    top = np.argsort(-planes["count"], kind="stable")[:10]
    assert st["largest"] == [dict(count=int(planes["count"][k]), rms=float(planes["rms"][k])) for k in top]
    assert set(on.stats) - set(off.stats) == {"cloud_normals", "cloud_planes"}
    assert set(on.timings) - set(off.timings) == {"cloud_normals_s", "cloud_planes_s"} and on.timings["cloud_planes_s"] >= 0
    res = _reference(xyz, dn, dc, VOXEL)
    print(f"small scene: {n} points, counts {res.counts}, plane sizes {res.planes['count'].tolist()}")
    assert res.counts == tuple(counts[k] for k in COUNT_KEYS) and np.array_equal(res.plane_id, ids)
    assert np.array_equal(res.planes["count"], planes["count"]) and np.array_equal(res.planes["seed"], planes["seed"])
    # the file: `plane` last, behind the colour (and behind `curvature` when that is written)
    on.save_reconstruction(xyz, rgb, str(tmp_path / "on.ply"), normals=on.cloud_normals, planes=on.cloud_plane_ids)
    names, rec = _parse(tmp_path / "on.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "plane"] and np.array_equal(rec["plane"], ids)
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), xyz)
    on.save_reconstruction(xyz, rgb, str(tmp_path / "c.ply"), normals=on.cloud_normals, curvature=dc, planes=on.cloud_plane_ids)
    assert _parse(tmp_path / "c.ply")[0] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "curvature", "plane"]


def test_curvature_is_still_written_only_when_asked_for(runs, scene):
    _, (on, _) = runs
    both, _ = _run(scene, cloud_curvature=True, **ON)
    assert both.cloud_curvature is not None and both.cloud_plane_ids.tobytes() == on.cloud_plane_ids.tobytes()
    assert both.cloud_planes.tobytes() == on.cloud_planes.tobytes()


def _partition(xyz, ids):
    """the ids in the order of the sorted points"""
    order = np.lexsort(np.asarray(xyz, np.float64).T[::-1])
    return np.asarray(xyz)[order], np.asarray(ids)[order]


def test_blocked_run_gives_the_single_lattices_partition(runs, scene):
    _, (one, (xyz, _, _)) = runs
    assert one.stats["blocks"] == 1
    many, (mxyz, _, _) = _run(scene, limit=one.grid.nvox // 3, **ON)
    assert many.stats["blocks"] >= 2 and "cloud_planes_s" in many.timings
    assert not np.array_equal(xyz, mxyz)                                   # the blocks' clouds come in another order
    (pa, a), (pb, b) = _partition(xyz, one.cloud_plane_ids), _partition(mxyz, many.cloud_plane_ids)
    assert pa.tobytes() == pb.tobytes()
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)                    # the numbering follows the order; the partition does not
    assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1])) and np.array_equal(a == -1, b == -1)
    assert {k: many.stats["cloud_planes"][k] for k in COUNT_KEYS} == {k: one.stats["cloud_planes"][k] for k in COUNT_KEYS}
    assert sorted(many.cloud_planes["count"].tolist()) == sorted(one.cloud_planes["count"].tolist())


def test_planes_without_normals_are_refused_before_anything_is_fused(scene):
    with pytest.raises(ValueError, match="needs cloud_normals"):
        _run(scene, cloud_planes=True)


def test_both_command_lines_write_the_property_and_the_report(scene, tmp_path, capsys):
    from PIL import Image
    import depth_enhanced_reconstruction as der
    import depth_to_reconstruction as d2r
    poses, frames = scene
    rgb_dir, depth_dir = tmp_path / "rgb", tmp_path / "depth"
    rgb_dir.mkdir()
    depth_dir.mkdir()
    for i, (d, c) in enumerate(frames):
        Image.fromarray(c[..., ::-1]).save(rgb_dir / f"frame_{i:04d}.png")
        np.save(depth_dir / f"frame_{i:04d}_depth.npy", d)
    cam = ["--fx", str(SMALL["fx"]), "--fy", str(SMALL["fy"]), "--cx", str(SMALL["cx"]), "--cy", str(SMALL["cy"])]
    flags = ["--cloud-normals", "--cloud-planes", "--cloud-planes-angle", "12", "--cloud-planes-min-points", "100", "--cloud-planes-max-curvature", "0.06"]
    common = ["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--no-vis", "--voxel-size", "0.025", "--grid", "128", *cam]
    plain, seg, report = tmp_path / "plain.ply", tmp_path / "p.ply", tmp_path / "planes.json"
    assert d2r.main(common + ["--output", str(plain)]) == 0
    assert d2r.main(common + ["--output", str(seg), *flags, "--cloud-planes-report", str(report)]) == 0
    names, base = _parse(plain)
    assert names == ["x", "y", "z", "red", "green", "blue"] and len(base) > 1000
    # without --cloud-planes the file is the bytes it always was: the old header, and nothing in a record but position and colour
    rec = np.empty(len(base), dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    for a, b in zip(("x", "y", "z", "r", "g", "b"), ("x", "y", "z", "red", "green", "blue")):
        rec[a] = base[b]
    head = ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {len(base)}\n" + "property double x\nproperty double y\nproperty double z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert plain.read_bytes() == head.encode("ascii") + rec.tobytes()
    again = tmp_path / "again.ply"                                          # the options' defaults spelled out, planes off: the same bytes
    assert d2r.main(common + ["--output", str(again), "--cloud-planes-angle", "10", "--cloud-planes-min-points", "200",
                              "--cloud-planes-max-curvature", "0.05"]) == 0
    assert again.read_bytes() == plain.read_bytes()
    names, rec = _parse(seg)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "plane"]
    for a in ("x", "y", "z", "red", "green", "blue"):
        assert np.array_equal(rec[a], base[a])
    rows = json.load(open(report))["planes"]
    assert len(rows) == int(rec["plane"].max()) + 1 and rec["plane"].min() >= -1
    assert [r["count"] for r in rows] == np.bincount(rec["plane"][rec["plane"] >= 0], minlength=len(rows)).tolist()
    assert all(r["count"] >= 100 and set(r) == {"normal", "d", "centroid", "rms", "count"} for r in rows)
    out = tmp_path / "der"
    assert der.main(["--input", str(rgb_dir), "--depth-folder", str(depth_dir), "--output", str(out), *cam, *flags, "--cloud-curvature",
                     "--cloud-planes-report", str(out / "planes.json")]) == 0
    names, rec = _parse(out / "reconstruction.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "curvature", "plane"] and len(rec) > 1000
    der_args = ["--input", str(rgb_dir), "--depth-folder", str(depth_dir), *cam]
    assert der.main(der_args + ["--output", str(tmp_path / "der_n"), "--cloud-normals", "--cloud-curvature"]) == 0
    names, without = _parse(tmp_path / "der_n" / "reconstruction.ply")         # the same run without the planes: the same file but for `plane`
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "curvature"]
    assert all(np.array_equal(without[a], rec[a]) for a in names)
    rows = json.load(open(out / "planes.json"))["planes"]
    assert [r["count"] for r in rows] == np.bincount(rec["plane"][rec["plane"] >= 0], minlength=len(rows)).tolist()
    capsys.readouterr()
    for cli, args in ((d2r, common), (der, ["--input", str(rgb_dir), "--output", str(out)])):
        with pytest.raises(SystemExit):
            cli.main(args + ["--cloud-planes"])
        assert "it needs --cloud-normals" in capsys.readouterr().err


def test_the_corridors_walls_floor_and_ceiling():
    """Six QVGA frames down the corridor of config 3 (the one the mesh tests fuse at VGA), 2 cm voxels, the pipeline's defaults.  The
    condition is stated on the reference alone: at least 4 accepted planes whose normals are pairwise within 10 degrees of parallel
    or of perpendicular.  Then the pipeline's arrays are the reference's."""
    cam = dict(fx=256.0, fy=256.0, cx=160.0, cy=120.0)
    poses = synth.dolly_poses(6, (0.0, 0.0, 0.0), (0.0, 0.0, 0.1))
    frames = [synth.render(synth.corridor_scene(), p, 320, 240, **cam) for p in poses]
    base = dict(**cam, voxel_size=VOXEL, subsample_factor=1, grid_dim=512, outlier_filter=False)
    pipe, (xyz, _, _) = _run((poses, frames), base=base, cloud_curvature=True, **ON)
    res = _reference(xyz, pipe.cloud_normals, pipe.cloud_curvature, VOXEL)
    nv = res.planes["normal"]
    print(f"corridor: {len(xyz)} points, counts {res.counts}, plane sizes {res.planes['count'].tolist()}, rms {np.round(res.planes['rms'], 5).tolist()}")
    assert len(nv) >= 4
    cos = np.abs(nv @ nv.T)
    assert np.all((cos >= math.cos(math.radians(10.0))) | (cos <= math.sin(math.radians(10.0))))
    assert len({tuple(np.round(np.abs(v)).astype(int)) for v in nv}) >= 2          # walls AND floor / ceiling: two directions at the least
    assert res.counts == tuple(pipe.stats["cloud_planes"][k] for k in COUNT_KEYS) and np.array_equal(res.plane_id, pipe.cloud_plane_ids)
    assert np.array_equal(res.planes["count"], pipe.cloud_planes["count"]) and np.array_equal(res.planes["seed"], pipe.cloud_planes["seed"])
