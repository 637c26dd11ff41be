"""GPU: config.cloud_normals / cloud_curvature through the pipeline, the saved files and both command lines (DESIGN.md section
4.5), on the SMALL scene of tests/helpers.py: off by default with no trace; on, the bytes of a direct FusionContext.estimate_normals
call with the camera centres as viewpoints, within the bars of tests/cloud_normals_common.py of the fp64 reference run on the
pipeline's own cloud; the same normals from a blocked run."""
import numpy as np
import pytest

import cloud_normals_common as cn
import tl3d
from helpers import SMALL, small_scene_frames
from tl3d import fileio
from tl3d import pipeline as pl
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu

CAM = {k: SMALL[k] for k in ("fx", "fy", "cx", "cy")}
VOXEL = 0.02
BASE = dict(**CAM, voxel_size=VOXEL, subsample_factor=1, grid_dim=128)


@pytest.fixture(scope="module")
def scene():
    # 2 mm of depth noise: the noise-free renders put voxel centroids on regular patterns whose exact ties at the k-th distance
    # hand the choice of a member to the index, and the blocked run numbers the points another way
    return small_scene_frames(n=3, noise=0.002)


def _run(scene, limit=None, **kw):
    poses, frames = scene
    old = pl.MAX_BLOCK_VOXELS
    try:
        if limit is not None:
            pl.MAX_BLOCK_VOXELS = limit
        pipe = DepthToReconstructionPipeline(ReconstructionConfig(**BASE, **kw))
        pipe.set_frames([c for d, c in frames], [d for d, c in frames])
        out = pipe.reconstruct(poses=poses)
    finally:
        pl.MAX_BLOCK_VOXELS = old
    return pipe, out


@pytest.fixture(scope="module")
def runs(scene):
    return _run(scene), _run(scene, cloud_normals=True, cloud_curvature=True)


def _centres(poses):
    return np.array([-np.asarray(R, np.float64).T @ np.asarray(t, np.float64).reshape(3) for R, t in poses])


def _parse(path):
    """(property names, structured vertex array) of a binary PLY cloud"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    props = [ln.split()[1:] for ln in head if ln.startswith("property")]
    types = {"double": "<f8", "float": "<f4", "uchar": "u1"}
    nv = int(next(ln for ln in head if ln.startswith("element vertex")).split()[-1])
    rec = np.frombuffer(data, np.dtype([(nm, types[t]) for t, nm in props]), nv, end)
    assert len(data) == end + nv * rec.dtype.itemsize
    return [nm for _, nm in props], rec


def test_off_by_default_leaves_no_trace(runs, tmp_path):
    (off, (xyz, rgb, _)), _ = runs
    assert off.cloud_normals is None and off.cloud_curvature is None
    assert "cloud_normals" not in off.stats and "cloud_normals_s" not in off.timings
    off.save_reconstruction(xyz, rgb, str(tmp_path / "off.ply"))
    rec = np.empty(len(xyz), dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    for a, col in zip("xyz", xyz.T):
        rec[a] = col
    for a, col in zip("rgb", np.asarray(rgb).T):
        rec[a] = col
    head = ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {len(xyz)}\n" + "property double x\nproperty double y\nproperty double z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert len(xyz) > 1000 and (tmp_path / "off.ply").read_bytes() == head.encode("ascii") + rec.tobytes()


def test_on_gives_the_direct_calls_normals_within_the_bar(runs, scene):
    (off, (xyz0, rgb0, _)), (on, (xyz, rgb, poses)) = runs
    assert xyz.tobytes() == xyz0.tobytes() and np.asarray(rgb).tobytes() == np.asarray(rgb0).tobytes()
    n = len(xyz)
    assert on.cloud_normals.shape == (n, 3) and on.cloud_normals.dtype == np.float32
    assert on.cloud_curvature.shape == (n,) and on.cloud_curvature.dtype == np.float32
    centres = _centres(poses)
    assert len(centres) == 3 == len(scene[0])
    p32 = xyz.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), xyz)                     # the returned points are the float32 cloud, widened
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as ctx:
        dn, dc = ctx.estimate_normals(p32, 30, viewpoints=centres, cell_size=2 * VOXEL, curvature=True)
        deg = ctx.last_normals_degenerate
    assert on.cloud_normals.tobytes() == dn.tobytes() and on.cloud_curvature.tobytes() == dc.tobytes()
    assert on.stats["cloud_normals"] == dict(neighbors=30, radius=0.0, viewpoints=3, degenerate=deg)
    assert set(on.stats) - set(off.stats) == {"cloud_normals"} and set(on.timings) - set(off.timings) == {"cloud_normals_s"}
    assert on.timings["cloud_normals_s"] >= 0
    # the reference on the pipeline's own cloud.  Its k-d tree does not know the tie rule: a point with a tie at the k-th distance
    # is held to the brute-force reference instead, which does.
    from scipy.spatial import cKDTree
    d, _ = cKDTree(xyz).query(xyz, k=31)
    tied = np.flatnonzero(d[:, 29] == d[:, 30])
    print(f"pipeline cloud: {n} points, {len(tied)} with a tie at the 30th distance")
    assert len(tied) <= n // 100
    r = cn.ref(p32, 30, viewpoints=centres)
    if len(tied):
        b = cn.brute(p32, 30, viewpoints=centres, rows=tied)
        cn.check(on.cloud_normals[tied], on.cloud_curvature[tied], b, False, "pipeline cloud, tied points", allow_excluded=True)
        free = np.setdiff1d(np.arange(n), tied)
        r = cn.Result(r.normals[free], r.curvature[free], r.lam[free], r.members[free], r.degenerate[free])
        cn.check(on.cloud_normals[free], on.cloud_curvature[free], r, False, "pipeline cloud", allow_excluded=True)
        assert deg == int(r.degenerate.sum()) + int(b.degenerate.sum())
    else:
        cn.check(on.cloud_normals, on.cloud_curvature, r, False, "pipeline cloud", allow_excluded=True)
        assert deg == int(r.degenerate.sum())
    to = centres[None, :, :] - xyz[:, None, :]
    to = to[np.arange(n), (to * to).sum(axis=-1).argmin(axis=1)]
    assert np.all((on.cloud_normals.astype(np.float64) * to).sum(axis=1) >= 0)
    # normals alone
    only, _ = _run(scene, cloud_normals=True, cloud_normals_neighbors=12, cloud_normals_radius=0.1)
    assert only.cloud_curvature is None and only.cloud_normals.shape == (n, 3)
    assert only.stats["cloud_normals"]["neighbors"] == 12 and only.stats["cloud_normals"]["radius"] == 0.1
    assert not np.array_equal(only.cloud_normals, on.cloud_normals)


def test_saved_files_carry_the_attributes(runs, tmp_path):
    _, (on, (xyz, rgb, _)) = runs
    on.save_reconstruction(xyz, rgb, str(tmp_path / "on.ply"), normals=on.cloud_normals, curvature=on.cloud_curvature)
    names, rec = _parse(tmp_path / "on.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "curvature"]
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), xyz)
    assert np.array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], 1).astype(np.float32), on.cloud_normals)
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), rgb) and np.array_equal(rec["curvature"], on.cloud_curvature)
    assert np.array_equal(fileio.read_ply_points(tmp_path / "on.ply"), xyz.astype(np.float32))
    on.save_reconstruction(xyz, rgb, str(tmp_path / "n.ply"), normals=on.cloud_normals)
    assert _parse(tmp_path / "n.ply")[0] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]


def _sorted_rows(*cols):
    a = np.concatenate([np.asarray(c, np.float64).reshape(len(c), -1) for c in cols], axis=1)
    return a[np.lexsort(a.T[::-1])]


def test_blocked_run_gives_the_single_lattices_normals(runs, scene):
    _, (one, (xyz, rgb, _)) = runs
    assert one.stats["blocks"] == 1
    many, (mxyz, mrgb, _) = _run(scene, limit=one.grid.nvox // 3, cloud_normals=True, cloud_curvature=True)
    assert many.stats["blocks"] >= 2 and "cloud_normals_s" in many.timings
    assert not np.array_equal(xyz, mxyz)                                   # the blocks' clouds come in another order
    a = _sorted_rows(xyz, rgb, one.cloud_normals, one.cloud_curvature)
    b = _sorted_rows(mxyz, mrgb, many.cloud_normals, many.cloud_curvature)
    assert a.tobytes() == b.tobytes(), f"{(a != b).any(axis=1).sum()} of {len(a)} points differ between the single and the blocked run"
    assert many.stats["cloud_normals"] == one.stats["cloud_normals"]


def test_curvature_alone_is_refused_before_anything_is_fused(scene):
    with pytest.raises(ValueError, match="needs cloud_normals"):
        _run(scene, cloud_curvature=True)


def test_both_command_lines_write_the_properties(scene, tmp_path):
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
    flags = ["--cloud-normals", "--cloud-normals-neighbors", "12", "--cloud-normals-radius", "0.2"]
    common = ["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--no-vis", "--voxel-size", "0.025", "--grid", "128", *cam]
    plain, nrm, cur = tmp_path / "plain.ply", tmp_path / "n.ply", tmp_path / "c.ply"
    assert d2r.main(common + ["--output", str(plain)]) == 0
    assert d2r.main(common + ["--output", str(nrm), *flags]) == 0
    assert d2r.main(common + ["--output", str(cur), *flags, "--cloud-curvature"]) == 0
    names, base = _parse(plain)
    assert names == ["x", "y", "z", "red", "green", "blue"] and len(base) > 1000
    names, with_n = _parse(nrm)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    names, with_c = _parse(cur)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "curvature"]
    for rec in (with_n, with_c):
        for a in ("x", "y", "z", "red", "green", "blue"):
            assert np.array_equal(rec[a], base[a])
        length = np.sqrt(rec["nx"] ** 2 + rec["ny"] ** 2 + rec["nz"] ** 2)
        assert np.all((np.abs(length - 1) <= cn.F32) | (length == 0)) and (length > 0).mean() > 0.99
    assert np.array_equal(with_n["nx"], with_c["nx"]) and np.all(with_c["curvature"] >= -1e-6) and np.all(with_c["curvature"] <= 1 / 3 + 1e-6)
    out = tmp_path / "der"
    assert der.main(["--input", str(rgb_dir), "--depth-folder", str(depth_dir), "--output", str(out), *cam, *flags, "--cloud-curvature"]) == 0
    names, rec = _parse(out / "reconstruction.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "curvature"] and len(rec) > 1000
    length = np.sqrt(rec["nx"] ** 2 + rec["ny"] ** 2 + rec["nz"] ** 2)
    assert np.all((np.abs(length - 1) <= cn.F32) | (length == 0)) and (length > 0).mean() > 0.99
