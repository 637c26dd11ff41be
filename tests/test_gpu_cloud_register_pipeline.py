"""GPU: compare_align in the pipeline and on the command line: the fused cloud is registered onto a reference
scan that lies in ANOTHER frame before it is scored.  The scan is a sampling of the true surface (the rendered depth back-projected
at the true poses, every third pixel), moved by a planted transform of 2 degrees and 3 cm, and for the scale case scaled by 1.05 too,
on the closed object scene.  The alignment is held to the numpy reference (tests/cloud_register_reference.py) run on the downloaded
fused cloud and the same scan, within the project's ICP parity bar of 1e-4.  The Chamfer distances are printed; DESIGN.md section 14
records them."""
import numpy as np
import pytest

import cloud_register_common as cc
import cloud_register_reference as cr
import tl3d
from tl3d import fileio, synth
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu

CAM = dict(fx=130.0, fy=130.0, cx=80.0, cy=60.0)
W, H = 160, 120
PLANTED = cc.pose((2, -1, 1), 2.0, (0.02, -0.01, 0.02))     # 2 degrees and 3 cm, reconstruction -> scan


def _surface(frames, rel, step=3):
    """The rendered depth back-projected into the first camera's frame (the reconstruction's), every step-th pixel."""
    v, u = np.mgrid[0:H:step, 0:W:step]
    out = []
    for (d, _), (R, t) in zip(frames, rel):
        z = d[v, u].astype(np.float64)
        cam = np.stack([(u - CAM["cx"]) / CAM["fx"] * z, (v - CAM["cy"]) / CAM["fy"] * z, z], axis=-1).reshape(-1, 3)
        cam = cam[np.isfinite(cam).all(axis=1) & (cam[:, 2] > 0.1) & (cam[:, 2] < 10.0)]
        out.append((cam - np.asarray(t).reshape(3)) @ np.asarray(R))
    return np.concatenate(out)


def _pipe(frames, **kw):
    cfg = ReconstructionConfig(**CAM, voxel_size=0.02, subsample_factor=1, grid_dim=256, **kw)
    pipe = DepthToReconstructionPipeline(cfg)
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    return pipe


def _runs(tmp, scene, poses, sigma, extract_mesh):
    r0, t0 = poses[0]
    rel = [(r @ r0.T, t.reshape(3, 1) - (r @ r0.T) @ t0.reshape(3, 1)) for r, t in poses]
    frames = [synth.render(scene, p, W, H, **CAM) for p in poses]
    surface = _surface(frames, rel)
    here, there = tmp / "here.ply", tmp / "there.ply"
    grey = np.full((len(surface), 3), 128, np.uint8)
    fileio.write_ply_binary(here, surface.astype(np.float32), grey)
    fileio.write_ply_binary(there, cc.move(surface.astype(np.float32), PLANTED, sigma), grey)
    out = {}
    for name, kw in (("plain", {}), ("unmoved", dict(compare_to=str(here))), ("unaligned", dict(compare_to=str(there))),
                     ("aligned", dict(compare_to=str(there), compare_align=True, compare_align_scale=sigma != 1.0))):
        pipe = _pipe(frames, extract_mesh=extract_mesh, **kw)
        pts, col, _ = pipe.reconstruct(poses=rel)
        out[name] = (pipe, pts, col)
    out["scan"] = fileio.read_ply_points(there)
    return out


@pytest.fixture(scope="module")
def rigid(tmp_path_factory):
    return _runs(tmp_path_factory.mktemp("rigid"), synth.plane_sphere_scene(), synth.dolly_poses(3, (-0.02, 0.0, 0.0), (0.02, 0.0, 0.0)), 1.0, True)


@pytest.fixture(scope="module")
def scaled(tmp_path_factory):
    return _runs(tmp_path_factory.mktemp("scaled"), synth.object_scene(), synth.orbit_poses(3, 1.0, 20.0), 1.05, False)


def _check(runs, sigma, what):
    pipe, pts, _ = runs["aligned"]
    al = pipe.stats["compare"]["alignment"]
    assert sorted(al) == ["T", "fitness", "iters_run", "n_corr", "rmse", "scale", "status"]
    T = np.array(al["T"])
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as ctx:
        normals = ctx.estimate_normals(runs["scan"])
    ref = cr.register(np.asarray(pts, np.float32), runs["scan"], normals, estimate_scale=sigma != 1.0, nearest=cr.nearest_kdtree)
    dT, ds = float(np.linalg.norm(T - ref["T"])), abs(al["scale"] - ref["scale"])
    ch = {k: runs[k][0].stats["compare"]["chamfer_mean"] for k in ("aligned", "unaligned", "unmoved")}
    print(f"{what}: {len(pts)} points against {len(runs['scan'])}; |T - T_ref|_F {dT:.3g}, |scale - scale_ref| {ds:.3g}; to the planted "
          f"transform {np.linalg.norm(T - PLANTED):.3g}, scale {al['scale']:.6g} (planted {sigma}); status {al['status']}, iters {al['iters_run']}, "
          f"fitness {al['fitness']:.4f}, rmse {al['rmse']:.4g}; chamfer aligned {ch['aligned']:.6g}, unaligned {ch['unaligned']:.6g}, "
          f"unmoved scan without alignment {ch['unmoved']:.6g}")
    assert dT <= cc.PARITY and ds <= cc.PARITY
    assert al["iters_run"] == ref["iters_run"] and al["status"] == ref["status"] and al["n_corr"] == ref["n_corr"]
    assert ch["aligned"] < ch["unaligned"]
    if sigma == 1.0:
        assert al["scale"] == 1.0


def test_alignment_is_the_references_and_chamfer_drops(rigid):
    _check(rigid, 1.0, "plane and sphere")
    cmp = rigid["aligned"][0].stats["compare"]
    plain = rigid["unaligned"][0].stats["compare"]
    assert cmp["mesh"]["points_to_surface"]["mean"] < plain["mesh"]["points_to_surface"]["mean"]     # the mesh's vertices were moved too


def test_alignment_with_scale_on_the_closed_scene(scaled):
    _check(scaled, 1.05, "object in its room, scale 1.05")


def test_outputs_do_not_move(rigid, tmp_path):
    (plain, pts, col), (on, pts2, col2), (off, pts3, _) = rigid["plain"], rigid["aligned"], rigid["unaligned"]
    assert np.array_equal(pts2, pts) and np.array_equal(col2, col) and np.array_equal(pts3, pts)
    for m2, m1 in zip(on.mesh, plain.mesh):
        assert np.array_equal(m2, m1)
    assert {k: v for k, v in on.stats.items() if k != "compare"} == plain.stats
    assert "alignment" not in off.stats["compare"]
    assert {k for k in on.stats["compare"]} - {"alignment"} == set(off.stats["compare"])
    a, b = tmp_path / "a.ply", tmp_path / "b.ply"
    fileio.write_ply_binary(a, pts, col)
    fileio.write_ply_binary(b, pts2, col2)
    assert a.read_bytes() == b.read_bytes()


def test_command_line(rigid, tmp_path, capsys):
    from PIL import Image
    import depth_to_reconstruction as cli
    poses = synth.dolly_poses(3, (-0.02, 0.0, 0.0), (0.02, 0.0, 0.0))
    frames = [synth.render(synth.plane_sphere_scene(), p, W, H, **CAM) for p in poses]
    rgb_dir, depth_dir = tmp_path / "rgb", tmp_path / "depth"
    rgb_dir.mkdir()
    depth_dir.mkdir()
    for k, (d, c) in enumerate(frames):
        Image.fromarray(c[..., ::-1]).save(rgb_dir / f"frame_{k:04d}.png")
        np.save(depth_dir / f"frame_{k:04d}_depth.npy", d)
    common = ["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--fx", "130", "--fy", "130", "--cx", "80", "--cy", "60",
              "--voxel-size", "0.02", "--grid", "256", "--no-vis"]
    first, second = tmp_path / "first.ply", tmp_path / "second.ply"
    assert cli.main(common + ["--output", str(first)]) == 0
    # the first run's own output, moved: the registration brings it back, and the written file is the first run's
    moved = tmp_path / "moved.ply"
    p = fileio.read_ply_points(first)
    fileio.write_ply_binary(moved, cc.move(p, PLANTED), np.full((len(p), 3), 128, np.uint8))
    np.savetxt(tmp_path / "init.txt", np.eye(4))
    capsys.readouterr()
    assert cli.main(common + ["--output", str(second), "--compare-to", str(moved), "--compare-align", "--compare-align-init", str(tmp_path / "init.txt"),
                              "--compare-threshold", "0.01"]) == 0
    out = capsys.readouterr().out
    assert len([ln for ln in out.splitlines() if "Align: status" in ln]) == 1 and len([ln for ln in out.splitlines() if "Compare:" in ln]) == 1
    assert first.read_bytes() == second.read_bytes()
    with pytest.raises(SystemExit):
        cli.main(common + ["--output", str(second), "--compare-align"])
    assert "needs compare_to" in capsys.readouterr().err
