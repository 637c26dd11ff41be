"""GPU: ray casting of the TSDF channel (tl3d_raycast) against the numpy restatement of the rules
(tests/raycast_reference.py) on fused and crafted grids, dense and sparse; host / device outputs; the frame-slot path into
normals, ICP and fusion; errors; the pipeline option and the command-line flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

import raycast_reference as rr
import tl3d
from helpers import SMALL, make_pair, small_scene_frames
from tl3d import _cabi as abi
from tl3d import synth
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, VOXEL, CENTRE = (96, 96, 96), 0.025, (0.0, -0.2, 0.0)


def _spec_of(ctx):
    g = ctx.grid
    return tuple(g.dims), tuple(g.origin), g.voxel_size, g.sdf_trunc


def _assert_same(got, want):
    for a, b, name in zip(got, want, ("depth", "normals", "bgr")):
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), (name, int((a != b).sum()))


def _reference(ctx, tsdf, pose, min_weight=0, centroid=None):
    dims, origin, voxel, trunc = _spec_of(ctx)
    return rr.raycast(tsdf, dims, origin, voxel, trunc, SMALL, pose, min_weight=min_weight, z_near=ctx.min_depth,
                      z_far=ctx.max_depth, centroid=centroid)[:3]


def _novel_pose(poses):
    """between the first two fused cameras, a little closer to the scene"""
    R = synth.orbit_poses(9, 1.0, 5.0)[1][0]
    t = 0.5 * (np.asarray(poses[0][1]) + np.asarray(poses[1][1])) - np.array([0.0, 0.0, 0.05]).reshape(np.shape(poses[0][1]))
    return R, t


def _fused_pair(n=6, deg=8.0):
    poses, frames = small_scene_frames(n=n, deg=deg)
    ctx, orc = make_pair(dims=DIMS, voxel=VOXEL, centre=CENTRE, n_slots=n + 2)
    for i, ((depth, bgr), pose) in enumerate(zip(frames, poses)):
        ctx.upload(i, depth, bgr)
        ctx.integrate(i, pose)
        ctx.accumulate_centroid(i, pose)
        orc.tsdf_integrate(depth, pose[0], pose[1])
        orc.centroid_accumulate(depth, bgr, pose[0], pose[1])
    return ctx, orc, poses, frames


def test_fused_grid_view_equals_reference():
    ctx, orc, poses, frames = _fused_pair()
    with ctx:
        for mw in (0, 2):
            for pose in (poses[0], poses[3], _novel_pose(poses)):
                got = ctx.raycast(pose, min_weight=mw)
                want = _reference(ctx, orc.tsdf, pose, mw, orc.centroid)
                assert (want[0] > 0).sum() > 2000
                assert (want[2] != 128).any()
                _assert_same(got, want)


def _crafted(dims, voxel, origin):
    """{sum, weight} volumes: spheres cut by the grid's faces, weights 1..3, an unobserved slab and column, truncated voxels"""
    rng = np.random.default_rng(11)
    ii, jj, kk = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    p = np.stack([origin[a] + (g + 0.5) * voxel for a, g in enumerate((ii, jj, kk))], axis=-1)
    s1 = np.linalg.norm(p - np.array([0.1, 0.05, 0.6]), axis=-1) - 0.17
    s2 = np.linalg.norm(p - np.array([0.45, 0.2, 0.9]), axis=-1) - 0.3         # cut by the upper x and y faces
    s3 = np.linalg.norm(p - np.array([0.2, 0.1, 1.4]), axis=-1) - 0.2          # cut by the upper z face
    sdf = np.minimum(np.minimum(s1, s2), s3)
    t = np.clip(sdf / (3 * voxel), -1.0, 1.0)
    w = rng.integers(1, 4, size=dims)
    s = np.rint(t * 32767.0).astype(np.int64) * w
    far = np.abs(sdf) > 3.5 * voxel
    s[far] = np.sign(sdf[far]).astype(np.int64) * 32767 * w[far]
    w[:, :, 10:13] = 0                                                         # unobserved slab across a brick face
    s[:, :, 10:13] = 0
    w[5:9, 3:7, :] = 0
    s[5:9, 3:7, :] = 0
    return rr.records_from_volume(s, w)


def test_crafted_grid_view_equals_reference():
    dims, voxel, centre = (40, 24, 72), 0.02, (0.3, 0.2, 0.7)
    ctx, _ = make_pair(dims=dims, voxel=voxel, centre=centre, channels=tl3d.CH_TSDF)
    with ctx:
        _, origin, _, _ = _spec_of(ctx)
        rec = _crafted(dims, voxel, origin)
        ctx.upload_grid(tl3d.CH_TSDF, rec)
        c, s = np.cos(0.3), np.sin(0.3)
        views = [(np.eye(3), np.array([-0.3, -0.2, 0.2])),                     # camera at z = 0.5, looking along +z
                 (np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]]), np.array([-0.2, -0.2, 0.3])),
                 (np.eye(3), np.array([-0.05, -0.1, -1.0]))]                    # inside the volume, in front of the third sphere
        for mw in (0, 2):
            for pose in views:
                got = ctx.raycast(pose, min_weight=mw)
                want = _reference(ctx, rec, pose, mw)
                assert (want[0] > 0).sum() > (500 if mw == 0 else 30)       # (mw 2: a third of the voxels are gated out)
                _assert_same(got, want)
                assert (got[2] == 128).all()


def test_sparse_grid_renders_like_dense():
    poses, frames = small_scene_frames(n=5, deg=4.0)
    ctx, _ = make_pair(dims=DIMS, voxel=VOXEL, centre=CENTRE, n_slots=5)
    origin = tuple(CENTRE[i] - 0.5 * DIMS[i] * VOXEL for i in range(3))
    sp = tl3d.FusionContext(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], n_slots=5, grid=None)
    with ctx, sp:
        for c in (ctx, sp):
            for i, (d, col) in enumerate(frames):
                c.upload(i, d, col)
        geom = tl3d.GridSpec(DIMS, origin, VOXEL, 4 * VOXEL, tl3d.CH_TSDF | tl3d.CH_CENTROID)
        nt, nc = sp.count_bricks(geom, list(range(5)), poses, centroid_subsample=1)
        assert 0 < nt < 96 ** 3 // 512
        sp.attach_grid(tl3d.GridSpec(DIMS, origin, VOXEL, 4 * VOXEL, tl3d.CH_TSDF | tl3d.CH_CENTROID, pool_tsdf=nt + 8,
                                     pool_centroid=nc + 8))
        for c in (ctx, sp):
            for i in range(5):
                c.integrate(i, poses[i])
                c.accumulate_centroid(i, poses[i], subsample=1)
        for mw in (0, 2):
            for pose in (poses[2], _novel_pose(poses)):
                a = sp.raycast(pose, min_weight=mw)
                b = ctx.raycast(pose, min_weight=mw)
                assert (b[0] > 0).sum() > 2000
                _assert_same(a, b)


def test_device_outputs_and_flush_after_fuse_frames():
    import torch
    poses, frames = small_scene_frames(n=4, deg=4.0)
    ctx, _ = make_pair(dims=DIMS, voxel=VOXEL, centre=CENTRE, n_slots=4)
    with ctx:
        for i, (d, col) in enumerate(frames):
            ctx.upload(i, d, col)
        ctx.fuse_frames(list(range(4)), poses, centroid_subsample=1)
        early = ctx.raycast(poses[1])                    # straight after fuse_frames: the deferred batch is flushed first
        ctx.sync()
        late = ctx.raycast(poses[1])
        _assert_same(early, late)
        want = _reference(ctx, ctx.download_grid(tl3d.CH_TSDF), poses[1], 0, ctx.download_grid(tl3d.CH_CENTROID))
        _assert_same(late, want)
        H, W = SMALL["height"], SMALL["width"]
        dev = (torch.empty((H, W), dtype=torch.float32, device="cuda"), torch.empty((H, W, 3), dtype=torch.float32, device="cuda"),
               torch.empty((H, W, 3), dtype=torch.uint8, device="cuda"))
        ctx.raycast(poses[1], out=dev)
        _assert_same(tuple(t.cpu().numpy() for t in dev), late)
        # outputs may be left out, mixed host and device
        d_only = np.empty((H, W), np.float32)
        ctx.raycast(poses[1], out=(d_only, None, dev[2]))
        assert np.array_equal(d_only, late[0])


def test_fidelity_at_a_fused_pose():
    ctx, _, poses, frames = _fused_pair(n=6, deg=8.0)
    with ctx:
        for k in (0, 4):
            depth, nrm, _ = ctx.raycast(poses[k])
            z = frames[k][0].astype(np.float64)
            R, t = (np.asarray(p, np.float64) for p in poses[k])
            vv, uu = np.mgrid[0:SMALL["height"], 0:SMALL["width"]]
            pc = np.stack([(uu - SMALL["cx"]) / SMALL["fx"] * z, (vv - SMALL["cy"]) / SMALL["fy"] * z, z], axis=-1)
            pw = (pc - t.reshape(1, 1, 3)) @ R                                  # R^T (p - t)
            g = (pw - np.array(ctx.grid.origin)) / VOXEL - 0.5
            in_grid = (z > 0) & np.all((g > 3) & (g < np.array(DIMS) - 4), axis=-1)
            # away from occluding edges (depth range over 5 x 5 pixels below 2 voxels) and the image border: the surface the
            # frames saw head-on.  (At an occluding edge a ray passes through the band behind the nearer surface.)
            win = np.lib.stride_tricks.sliding_window_view(np.pad(z, 2, mode="edge"), (5, 5))
            in_grid &= (win.max(axis=(2, 3)) - win.min(axis=(2, 3))) < 2 * VOXEL
            in_grid[:3] = in_grid[-3:] = False
            in_grid[:, :3] = in_grid[:, -3:] = False
            assert in_grid.sum() > 3000
            cover = (depth[in_grid] > 0).mean()
            both = in_grid & (depth > 0)
            med = np.median(np.abs(depth[both] - z[both])) / VOXEL
            print(f"view {k}: coverage {cover:.4f}, median |dz| {med:.4f} voxel")
            assert cover >= 0.95
            assert med < 0.1
            assert (np.linalg.norm(nrm[both], axis=-1) > 0.99).mean() > 0.95


def test_slot_path_feeds_normals_icp_and_fusion():
    ctx, _, poses, frames = _fused_pair(n=6, deg=2.0)
    k = 7
    with ctx:
        # the model at camera 3 in slot k: frame 2 registers onto it like onto frame 3
        depth, _, bgr = ctx.raycast(poses[3], slot=k)
        assert np.array_equal(ctx.download_depth(k), depth)
        ctx.build_normals(k, depth_jump=0.02)                 # (no normals across the model's occluding edges)
        res = ctx.icp(2, k, iters=30, stride=1, max_dist=0.02)
        r_rel, t_rel = synth.relative_pose(poses[2], poses[3])
        ang = np.degrees(np.arccos(np.clip((np.trace(res["T"][:3, :3] @ np.asarray(r_rel).T) - 1) / 2, -1, 1)))
        dt = np.linalg.norm(res["T"][:3, 3] - np.asarray(t_rel).ravel())
        print(f"ICP onto the model view: {dt / VOXEL:.4f} voxel, {ang:.4f} deg, status {res['status']}")
        assert dt < 0.1 * VOXEL and ang < 0.1
    # a slot that held a 16-bit frame fuses from the rendered f32 image afterwards
    ctx, orc, poses, frames = _fused_pair(n=4, deg=6.0)
    fresh, orc2 = make_pair(dims=DIMS, voxel=VOXEL, centre=CENTRE, n_slots=1)
    fresh.close()
    with ctx:
        mm = np.clip(np.rint(frames[0][0] * 1000.0), 0, 65535).astype(np.uint16)
        ctx.upload(5, mm, frames[0][1])
        depth, _, _ = ctx.raycast(poses[1], slot=5)
        assert (depth > 0).sum() > 2000
        ctx.reset()
        ctx.integrate(5, poses[1])
        orc2.tsdf_integrate(depth, poses[1][0], poses[1][1])
        assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), orc2.tsdf)


def test_errors():
    cen_only, _ = make_pair(dims=(16, 16, 16), channels=tl3d.CH_CENTROID)
    with cen_only:
        with pytest.raises(abi.Tl3dError) as e:
            cen_only.raycast((np.eye(3), np.zeros(3)))
        assert e.value.code == abi.E_STATE and "TSDF" in str(e.value)
    ctx, _ = make_pair(dims=(16, 16, 16), n_slots=2)
    with ctx:
        with pytest.raises(abi.Tl3dError) as e:
            ctx.raycast((np.eye(3), np.zeros(3)), slot=2)
        assert e.value.code == abi.E_INVALID and "slot" in str(e.value)
        lib = abi.load()
        assert lib.tl3d_raycast(ctx._h, None, None, 0, 0.0, 0.0, -1, None, None, None) == abi.E_INVALID


# ---- pipeline and command line --------------------------------------------------------------------------------------
CAM = dict(fx=525.0, fy=525.0, cx=320.0, cy=240.0)
W, H = 640, 480


def _object_sequence(n):
    scene = synth.object_scene(with_room=True)
    poses = synth.orbit_poses(n, 1.0, 1.5)
    r0, t0 = poses[0]
    rel = []
    for r, t in poses:
        rr_ = r @ r0.T
        rel.append((rr_, t.reshape(3, 1) - rr_ @ t0.reshape(3, 1)))
    frames = [synth.render(scene, p, W, H, **CAM) for p in poses]
    return scene, poses, rel, frames


def test_pipeline_render_dir(tmp_path):
    _, _, rel, frames = _object_sequence(6)
    cfg = ReconstructionConfig(**CAM, voxel_size=0.005, subsample_factor=2, grid_dim=256, tsdf_min_weight=1,
                               render_dir=str(tmp_path / "views"))
    pipe = DepthToReconstructionPipeline(cfg)
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    pipe.reconstruct(poses=rel)
    assert pipe.stats["render_views"] == len(pipe.frame_index) == 6 and "render_s" in pipe.timings
    res = pipe.stats["render_residual_mm"]
    print("render residual (mm):", res)
    assert all(r is not None and r < 0.25 * cfg.voxel_size * 1e3 for r in res)
    names = sorted(os.listdir(tmp_path / "views"))
    assert len(names) == 18 and all(n.startswith("frame_") for n in names)
    # the .npy is what raycast gives at that pose on the same fused grid
    grid = pipe.grid
    with tl3d.FusionContext(W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], cfg.min_depth, cfg.max_depth, n_slots=6, grid=grid) as ctx:
        for i, (d, c) in enumerate(frames):
            ctx.upload(i, d, c)
        ctx.fuse_frames(pipe.frame_index, pipe.camera_poses, [pipe.scales[i] for i in pipe.frame_index],
                        centroid_subsample=cfg.subsample_factor)
        for i in (0, 5):
            want = ctx.raycast(pipe.camera_poses[i], min_weight=1)[0]
            got = np.load(tmp_path / "views" / f"frame_{i:04d}_model_depth.npy")
            assert np.array_equal(got, want)
    # without the option nothing is rendered
    cfg2 = ReconstructionConfig(**CAM, voxel_size=0.005, subsample_factor=2, grid_dim=256, tsdf_min_weight=1)
    pipe2 = DepthToReconstructionPipeline(cfg2)
    pipe2.set_frames([c for d, c in frames], [d for d, c in frames])
    pipe2.reconstruct(poses=rel)
    assert "render_views" not in pipe2.stats and "render_s" not in pipe2.timings


def test_cli_render_output(tmp_path):
    from PIL import Image
    _, _, _, frames = _object_sequence(5)
    rgb_dir, depth_dir = tmp_path / "rgb", tmp_path / "depth"
    rgb_dir.mkdir(); depth_dir.mkdir()
    for i, (d, c) in enumerate(frames):
        Image.fromarray(c[..., ::-1]).save(rgb_dir / f"frame_{i:04d}.png")
        np.save(depth_dir / f"frame_{i:04d}_depth.npy", d)
    common = ["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--fx", "525", "--fy", "525", "--cx", "320", "--cy", "240",
              "--no-vis", "--tsdf-min-weight", "1", "--grid", "256"]
    env = dict(os.environ)
    exe = [sys.executable, os.path.join(ROOT, "depth_to_reconstruction.py"), *common]

    def run(*extra):
        r = subprocess.run(exe + list(extra), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r
    plain, with_views, views = tmp_path / "plain.ply", tmp_path / "v.ply", tmp_path / "views"
    before = set(os.listdir(tmp_path))
    run("--output", str(plain))
    assert set(os.listdir(tmp_path)) - before == {"plain.ply"}
    r = run("--output", str(with_views), "--render-output", str(views))
    assert plain.read_bytes() == with_views.read_bytes()
    names = sorted(os.listdir(views))
    kept = r.stdout.count(": fused")
    assert kept >= 2 and len([n for n in names if n.endswith("_model_depth.npy")]) == kept and len(names) == 3 * kept
    for n in names:
        if n.endswith("_model_depth.npy"):
            d = np.load(views / n)
            assert d.shape == (H, W) and d.dtype == np.float32 and (d > 0).mean() > 0.3
            png = np.asarray(Image.open(views / n.replace(".npy", ".png")))
            assert png.dtype == np.uint16 and np.array_equal(png, np.clip(d * 1000.0, 0, 65535).astype(np.uint16))
            col = np.asarray(Image.open(views / n.replace("_model_depth.npy", "_model_color.png")))
            assert col.shape == (H, W, 3)
