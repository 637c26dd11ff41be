"""GPU: point-to-SDF tracking against the TSDF channel (tl3d_track_evaluate / tl3d_track_frame) against the
numpy restatement (tests/track_reference.py) on fused and crafted grids, dense and sparse; repeatability and the flush; convergence;
too few correspondences; errors; the pipeline option, its refusals and the command-line flag."""
import os

import numpy as np
import pytest

import track_reference as tr
import tl3d
from helpers import SMALL, make_pair, small_scene_frames
from tl3d import _cabi as abi
from tl3d import synth
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline
from track_common import (ARC, CRAFTED_CENTRE, CRAFTED_DIMS, CRAFTED_VOXEL, FINE_CENTRE, FINE_DIMS, FINE_VOXEL, LEVELS, arc_frames, centre_errors_mm,
                          crafted_depth, crafted_records, crafted_views, novel_pose, offset_pose, pose_delta)

pytestmark = pytest.mark.gpu
DIMS, VOXEL, CENTRE = (96, 96, 96), 0.025, (0.0, -0.2, 0.0)       # the fused grid of the ray-cast tests


def _spec_of(ctx):
    g = ctx.grid
    return tuple(g.dims), tuple(g.origin), g.voxel_size, g.sdf_trunc


def _fused_pair(n=6, deg=8.0, extra_slots=2):
    """the ray-cast tests' recipe: n frames of small_scene_frames integrated at their poses (TSDF only is read here)"""
    poses, frames = small_scene_frames(n=n, deg=deg)
    ctx, _ = make_pair(dims=DIMS, voxel=VOXEL, centre=CENTRE, n_slots=n + extra_slots, channels=tl3d.CH_TSDF)
    for i, ((depth, bgr), pose) in enumerate(zip(frames, poses)):
        ctx.upload(i, depth, bgr)
        ctx.integrate(i, pose)
    return ctx, poses, frames


def _between(poses):
    """between the first two fused cameras, a little closer to the scene"""
    R = synth.orbit_poses(9, 1.0, 5.0)[1][0]
    t = 0.5 * (np.asarray(poses[0][1]) + np.asarray(poses[1][1])) - np.array([0.0, 0.0, 0.05]).reshape(np.shape(poses[0][1]))
    return R, t


def _check_pass(ctx, rec, slot, depth, pose, stride, gate, mw, what):
    """one track_evaluate against the reference: exact counts, every sum within the fp64 reordering bound.  The device adds the
    reference's very terms (f32 values, exact fp64 products) in another order: n_corr terms summed in any order differ from their
    exactly rounded sum by at most (n_corr - 1) u sum|term| (1 + O(n u)), u = 2^-53 -- n_corr 2^-52 sum|term| holds it twice over."""
    dims, origin, voxel, trunc = _spec_of(ctx)
    got = ctx.track_evaluate(slot, pose, stride=stride, max_dist=gate, min_weight=mw)
    want = tr.sums(rec, dims, origin, voxel, trunc, SMALL, depth, pose, stride=stride, max_dist=gate, min_weight=mw, min_depth=ctx.min_depth,
                   max_depth=ctx.max_depth)
    assert want["n_corr"] > 500, (what, want["n_corr"])
    assert got["n_src"] == want["n_src"] and got["n_corr"] == want["n_corr"], (what, got["n_src"], want["n_src"], got["n_corr"], want["n_corr"])
    bound = want["n_corr"] * 2.0 ** -52 * want["abs"]
    g = np.concatenate([got["A"][np.triu_indices(6)], got["b"], [got["e"]]])
    w = np.concatenate([want["A"], want["b"], [want["e"]]])
    assert np.all(np.abs(g - w) <= bound), (what, np.max(np.abs(g - w) / np.maximum(bound, 1e-300)))
    return got


def test_evaluate_equals_reference_on_a_fused_grid():
    ctx, poses, frames = _fused_pair()
    with ctx:
        rec = ctx.download_grid(tl3d.CH_TSDF)
        mid = _between(poses)                              # a frame of its own, seen from between two fused cameras
        frames.append(synth.render(synth.object_scene(), mid, SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], seed=60))
        ctx.upload(6, frames[6][0], None)
        cases = [(3, poses[3], "fused pose"), (6, mid, "between two cameras"),
                 (2, offset_pose(poses[2], 0.0, VOXEL), "1 voxel off"), (4, offset_pose(poses[4], 0.5, 0.0), "0.5 degrees off"),
                 (0, offset_pose(poses[0], 0.5, VOXEL), "1 voxel and 0.5 degrees off")]
        for slot, pose, name in cases:
            for stride in (1, 2, 3):                       # 3: partial tiles, ceil(160 / 3) = 54 columns
                for mw in (0, 2):
                    for gate in (VOXEL, 3 * VOXEL):
                        _check_pass(ctx, rec, slot, frames[slot][0], pose, stride, gate, mw, (name, stride, mw, gate))


def test_evaluate_equals_reference_on_a_crafted_grid():
    """unobserved slab and column, spheres cut by the grid's faces, weights 1..3; the third view is a camera inside the volume.  (The
    weight gate at 2 leaves 4 % of this grid's cells, below the 500 correspondences every case must have: it is exercised on the
    fused grid.)"""
    ctx, _ = make_pair(dims=CRAFTED_DIMS, voxel=CRAFTED_VOXEL, centre=CRAFTED_CENTRE, channels=tl3d.CH_TSDF, n_slots=3)
    with ctx:
        rec = crafted_records()
        ctx.upload_grid(tl3d.CH_TSDF, rec)
        for slot, view in enumerate(crafted_views()):
            depth = crafted_depth(rec, view)
            ctx.upload(slot, depth, None)
            for pose, name in ((view, "at the view"), (offset_pose(view, 0.25, 0.5 * CRAFTED_VOXEL), "half a voxel and 0.25 degrees off")):
                for stride in (1, 2, 3):
                    for gate in (CRAFTED_VOXEL, 3 * CRAFTED_VOXEL):
                        _check_pass(ctx, rec, slot, depth, pose, stride, gate, 0, (slot, name, stride, gate))
            # 1 voxel and 0.5 degrees off, the 1-voxel gate keeps more than 500 correspondences of these small views at stride 1 only
            pose = offset_pose(view, 0.5, CRAFTED_VOXEL)
            for stride, gate in ((1, CRAFTED_VOXEL), (1, 3 * CRAFTED_VOXEL), (2, 3 * CRAFTED_VOXEL), (3, 3 * CRAFTED_VOXEL)):
                _check_pass(ctx, rec, slot, depth, pose, stride, gate, 0, (slot, "1 voxel and 0.5 degrees off", stride, gate))


def test_sparse_grid_gives_the_dense_grids_sums():
    poses, frames = small_scene_frames(n=5, deg=4.0)
    ctx, _ = make_pair(dims=DIMS, voxel=VOXEL, centre=CENTRE, n_slots=5, channels=tl3d.CH_TSDF)
    origin = tuple(CENTRE[i] - 0.5 * DIMS[i] * VOXEL for i in range(3))
    sp = tl3d.FusionContext(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], n_slots=5, grid=None)
    with ctx, sp:
        for c in (ctx, sp):
            for i, (d, col) in enumerate(frames):
                c.upload(i, d, col)
        geom = tl3d.GridSpec(DIMS, origin, VOXEL, 4 * VOXEL, tl3d.CH_TSDF)
        nt, _ = sp.count_bricks(geom, list(range(5)), poses, centroid_subsample=1)
        assert 0 < nt < 96 ** 3 // 512
        sp.attach_grid(tl3d.GridSpec(DIMS, origin, VOXEL, 4 * VOXEL, tl3d.CH_TSDF, pool_tsdf=nt + 8))
        for c in (ctx, sp):
            for i in range(5):
                c.integrate(i, poses[i])
        for mw in (0, 2):
            for pose in (poses[2], offset_pose(poses[2], 0.5, VOXEL)):
                a = sp.track_evaluate(2, pose, stride=1, max_dist=3 * VOXEL, min_weight=mw)
                b = ctx.track_evaluate(2, pose, stride=1, max_dist=3 * VOXEL, min_weight=mw)
                assert b["n_corr"] > 500
                for k in ("A", "b", "e", "n_corr", "n_src"):
                    assert np.array_equal(a[k], b[k]), k


def test_repeatable_and_flushes_pending_integrations():
    poses, frames = small_scene_frames(n=4, deg=4.0)
    ctx, _ = make_pair(dims=DIMS, voxel=VOXEL, centre=CENTRE, n_slots=4, channels=tl3d.CH_TSDF)
    with ctx:
        for i, (d, col) in enumerate(frames):
            ctx.upload(i, d, col)
            ctx.integrate(i, poses[i])
        pose = offset_pose(poses[1], 0.5, VOXEL)
        early = ctx.track_evaluate(1, pose, stride=2, max_dist=0.05)        # straight after integrate: the deferred batch is issued first
        ctx.sync()
        late = ctx.track_evaluate(1, pose, stride=2, max_dist=0.05)
        again = ctx.track_evaluate(1, pose, stride=2, max_dist=0.05)
        assert late["n_corr"] > 500
        for k in ("A", "b", "e", "n_corr", "n_src"):
            assert np.array_equal(early[k], late[k]) and np.array_equal(late[k], again[k]), k
        r1, r2 = ctx.track(1, pose, LEVELS), ctx.track(1, pose, LEVELS)
        assert np.array_equal(r1["T"], r2["T"]) and r1["rmse"] == r2["rmse"] and r1["iters_run"] == r2["iters_run"]


def test_track_recovers_a_frame_that_is_not_in_the_model():
    """The CPU test's shape (tests/test_track_reference_cpu.py: why 10 mm voxels), on the device: within the bars of the analytic
    pose, within the project's ICP parity bar of the reference."""
    scene = synth.object_scene()
    poses = synth.orbit_poses(6, 1.0, 8.0)
    ctx, _ = make_pair(dims=FINE_DIMS, voxel=FINE_VOXEL, centre=FINE_CENTRE, n_slots=7, channels=tl3d.CH_TSDF)
    with ctx:
        for i, p in enumerate(poses):
            d, _ = synth.render(scene, p, SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], seed=i)
            ctx.upload(i, d, None)
            ctx.integrate(i, p)
        truth = novel_pose()
        depth, _ = synth.render(scene, truth, SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], seed=50)
        ctx.upload(6, depth, None)
        start = offset_pose(truth, 0.5, 0.010)
        res = ctx.track(6, start, LEVELS)
        dims, origin, voxel, trunc = _spec_of(ctx)
        ref = tr.track(ctx.download_grid(tl3d.CH_TSDF), dims, origin, voxel, trunc, SMALL, depth, start, LEVELS, min_depth=ctx.min_depth,
                       max_depth=ctx.max_depth)
    d1 = pose_delta(res["T"], tr.pose_matrix(truth), voxel)
    diff = float(np.linalg.norm(res["T"] - ref["T"]))
    print(f"recovered to {d1[0]:.4f} voxel / {d1[1]:.4f} deg; fitness {res['fitness']:.3f}, rmse {res['rmse'] * 1e3:.3f} mm, {res['iters_run']} "
          f"iterations, status {res['status']}; |T - T_reference| = {diff:.2e} (reference: {ref['iters_run']} iterations, status {ref['status']})")
    assert d1[0] < 0.1 and d1[1] < 0.1
    assert diff < 1e-4
    assert res["status"] in (0, 1) and 1 <= res["iters_run"] <= LEVELS[-1]["iters"]
    assert res["n_corr"] == ref["n_corr"] or abs(res["n_corr"] - ref["n_corr"]) < 0.01 * ref["n_corr"]
    assert np.array_equal(res["pose"][0], res["T"][:3, :3]) and np.array_equal(res["pose"][1], res["T"][:3, 3]) and res["scale"] == 1.0


def test_too_few_correspondences_is_status_2_at_the_initial_pose():
    ctx, _ = make_pair(dims=CRAFTED_DIMS, voxel=CRAFTED_VOXEL, centre=CRAFTED_CENTRE, channels=tl3d.CH_TSDF, n_slots=1)
    with ctx:
        rec = crafted_records()
        ctx.upload_grid(tl3d.CH_TSDF, rec)
        ctx.upload(0, np.full((SMALL["height"], SMALL["width"]), 0.25, np.float32), None)
        # a camera facing the unobserved slab (voxels 10..12 along z) whose flat frame lies in it, on the plane of voxel centres 11:
        # every cell there has corners nobody saw (and what falls beside the grid has no cell)
        origin = _spec_of(ctx)[1]
        eye = np.array([origin[0] + 0.4, origin[1] + 0.24, origin[2] + 11.5 * CRAFTED_VOXEL - 0.25])
        start = (np.eye(3), -eye)
        ev = ctx.track_evaluate(0, start, stride=1, max_dist=0.05)
        assert ev["n_src"] == SMALL["width"] * SMALL["height"] and ev["n_corr"] == 0
        res = ctx.track(0, start, LEVELS)
        assert res["status"] == 2 and res["iters_run"] == 0
        assert np.array_equal(res["T"], tr.pose_matrix(start))
        # the counts are those of the final pass of the level that failed, the first one
        ev0 = ctx.track_evaluate(0, start, stride=LEVELS[0]["stride"], max_dist=LEVELS[0]["max_dist"])
        assert res["n_corr"] == ev0["n_corr"] == 0 and res["n_src"] == ev0["n_src"] > 1000 and res["fitness"] == 0.0 and res["rmse"] == 0.0


def test_errors():
    import ctypes as C
    lib = abi.load()
    eye, zero = abi.d9(np.eye(3)), abi.d3(np.zeros(3))
    ev, res = abi.IcpEval(), abi.IcpResult()
    lv = (abi.IcpParams * 5)(*[abi.IcpParams(2, 2, 0.05, 1e-6, 1e-7, 1e-4, 0, 0) for _ in range(5)])

    def evaluate(c, slot=0, R=eye, t=zero, stride=2, gate=0.05):
        return lib.tl3d_track_evaluate(c._h, slot, 1.0, abi.ptr(R), abi.ptr(t), 1, stride, gate, C.byref(ev))

    def frame(c, slot=0, R=eye, t=zero, levels=lv, n=2):
        return lib.tl3d_track_frame(c._h, slot, 1.0, abi.ptr(R), abi.ptr(t), 1, levels, n, C.byref(res))
    depth = np.full((SMALL["height"], SMALL["width"]), 0.5, np.float32)
    cen_only, _ = make_pair(dims=(16, 16, 16), channels=tl3d.CH_CENTROID)
    with cen_only:
        cen_only.upload(0, depth, None)
        assert evaluate(cen_only) == abi.E_STATE and frame(cen_only) == abi.E_STATE          # no TSDF channel
        with pytest.raises(abi.Tl3dError) as e:
            cen_only.track_evaluate(0, (np.eye(3), np.zeros(3)))
        assert e.value.code == abi.E_STATE and "TSDF" in str(e.value)
    ctx, _ = make_pair(dims=(16, 16, 16), n_slots=3, channels=tl3d.CH_TSDF)
    with ctx:
        ctx.upload(0, depth, None)
        ctx.upload(1, depth, None)
        assert evaluate(ctx) == abi.OK and frame(ctx) == abi.OK
        assert evaluate(ctx, slot=2) == abi.E_STATE and frame(ctx, slot=2) == abi.E_STATE    # an empty slot
        for bad in (3, -1):
            assert evaluate(ctx, slot=bad) == abi.E_INVALID and frame(ctx, slot=bad) == abi.E_INVALID
        assert evaluate(ctx, stride=0) == abi.E_INVALID and evaluate(ctx, gate=0.0) == abi.E_INVALID and evaluate(ctx, gate=-1.0) == abi.E_INVALID
        assert evaluate(ctx, R=None) == abi.E_INVALID and evaluate(ctx, t=None) == abi.E_INVALID
        assert frame(ctx, R=None) == abi.E_INVALID and frame(ctx, t=None) == abi.E_INVALID
        assert frame(ctx, n=0) == abi.E_INVALID and frame(ctx, n=abi.ICP_MAX_LEVELS + 1) == abi.E_INVALID
        assert frame(ctx, n=abi.ICP_MAX_LEVELS) == abi.OK
        for field, value in (("stride", 0), ("max_dist", 0.0), ("estimate_scale", 1)):
            one = (abi.IcpParams * 1)(abi.IcpParams(2, 2, 0.05, 1e-6, 1e-7, 1e-4, 0, 0))
            setattr(one[0], field, value)
            assert frame(ctx, levels=one, n=1) == abi.E_INVALID, field
        # an uncollected ICP batch
        ctx.build_normals(0)
        ctx.build_normals(1)
        ctx.icp_batch_enqueue([(0, 1)], [dict(iters=2, stride=2, max_dist=0.1)])
        assert evaluate(ctx) == abi.E_STATE and frame(ctx) == abi.E_STATE
        ctx.icp_batch_collect()
        assert evaluate(ctx) == abi.OK
        # a block: a core set
        ctx.set_block_core((32, 16, 16), (0, 0, 0), (8, 16, 16))
        assert evaluate(ctx) == abi.E_STATE and frame(ctx) == abi.E_STATE
    origin = (-0.16, -0.16, -0.16)
    off = tl3d.FusionContext(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], n_slots=1,
                             grid=tl3d.GridSpec((16, 16, 16), origin, 0.02, 0.08, tl3d.CH_TSDF, voxel_offset=(8, 0, 0)))
    with off:
        off.upload(0, depth, None)
        assert evaluate(off) == abi.E_STATE and frame(off) == abi.E_STATE                    # a block: a voxel offset


# ---- pipeline and command line --------------------------------------------------------------------------------------
def _arc_pipeline(frames, **kw):
    cfg = ReconstructionConfig(fx=SMALL["fx"], fy=SMALL["fy"], cx=SMALL["cx"], cy=SMALL["cy"], voxel_size=ARC["voxel"], subsample_factor=2,
                               grid_dim=256, **kw)
    pipe = DepthToReconstructionPipeline(cfg)
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    pts, col, poses = pipe.reconstruct()
    return pipe, pts, poses


def test_pipeline_tracks_the_arc(capsys):
    """the arc fixed by the CPU test (track_common.ARC), through reconstruct()"""
    truth_poses, frames = arc_frames()
    truth = np.stack([tr.pose_matrix(p) for p in truth_poses])
    capsys.readouterr()
    on, pts_on, poses_on = _arc_pipeline(frames, model_tracking=True)
    out_on = capsys.readouterr().out
    off, pts_off, poses_off = _arc_pipeline(frames)
    out_off = capsys.readouterr().out
    assert len(poses_on) == len(poses_off) == ARC["n"]
    # the chain is what it is without the option, bit for bit; the tracked poses replace camera_poses
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(on.chain_poses, poses_off))
    assert poses_on is on.camera_poses and all(np.shape(a[1]) == np.shape(b[1]) for a, b in zip(poses_on, poses_off))
    mt = on.stats["model_tracking"]
    print(mt, on.timings)
    assert set(mt) == {"frames", "tracked", "lost", "mean_fitness", "mean_rmse_mm", "max_correction_mm", "max_correction_deg", "voxel_size"}
    assert mt["frames"] == ARC["n"] and mt["lost"] == 0 and mt["tracked"] == ARC["n"] - 1 and mt["voxel_size"] == ARC["voxel"]
    assert "track_s" in on.timings and "track_s" not in off.timings and "model_tracking" not in off.stats
    e_chain = centre_errors_mm(np.stack([tr.pose_matrix(p) for p in on.chain_poses]), truth)
    e_track = centre_errors_mm(np.stack([tr.pose_matrix(p) for p in poses_on]), truth)
    print(f"mean camera-centre error: chain {e_chain.mean():.4f} mm, tracked {e_track.mean():.4f} mm")
    assert e_track.mean() < e_chain.mean()
    assert len(pts_on) > 1000 and len(pts_off) > 1000
    extra = [l for l in out_on.splitlines() if l not in out_off.splitlines() and l.strip()]
    assert len([l for l in extra if "Step 1c" in l]) == 1 and len([l for l in extra if l.startswith("  Model tracking:")]) == 1, extra
    # with poses given nothing is registered and the option is ignored
    pipe = DepthToReconstructionPipeline(ReconstructionConfig(fx=SMALL["fx"], fy=SMALL["fy"], cx=SMALL["cx"], cy=SMALL["cy"], voxel_size=ARC["voxel"],
                                                              subsample_factor=2, grid_dim=256, model_tracking=True))
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    p2, _, e2 = pipe.reconstruct(poses=poses_off)
    assert np.array_equal(p2, pts_off) and "model_tracking" not in pipe.stats


def test_refusals_and_cli(tmp_path, capsys):
    from PIL import Image
    _, frames = small_scene_frames(n=5, deg=2.0)
    rgb_dir, depth_dir = tmp_path / "rgb", tmp_path / "depth"
    rgb_dir.mkdir()
    depth_dir.mkdir()
    for i, (d, c) in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(c[..., ::-1])).save(rgb_dir / f"frame_{i:04d}.png")
        np.save(depth_dir / f"frame_{i:04d}_depth.npy", d)
    intr = ["--fx", str(SMALL["fx"]), "--fy", str(SMALL["fy"]), "--cx", str(SMALL["cx"]), "--cy", str(SMALL["cy"])]
    import depth_to_reconstruction as d2r
    out = tmp_path / "tracked.ply"
    capsys.readouterr()
    assert d2r.main(["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--output", str(out), *intr, "--no-vis", "--grid", "256",
                     "--voxel-size", "0.025", "--model-tracking"]) == 0
    assert out.exists() and os.path.getsize(out) > 1000 and "  Model tracking:" in capsys.readouterr().out
    # refused before any work, with a message: several GPUs, and together with --estimate-scale
    for extra in (["--gpus", "2"], ["--estimate-scale"]):
        with pytest.raises(SystemExit) as ei:
            d2r.main(["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--output", str(tmp_path / "no.ply"), *intr, "--no-vis",
                      "--model-tracking", *extra])
        assert ei.value.code == 2 and "--model-tracking" in capsys.readouterr().err
    assert not (tmp_path / "no.ply").exists()
    # the library refuses the same combinations
    pipe = DepthToReconstructionPipeline(ReconstructionConfig(fx=SMALL["fx"], fy=SMALL["fy"], cx=SMALL["cx"], cy=SMALL["cy"], model_tracking=True))
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    with pytest.raises(ValueError, match="estimate_scale"):
        pipe.reconstruct(estimate_scale=True)
    with pytest.raises(ValueError, match="single GPU"):
        pipe.reconstruct_sharded(None)
