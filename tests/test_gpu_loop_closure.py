"""GPU: loop closure through reconstruct() (config.loop_closure) -- the closed orbit of tests/test_posegraph_cpu.py with the
device as the source of the edges --, the cases where it must change nothing, pruning of a wrong closure, the command lines."""
import functools
import os

import numpy as np
import pytest

import tl3d
from tl3d import fileio, synth
from tl3d import posegraph as pg
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

from loop_closure_common import GATE, LEVELS, ORBIT_CAM, STRIDE, check_loop_criteria, orbit_frames

pytestmark = pytest.mark.gpu

N_LOOP, SIGMA = 72, 0.002
BIG_CAM = dict(width=1080, height=1920, fx=1719.0, fy=1719.0, cx=540.0, cy=960.0)        # the project's default camera


@functools.lru_cache(maxsize=2)
def _orbit(big):
    if not big:
        return orbit_frames(N_LOOP, SIGMA)
    import torch
    frames, truth = orbit_frames(N_LOOP, SIGMA, cam=BIG_CAM, xp=torch, device="cuda")
    return [(d.cpu().numpy(), c.cpu().numpy()) for d, c in frames], truth


def _config(cam, **kw):
    return ReconstructionConfig(fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], voxel_size=0.01, subsample_factor=2, grid_dim=512,
                                loop_min_gap=N_LOOP // 2, **kw)


def _run(cam, frames, **kw):
    pipe = DepthToReconstructionPipeline(_config(cam, **kw))
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    pts, col, poses = pipe.reconstruct()
    return pipe, pts, col, poses


def _levels():
    return [dict(iters=it, stride=st, max_dist=g, damping=1e-6, eps=1e-7, eig_rel=1e-4) for it, st, g in LEVELS]


def _direct_pair(cam, frames):
    """frame 0 registered against frame N by the existing batched registration, from identity"""
    with tl3d.FusionContext(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], n_slots=2, grid=None) as ctx:
        ctx.set_normal_smoothing(1)
        for k, f in enumerate((frames[0], frames[-1])):
            ctx.upload(k, f[0], None)
            ctx.build_normals(k)
        res = ctx.icp_batch([(0, 1)], _levels())[0]
    assert res["status"] != 2
    return res["T"]


@pytest.mark.parametrize("big", [False, True], ids=["320x240", "1080x1920"])
def test_closed_orbit_through_reconstruct(big):
    cam = BIG_CAM if big else ORBIT_CAM
    frames, truth = _orbit(big)
    on, pts, _, poses = _run(cam, frames, loop_closure=True)
    off, pts_off, _, poses_off = _run(cam, frames)
    assert len(poses) == N_LOOP + 1 and len(poses_off) == N_LOOP + 1
    lc = on.stats["loop_closure"]
    print(lc, on.timings)
    assert lc["accepted"] > 0 and lc["candidates"] >= lc["scored"] >= lc["registered"] >= lc["accepted"] and lc["iterations"] > 0
    assert lc["cost_after"] < lc["cost_before"]
    assert "loop_closure_s" in on.timings and "loop_closure_s" not in off.timings and "loop_closure" not in off.stats
    # the chain is what it is without the option, bit for bit; the optimised poses replace camera_poses
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(on.chain_poses, poses_off))
    assert poses is on.camera_poses and not np.array_equal(pg.poses_to_matrices(poses), pg.poses_to_matrices(on.chain_poses))
    assert np.array_equal(poses[0][0], np.eye(3)) and not np.any(poses[0][1])
    check_loop_criteria(pg.poses_to_matrices(on.chain_poses), pg.poses_to_matrices(poses), _direct_pair(cam, frames), truth)
    assert len(pts) > 1000 and len(pts_off) > 1000


def test_corridor_dolly_is_untouched(capsys):
    scene = synth.corridor_scene()
    cam = ORBIT_CAM
    poses = synth.dolly_poses(40, (0.0, 0.0, 0.0), (0.0, 0.0, 0.1))
    frames = [synth.render(scene, p, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], noise_sigma=0.001, seed=i)
              for i, p in enumerate(poses)]

    def run(**kw):
        cfg = ReconstructionConfig(fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], voxel_size=0.02, subsample_factor=2, grid_dim=512, **kw)
        pipe = DepthToReconstructionPipeline(cfg)
        pipe.set_frames([c for d, c in frames], [d for d, c in frames])
        return (pipe,) + tuple(pipe.reconstruct())
    capsys.readouterr()
    on, p1, c1, e1 = run(loop_closure=True)
    out_on = capsys.readouterr().out
    off, p0, c0, e0 = run()
    out_off = capsys.readouterr().out
    assert len(e1) == len(e0) == 40
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(e1, e0))
    assert np.array_equal(p1, p0) and np.array_equal(c1, c0)
    assert on.stats["loop_closure"]["candidates"] == 0 and on.stats["loop_closure"]["accepted"] == 0
    extra = [l for l in out_on.splitlines() if l not in out_off.splitlines()]
    assert len(extra) == 1 and extra[0].startswith("Loop closure:"), extra           # one line says so
    # with poses given nothing is registered and the option is ignored
    pipe = DepthToReconstructionPipeline(ReconstructionConfig(fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], voxel_size=0.02,
                                                              grid_dim=512, loop_closure=True))
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    p2, c2, e2 = pipe.reconstruct(poses=e0)
    assert np.array_equal(p2, p0) and "loop_closure" not in pipe.stats


def test_planted_wrong_loop_edge_is_pruned():
    """Graph-level API on device edges: the orbit's chain and its loop candidates registered on the GPU, the weights from
    icp_evaluate, plus one closure of (0, N) that is 10 cm off: optimise_and_prune drops exactly that one, and the result is the
    optimum of the graph without it."""
    cam = ORBIT_CAM
    frames, truth = _orbit(False)
    n = len(frames)
    with tl3d.FusionContext(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], n_slots=n, grid=None) as ctx:
        ctx.set_normal_smoothing(1)
        for k, (d, c) in enumerate(frames):
            ctx.upload(k, d, None)
        ctx.build_normals_many(list(range(n)))
        chain_pairs = [(k, k + 1) for k in range(n - 1)]
        reg = ctx.icp_batch(chain_pairs, _levels())
        chain = [np.eye(4)]
        for r in reg:
            assert r["status"] != 2
            chain.append(r["T"] @ chain[-1])
        chain = np.stack(chain)
        ev = ctx.icp_evaluate(chain_pairs, [r["T"] for r in reg], STRIDE, GATE)
        edges = [(i, j, r["T"], e["A"]) for (i, j), r, e in zip(chain_pairs, reg, ev)]
        cands = pg.loop_candidates(chain, n // 2, 0.3, 20.0)
        assert (0, n - 1) in cands and len(cands) >= 4
        lreg = ctx.icp_batch(cands, _levels(), T_init=[pg.relative_pose(chain[i], chain[j]) for i, j in cands])
        lev = ctx.icp_evaluate(cands, [r["T"] for r in lreg], STRIDE, GATE)
        loops = [(i, j, r["T"], e["A"]) for (i, j), r, e in zip(cands, lreg, lev) if r["status"] != 2 and e["fitness"] >= 0.5]
        assert len(loops) >= 4
        k0 = cands.index((0, n - 1))
        wrong = np.array(lreg[k0]["T"])
        wrong[:3, 3] += np.array([0.1, 0.0, 0.0])
        graph = edges + loops + [(0, n - 1, wrong, lev[k0]["A"])]
        is_loop = [False] * len(edges) + [True] * (len(loops) + 1)
        out, info = pg.optimise_and_prune(chain, graph, is_loop, 0.05, device="cuda")
        print(info["pruned"], sorted(info["residual_m"])[-3:])
        assert info["pruned"] == [len(graph) - 1]
        clean, _ = pg.optimise(chain, edges + loops, device="cuda")
        assert np.abs(out - clean).max() < 1e-9


def _write_sequence(tmp_path, frames):
    from PIL import Image
    rgb_dir, depth_dir = tmp_path / "rgb", tmp_path / "depth"
    rgb_dir.mkdir()
    depth_dir.mkdir()
    for i, (d, c) in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(c[..., ::-1])).save(rgb_dir / f"frame_{i:04d}.png")
        fileio.save_depth_like_processor(d, depth_dir, f"frame_{i:04d}")
        os.remove(depth_dir / f"frame_{i:04d}_depth.npy")               # leave only the 16-bit millimetre PNG
    return rgb_dir, depth_dir


def test_cli_flag_on_both_drivers_and_refusals(tmp_path, capsys):
    cam = ORBIT_CAM
    scene = synth.object_scene(True)
    poses = synth.orbit_poses(6, 1.0, 2.0)
    frames = [synth.render(scene, p, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]) for p in poses]
    rgb_dir, depth_dir = _write_sequence(tmp_path, frames)
    intr = ["--fx", "300", "--fy", "300", "--cx", "160", "--cy", "120"]
    import depth_to_reconstruction as d2r
    out = tmp_path / "d2r.ply"
    capsys.readouterr()
    assert d2r.main(["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--output", str(out), *intr, "--no-vis", "--grid", "512",
                     "--voxel-size", "0.02", "--loop-closure"]) == 0
    assert out.exists() and "Loop closure:" in capsys.readouterr().out
    # refused before any work: several GPUs, and together with --estimate-scale
    for extra in (["--gpus", "2"], ["--estimate-scale"]):
        with pytest.raises(SystemExit) as ei:
            d2r.main(["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--output", str(tmp_path / "no.ply"), *intr, "--no-vis",
                      "--loop-closure", *extra])
        assert ei.value.code == 2 and "--loop-closure" in capsys.readouterr().err
    assert not (tmp_path / "no.ply").exists()
    import depth_enhanced_reconstruction as der
    for i, (d, c) in enumerate(frames):
        np.save(rgb_dir / f"frame_{i:04d}_depth.npy", d)
    out_dir = tmp_path / "der"
    assert der.main(["--input", str(rgb_dir), "--output", str(out_dir), *intr, "--grid", "512", "--loop-closure"]) == 0
    assert (out_dir / "reconstruction.ply").exists() and "Loop closure:" in capsys.readouterr().out
    # the library refuses the same combinations
    pipe = DepthToReconstructionPipeline(ReconstructionConfig(fx=300.0, fy=300.0, cx=160.0, cy=120.0, loop_closure=True))
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    with pytest.raises(ValueError, match="estimate_scale"):
        pipe.reconstruct(estimate_scale=True)
    with pytest.raises(ValueError, match="single GPU"):
        pipe.reconstruct_sharded(None)
