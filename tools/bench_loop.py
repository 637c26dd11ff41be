#!/usr/bin/env python3
"""Loop closure, measured.

    python tools/bench_loop.py eval [--pairs 1024] [--reps 9]
        FusionContext.icp_evaluate on `pairs` pairs of 1080x1920 frames of the headline orbit (resident in HBM) at stride 2 and
        stride 4, beside the batched registration of the same pairs with one level of ONE iteration (two passes over the same
        samples), interleaved, medians; bytes per sample (20 B) as a fraction of 8 TB/s.
    python tools/bench_loop.py config4 [--frames 1000] [--reps 2]
        BASELINE config 4 (tools/run_config.py: 1280x720 orbit of the cylinder + ground, 0.36 degrees per frame, closed after 1000
        frames) through reconstruct() with config.loop_closure off and on, interleaved: stage times, the loop-closure counts, and
        the closure error (last frame against the analytic pose) and mean camera-centre error of the chain and of the optimised poses.
One JSON object on stdout.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import tl3d  # noqa: E402
from tl3d import posegraph as pg  # noqa: E402
from tl3d import synth  # noqa: E402
from tl3d.config import ReconstructionConfig  # noqa: E402
from tl3d.pipeline import DepthToReconstructionPipeline  # noqa: E402

HBM_BYTES_PER_S = 8e12


def median(xs):
    return sorted(xs)[len(xs) // 2]


def bench_eval(args):
    W, H = 1080, 1920
    cam = dict(fx=1719.0, fy=1719.0, cx=540.0, cy=960.0)
    per = 4                                               # pairs (k, k + 1 .. k + per) of every frame k
    n = (args.pairs + per - 1) // per + per
    scene = synth.object_scene(True)
    poses = synth.orbit_poses(512, 1.0, 0.7)[:n]
    dev = torch.device("cuda", 0)
    ctx = tl3d.FusionContext(W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"], n_slots=n, grid=None)
    ctx.set_normal_smoothing(1)
    for i, p in enumerate(poses):
        d, _ = synth.render(scene, p, W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"], xp=torch, device=dev, noise_sigma=0.001, seed=i,
                            want_color=False)
        d = d.contiguous()
        torch.cuda.synchronize()
        ctx.upload(i, d, None)
        ctx.sync()
    ctx.build_normals_many(list(range(n)))
    ctx.sync()
    pairs = [(k, k + s) for k in range(n - per) for s in range(1, per + 1)][:args.pairs]
    Ts = []
    for a, b in pairs:
        r, t = synth.relative_pose(poses[a], poses[b])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = r, np.asarray(t).ravel()
        Ts.append(T)
    out = dict(mode="eval", pairs=len(pairs), frames=n, width=W, height=H, reps=args.reps)
    for stride in (2, 4):
        level = [dict(iters=1, stride=stride, max_dist=0.05, eps=0.0)]
        first = ctx.icp_evaluate(pairs, Ts, stride, 0.05)                # warm-up of both, and the reference bits
        ctx.icp_batch(pairs, level, T_init=Ts)
        te, tb, differing = [], [], 0
        for _ in range(args.reps):                                       # interleaved
            t0 = time.perf_counter()
            ev = ctx.icp_evaluate(pairs, Ts, stride, 0.05)
            te.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ctx.icp_batch(pairs, level, T_init=Ts)
            tb.append(time.perf_counter() - t0)
            differing += int(any(not np.array_equal(a["A"], b["A"]) or a["n_corr"] != b["n_corr"] for a, b in zip(ev, first)))
        samples = ((W + stride - 1) // stride) * ((H + stride - 1) // stride)
        e, b = median(te), median(tb)
        out[f"stride {stride}"] = dict(
            evaluate_ms=round(1e3 * e, 3), evaluate_ms_min_max=[round(1e3 * min(te), 3), round(1e3 * max(te), 3)],
            evaluate_us_per_pair=round(1e6 * e / len(pairs), 3),
            batch_one_iteration_ms=round(1e3 * b, 3), batch_ms_min_max=[round(1e3 * min(tb), 3), round(1e3 * max(tb), 3)],
            evaluate_over_batch=round(e / b, 3), samples_per_pair=samples, bytes_per_sample=20,
            evaluate_GB_per_s=round(20.0 * samples * len(pairs) / e / 1e9, 1),
            fraction_of_8_TB_per_s=round(20.0 * samples * len(pairs) / e / HBM_BYTES_PER_S, 4),
            fitness_mean=round(float(np.mean([r["fitness"] for r in first])), 4), calls_differing_from_the_first=differing)
        print(f"stride {stride}: {out[f'stride {stride}']}", flush=True)
    ctx.close()
    return out


def trajectory_errors(poses, index, truth):
    T = pg.poses_to_matrices(poses)
    centre = lambda M: -M[:3, :3].T @ M[:3, 3]
    err = [float(np.linalg.norm(centre(T[k]) - centre(truth[fi]))) * 1e3 for k, fi in enumerate(index)]
    R, Rt = T[-1][:3, :3], truth[index[-1]][:3, :3]
    ang = float(np.degrees(np.arccos(np.clip(0.5 * (np.trace(R @ Rt.T) - 1.0), -1.0, 1.0))))
    return dict(closure_mm=round(err[-1], 3), closure_deg=round(ang, 4), mean_centre_mm=round(float(np.mean(err)), 3), max_centre_mm=round(max(err), 3))


def bench_config4(args):
    W, H, n = 1280, 720, args.frames
    dev = torch.device("cuda", 0)
    scene = synth.cylinder_scene(ground=True)
    poses = synth.orbit_poses(n, 1.5, 0.36, height=-0.2)
    truth = pg.poses_to_matrices(poses)
    truth = truth @ np.linalg.inv(truth[0])
    kw = dict(fx=1000.0, fy=1000.0, cx=640.0, cy=360.0, voxel_size=0.01, subsample_factor=4, max_depth=4.0)
    gen = torch.Generator(device=dev).manual_seed(7)
    images, depths = [], []
    for p in poses:
        d, c = synth.render(scene, p, W, H, kw["fx"], kw["fy"], kw["cx"], kw["cy"], xp=torch, device=dev)
        if args.depth_noise_mm > 0:
            d = torch.where(d > 0, d + 1e-3 * args.depth_noise_mm * torch.randn(d.shape, device=dev, generator=gen, dtype=d.dtype), d)
        depths.append(d.contiguous())
        images.append(c.contiguous())
    torch.cuda.synchronize()
    out = dict(mode="config4", frames=n, width=W, height=H, depth_noise_mm=args.depth_noise_mm, runs=[])
    log = io.StringIO()
    for rep in range(args.reps + 1):                                    # the first pair of runs warms the process up
        for on in (False, True):
            pipe = DepthToReconstructionPipeline(ReconstructionConfig(**kw, loop_closure=on))
            pipe.set_frames(images, depths)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(log):
                pts, _, est = pipe.reconstruct()
            dt = time.perf_counter() - t0
            row = dict(rep=rep, loop_closure=on, reconstruct_s=round(dt, 3), stage_s=pipe.timings, cameras=len(est), points=int(len(pts)),
                       chain=trajectory_errors(pipe.chain_poses, pipe.frame_index, truth))
            if on:
                row["loop"] = pipe.stats["loop_closure"]
                row["optimised"] = trajectory_errors(est, pipe.frame_index, truth)
            out["runs"].append(row)
            print(row, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["eval", "config4"])
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--depth-noise-mm", type=float, default=0.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.reps <= 0:
        args.reps = 9 if args.mode == "eval" else 2
    out = bench_eval(args) if args.mode == "eval" else bench_config4(args)
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
