#!/usr/bin/env python3
"""Joint point-to-plane + photometric registration (rgbd_register) beside the batched ICP (icp_batch) on the same pairs: 1080x1920
frames of the headline orbit resident in HBM, 64 pairs (k-1, k), the pipeline's default levels.  The two calls are timed
ALTERNATELY inside one process (rgbd, icp, rgbd, icp, ...) after a warm-up of each, with the device synchronised around every
timed call; the median of each is reported as time per pair-iteration, with their ratio.  Rows:
  every iteration   eps = 0: all 10 + 15 iterations and the two final passes run, 27 passes per pair -- comparable per pass
  pipeline          eps = 1e-7 (config.icp_eps): levels stop when converged; per pair, with the mean iterations of the last level
The ratio is reported, not gated: icp_batch is one persistent launch with no launch boundary per iteration, rgbd_register pays two
launches per batch-iteration.  Algorithmic bytes per sample come from the shapes.

    python tools/bench_rgbd.py [--pairs 64] [--reps 7] [--out profiles/rgbd_register.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import tl3d  # noqa: E402
from tl3d import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=64)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--radius", type=int, default=1, help="normal smoothing (the pipeline's default: 1)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
W, H = 1080, 1920
cam = dict(fx=1719.0, fy=1719.0, cx=540.0, cy=960.0)
N = args.pairs + 1
scene = synth.object_scene(True)
poses = synth.orbit_poses(512, 1.0, 0.7)[:N]
dev = torch.device("cuda", 0)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


ctx = tl3d.FusionContext(W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"], n_slots=N, grid=None)
for i, p in enumerate(poses):
    d, c = synth.render(scene, p, W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"], xp=torch, device=dev)
    d, c = d.contiguous(), c.contiguous()
    torch.cuda.synchronize()
    ctx.upload(i, d, c)
    ctx.sync()
ctx.set_normal_smoothing(args.radius)
ctx.build_normals_many(list(range(N)))
ctx.sync()
t0 = time.perf_counter()
ctx.build_intensity(list(range(N)))
ctx.sync()
t_maps = time.perf_counter() - t0
pairs = [(k - 1, k) for k in range(1, N)]
base = [dict(iters=10, stride=4, max_dist=0.2), dict(iters=15, stride=2, max_dist=0.05)]
# algorithmic bytes per sample, from the shapes: what a pass must read of each sampled pixel
f32 = np.dtype(np.float32).itemsize
bytes_icp = f32 + 4 * f32                                   # source depth, target normal record (nx, ny, nz, d)
bytes_rgbd = bytes_icp + 4 * f32 + 4 * f32                  # + source map record, target map record (S, Sx, Sy, flag)
samples = [((W + lv["stride"] - 1) // lv["stride"]) * ((H + lv["stride"] - 1) // lv["stride"]) for lv in base]
say(f"joint registration against the batched ICP: {len(pairs)} pairs of {W}x{H} frames, normal smoothing {args.radius}, levels "
    f"{[(lv['iters'], lv['stride'], lv['max_dist']) for lv in base]}, photo_weight 0.1, photo_gate 0.2")
say(f"intensity maps: {1e3 * t_maps / N:.3f} ms per frame ({N} frames, radius 1)")
say(f"samples per pass: {samples}; algorithmic bytes per sample: icp {bytes_icp} B (source depth {f32}, target normal record {4 * f32}), "
    f"rgbd {bytes_rgbd} B (+ source map {4 * f32}, target map {4 * f32})")
for name, eps in (("every iteration", 0.0), ("pipeline", 1e-7)):
    levels = [dict(lv, eps=eps, photo_weight=0.1, photo_gate=0.2) for lv in base]
    calls = dict(rgbd=lambda: ctx.rgbd_register(pairs, levels), icp=lambda: ctx.icp_batch(pairs, levels))
    res, ts = {}, dict(rgbd=[], icp=[])
    for k, f in calls.items():                              # warm-up: buffers, code objects
        res[k] = f()
        ctx.sync()
    for _ in range(args.reps):
        for k, f in calls.items():                          # alternately
            ctx.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = f()
            ctx.sync()
            ts[k].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
    passes = sum(lv["iters"] + 1 for lv in base)
    dT = max(float(np.linalg.norm(a["T"] - b["T"])) for a, b in zip(res["rgbd"], res["icp"]))
    say(f"{name} (eps {eps:g}):")
    for k in ("rgbd", "icp"):
        row = f"  {k:5s} {1e3 * med[k]:9.3f} ms per call (min {1e3 * min(ts[k]):.3f}, max {1e3 * max(ts[k]):.3f}), {1e6 * med[k] / len(pairs):9.2f} us per pair"
        if eps == 0.0:
            row += f", {1e6 * med[k] / len(pairs) / passes:7.3f} us per pair-iteration ({passes} passes)"
            total = sum(s * (lv["iters"] + 1) for s, lv in zip(samples, base)) * len(pairs)
            row += f", {total * (bytes_rgbd if k == 'rgbd' else bytes_icp) / med[k] / 1e9:7.1f} GB/s algorithmic"
        else:
            row += f", mean iterations of the last level {np.mean([r['iters_run'] for r in res[k]]):.2f}"
        say(row)
    say(f"  ratio rgbd / icp {med['rgbd'] / med['icp']:.2f}; largest |T_rgbd - T_icp|_F {dT:.2e}; mean n_photo {np.mean([r['n_photo'] for r in res['rgbd']]):.0f}, "
        f"mean photometric rmse {np.mean([r['photo_rmse'] for r in res['rgbd']]):.4f}")
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
