"""Point-to-SDF tracking against the fused TSDF: what it costs and what it gives.

(a) per-iteration time of tl3d_track_frame on one 1080x1920 frame of the headline orbit against the 512^3 grid at 5 mm, strides 2
    and 4, beside tl3d_icp_p2plane on the same frame and stride in the same process: a run of N iterations (eps = 0: none stops
    early) minus a run of none, over N; device events around the blocking call for the tracker (it runs on the context's stream),
    the host clock around the blocking call for both; median of 20 after 2 warm-ups;
(b) per-frame cost of the pipeline stage -- FusionContext.track through the chain's levels, and the one-frame integration -- beside
    the route it replaces on the same frames: raycast(slot) + build_normals + icp through the same levels;
(c) camera-centre errors of the chain, the tracked poses and loop closure + tracking, through reconstruct(), on the open arc of
    tests/track_common.py and on the closed 72-frame orbit of section 11, at several tracking voxel sizes.

    python tools/bench_track.py [--frames 48] [--skip a,b,c]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def part_ab(args, out):
    import numpy as np
    import torch
    import tl3d
    from tl3d import synth

    hl = synth.HEADLINE
    W, H = hl["width"], hl["height"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    scene = synth.object_scene(with_room=True)
    n = args.frames
    poses = synth.orbit_poses(n + 4, hl["radius"], 360.0 / 512)
    spec = tl3d.GridSpec.cube(hl["grid"], hl["voxel"], centre=(0.0, -0.1, 0.0), channels=tl3d.CH_TSDF)
    common = dict(damping=1e-6, eig_rel=1e-4)
    chain = [dict(iters=10, stride=4, max_dist=0.20, eps=1e-7, **common), dict(iters=15, stride=2, max_dist=0.05, eps=1e-7, **common)]
    with tl3d.FusionContext(W, H, hl["fx"], hl["fy"], hl["cx"], hl["cy"], min_depth=0.1, max_depth=50.0, n_slots=n + 5, grid=spec, device=0,
                            stream=stream.cuda_stream) as ctx:
        for k in range(n + 4):
            d, c = synth.render(scene, poses[k], W, H, hl["fx"], hl["fy"], hl["cx"], hl["cy"], xp=torch, device=dev, noise_sigma=0.001, seed=k)
            ctx.upload(k, d.contiguous(), c.contiguous())
            stream.synchronize()
            del d, c
        ctx.fuse_frames(list(range(n)), poses[:n])
        ctx.sync()
        ctx.set_normal_smoothing(1)
        ctx.build_normals(n - 1)
        ctx.build_normals(n)

        def timed(fn, reps=20, warm=2):
            dev_ms, host_ms = [], []
            for i in range(warm + reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                a.record(stream)
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                b.record(stream)
                b.synchronize()
                if i >= warm:
                    dev_ms.append(a.elapsed_time(b))
                    host_ms.append(1e3 * (t1 - t0))
            return median(dev_ms), median(host_ms)

        if "a" not in args.skip:
            N = 20
            rel = synth.relative_pose(poses[n - 1], poses[n])
            T0 = np.eye(4)
            T0[:3, :3], T0[:3, 3] = rel[0], np.asarray(rel[1]).ravel()
            for stride, gate in ((2, 0.05), (4, 0.20)):
                row = dict(stride=stride, iterations=N)
                for name, iters in (("run", N), ("empty", 0)):
                    lv = [dict(iters=iters, stride=stride, max_dist=gate, eps=0.0, **common)]
                    row["track_dev_ms_" + name], row["track_host_ms_" + name] = timed(lambda: ctx.track(n, poses[n], lv))
                    _, row["icp_host_ms_" + name] = timed(lambda: ctx.icp(n - 1, n, T_init=T0, iters=iters, stride=stride, max_dist=gate, eps=0.0, **common))
                row["track_us_per_iteration_dev"] = round(1e3 * (row["track_dev_ms_run"] - row["track_dev_ms_empty"]) / N, 2)
                row["track_us_per_iteration_host"] = round(1e3 * (row["track_host_ms_run"] - row["track_host_ms_empty"]) / N, 2)
                row["icp_us_per_iteration_host"] = round(1e3 * (row["icp_host_ms_run"] - row["icp_host_ms_empty"]) / N, 2)
                res = ctx.track(n, poses[n], [dict(iters=N, stride=stride, max_dist=gate, eps=0.0, **common)])
                row.update(n_corr=res["n_corr"], n_src=res["n_src"], iters_run=res["iters_run"])
                out["a_stride_%d" % stride] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}
        if "b" not in args.skip:
            scratch = n + 4
            tr_ms, in_ms, rc_ms, nm_ms, icp_ms = [], [], [], [], []
            for k in range(n, n + 4):
                start = poses[k - 1]                       # the previous frame's pose as the start: one step of the orbit off
                _, t = timed(lambda: ctx.track(k, start, chain), reps=5, warm=1)
                tr_ms.append(t)
                _, t = timed(lambda: ctx.raycast(start, min_weight=1, slot=scratch, out=(None, None, None)), reps=5, warm=1)
                rc_ms.append(t)
                _, t = timed(lambda: (ctx.build_normals(scratch, depth_jump=0.02), ctx.sync()), reps=5, warm=1)
                nm_ms.append(t)
                _, t = timed(lambda: ctx.icp_batch([(k, scratch)], chain), reps=5, warm=1)
                icp_ms.append(t)
            for k in range(n, n + 4):                     # the integration last: it changes the model
                t0 = time.perf_counter()
                ctx.integrate(k, poses[k])
                ctx.sync()
                in_ms.append(1e3 * (time.perf_counter() - t0))
            res = ctx.track(n, poses[n - 1], chain)
            out["b"] = dict(track_ms=round(median(tr_ms), 3), integrate_one_frame_ms=round(median(in_ms), 3), raycast_slot_ms=round(median(rc_ms), 3),
                            build_normals_ms=round(median(nm_ms), 3), icp_levels_ms=round(median(icp_ms), 3),
                            stage_ms_per_frame=round(median(tr_ms) + median(in_ms), 3),
                            raycast_route_ms_per_frame=round(median(rc_ms) + median(nm_ms) + median(icp_ms) + median(in_ms), 3),
                            track_iters_run=res["iters_run"], track_status=res["status"], track_fitness=round(res["fitness"], 4))


def part_c(args, out):
    import numpy as np
    import track_reference as tr
    from loop_closure_common import ORBIT_CAM, orbit_frames
    from tl3d.config import ReconstructionConfig
    from tl3d.pipeline import DepthToReconstructionPipeline
    from track_common import ARC, SMALL, arc_frames, centre_errors_mm

    def run(cam, frames, **kw):
        import contextlib
        import io
        pipe = DepthToReconstructionPipeline(ReconstructionConfig(fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], subsample_factor=2,
                                                                  grid_dim=512, **kw))
        pipe.set_frames([c for d, c in frames], [d for d, c in frames])
        with contextlib.redirect_stdout(io.StringIO()):
            pipe.reconstruct()
        return pipe

    def errors(pipe, truth):
        T = np.stack([tr.pose_matrix(p) for p in pipe.camera_poses])
        e = centre_errors_mm(T, truth)
        return dict(mean_mm=round(float(e.mean()), 4), last_mm=round(float(e[-1]), 4))

    poses, frames = arc_frames()
    truth = np.stack([tr.pose_matrix(p) for p in poses])
    rows = {}
    for name, kw in (("chain", {}), ("tracked_26mm", dict(model_tracking=True)), ("tracked_13mm", dict(model_tracking=True, track_voxel_size=0.013)),
                     ("tracked_6.5mm", dict(model_tracking=True, track_voxel_size=0.0065))):
        pipe = run(SMALL, frames, voxel_size=ARC["voxel"], **kw)
        rows[name] = errors(pipe, truth)
        if "model_tracking" in pipe.stats:
            rows[name].update(stats=pipe.stats["model_tracking"], track_s=pipe.timings["track_s"],
                              frames_per_s=round((len(frames) - 1) / pipe.timings["track_s"], 1))
    out["c_arc_%d_frames_%g_mm_noise" % (ARC["n"], ARC["noise"] * 1e3)] = rows
    frames, truth = orbit_frames(72, 0.002)
    rows = {}
    for name, kw in (("chain", {}), ("loop_closure", dict(loop_closure=True)), ("tracked_20mm", dict(model_tracking=True)),
                     ("tracked_10mm", dict(model_tracking=True, track_voxel_size=0.01)), ("tracked_5mm", dict(model_tracking=True, track_voxel_size=0.005)),
                     ("loop_closure_and_tracked_5mm", dict(loop_closure=True, model_tracking=True, track_voxel_size=0.005))):
        pipe = run(ORBIT_CAM, frames, voxel_size=0.02, **kw)
        rows[name] = errors(pipe, truth)
        if "model_tracking" in pipe.stats:
            rows[name].update(stats=pipe.stats["model_tracking"], track_s=pipe.timings["track_s"],
                              frames_per_s=round((len(frames) - 1) / pipe.timings["track_s"], 1))
    out["c_closed_orbit_72_frames_2_mm_noise"] = rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48, help="headline frames fused into the model of (a) and (b)")
    ap.add_argument("--skip", type=str, default="", help="comma-separated parts to leave out: a, b, c")
    args = ap.parse_args()
    args.skip = set(args.skip.split(",")) if args.skip else set()
    out = {}
    if not {"a", "b"} <= args.skip:
        part_ab(args, out)
    if "c" not in args.skip:
        part_c(args, out)
    for k, v in out.items():
        print(json.dumps({k: v}))


if __name__ == "__main__":
    main()
