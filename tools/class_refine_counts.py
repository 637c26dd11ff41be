#!/usr/bin/env python3
"""What the refinement of replayed classification entries (tl3d_class_refine_info) decides on the headline job: the frames, poses,
camera and grid of plain `bench.py --gpus 1` (512 resident 1080 x 1920 frames of the object scene, 0.70 degrees apart, into a
512^3 grid of 5 mm voxels), fused as six scans with a reset between: the first saves the classification entries, the next four
refine them (eight frames of a 32-frame batch at a time), the sixth replays the refined ones.  Prints the cache's and the refinement's counters after every scan.
    python tools/class_refine_counts.py [--frames 512] [--u16]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import tl3d  # noqa: E402
from tl3d import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--u16", action="store_true")
    a = ap.parse_args()
    W, H, n = 1080, 1920, a.frames
    cam = dict(fx=1719.0, fy=1719.0, cx=W / 2.0, cy=H / 2.0)
    dev = torch.device("cuda", 0)
    scene = synth.object_scene(with_room=True)
    poses = synth.orbit_poses(n, 1.0, 360.0 / 512)
    spec = tl3d.GridSpec.cube(512, 0.005, centre=(0.0, -0.1, 0.0), channels=tl3d.CH_TSDF)
    # one explicit stream shared by torch (frame synthesis) and the library, so every hand-over is ordered (as bench.py does)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    with tl3d.FusionContext(W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"], min_depth=0.1, max_depth=50.0, n_slots=n, grid=spec,
                            device=0, stream=stream.cuda_stream) as ctx:
        for i, p in enumerate(poses):
            d, c = synth.render(scene, p, W, H, cam["fx"], cam["fy"], cam["cx"], cam["cy"], xp=torch, device=dev)
            if a.u16:
                d = torch.clamp(torch.round(d * 1000.0), 0, 65535).to(torch.int32).to(torch.uint16)
            ctx.upload(i, d.contiguous(), c.contiguous())
            stream.synchronize()                      # the tensors are freed right after: finish the copy first
        names = ("seen", "dropped", "free", "both_kinds", "masks_did_not_fit")
        for scan in range(6):
            ctx.reset()
            ctx.fuse_frames(list(range(n)), poses)
            ctx.sync()
            cl = ctx.class_cache_info()
            rf = ctx.class_refine_info()
            print(f"scan {scan}: classified {cl[0]} replayed {cl[1]} overflowed {cl[2]} | refine pairs per {n} frames: "
                  + " ".join(f"{k} {v}" for k, v in zip(names, rf)), flush=True)
        # the bricks behind those pairs: one more scan in counting mode (MIXED bricks = visited - free)
        ctx.reset()
        ctx.reset_stats()
        ctx.set_profile(count_records=True)
        ctx.fuse_frames(list(range(n)), poses)
        ctx.sync()
        st = ctx.stats()
        print(f"per {n} frames: bricks visited {st['tsdf_bricks_visited']} free {st['tsdf_bricks_free']} "
              f"records read {st['tsdf_records_read']} written {st['tsdf_records_written']}", flush=True)


if __name__ == "__main__":
    main()
