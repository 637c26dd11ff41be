"""Blocked fusion of a lattice beyond 2^32 voxels: the 2 m x 2.4 m x 120 m corridor at 5 mm (VGA, 0.5 m per frame, max depth 4 m,
given poses).  Per block: count (choose_layout), attach + core, fuse, extract (centroid points), keyed mesh, detach -- wall time
after a device sync each -- then the whole reconstruct() with extract_mesh.  One JSON line per block and one for the
whole run.
    python tools/bench_blocks.py [--frames 240] [--mesh 1] [--mesh-weld host|device]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tl3d  # noqa: E402
from tl3d import _cabi as abi  # noqa: E402
from tl3d import pipeline as pl  # noqa: E402
from tl3d import synth  # noqa: E402
from tl3d.config import ReconstructionConfig  # noqa: E402
from tl3d.pipeline import DepthToReconstructionPipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--mesh", type=int, default=1)
    ap.add_argument("--mesh-weld", choices=("host", "device"), default="host", help="where reconstruct() welds the blocks' meshes")
    args = ap.parse_args()
    W, H = 640, 480
    cam = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0)
    scene = synth.Scene(room=((-1.0, -1.2, -0.5), (1.0, 1.2, 120.0)))
    poses = synth.dolly_poses(args.frames, (0.0, 0.0, 0.0), (0.0, 0.0, 0.5))
    frames = [synth.render(scene, p, W, H, **cam) for p in poses]
    cfg = ReconstructionConfig(**cam, voxel_size=0.005, subsample_factor=2, grid_dim=512, max_depth=4.0, outlier_filter=False,
                               extract_mesh=bool(args.mesh), mesh_weld=args.mesh_weld if args.mesh else "host")
    n = len(frames)
    slots = list(range(n))
    clock = time.perf_counter
    with tl3d.FusionContext(W, H, cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.min_depth, cfg.max_depth, n_slots=n) as ctx:
        for i, (d, c) in enumerate(frames):
            ctx.upload(i, d, c)
        scales = [1.0] * n
        mn, mx = ctx.frames_bounds(slots, poses, scales, subsample=cfg.subsample_factor)
        lattice = pl.plan_lattice(mn, mx, cfg.voxel_size, cfg.grid_dim, trunc_voxels=cfg.sdf_trunc_voxels)
        blocks = pl.plan_blocks(lattice)
        print(json.dumps(dict(lattice=lattice.dims, nvox=lattice.nvox, blocks=len(blocks), frames=n)))
        for k, b in enumerate(blocks):
            ctx.sync()
            t0 = clock()
            layout = pl.choose_layout(ctx, b.grid, slots, poses, scales, cfg.subsample_factor, log=lambda *a: None)
            t1 = clock()
            ctx.attach_grid(layout)
            ctx.set_block_core(lattice.dims, b.lo, b.hi)
            ctx.sync()
            t2 = clock()
            ctx.fuse_frames(slots, poses, scales, centroid_subsample=cfg.subsample_factor)
            ctx.sync()
            t3 = clock()
            xyz, _ = ctx.extract(abi.EXTRACT_CENTROID, min_count=1, min_weight=cfg.tsdf_min_weight, max_abs_tsdf=cfg.tsdf_max_abs)
            t4 = clock()
            nv = nt = 0
            if args.mesh:
                mx_, _, mt, _ = ctx.extract_mesh(min_weight=cfg.tsdf_min_weight, keys=True)
                nv, nt = len(mx_), len(mt)
            t5 = clock()
            ctx.detach_grid()
            t6 = clock()
            print(json.dumps(dict(block=k, offset=layout.voxel_offset, dims=layout.dims, sparse=layout.sparse,
                                  gib=round(layout.device_bytes() / 2 ** 30, 2), points=len(xyz), mesh_vertices=nv, mesh_triangles=nt,
                                  count_s=round(t1 - t0, 3), attach_s=round(t2 - t1, 3), fuse_s=round(t3 - t2, 3),
                                  extract_s=round(t4 - t3, 3), mesh_s=round(t5 - t4, 3), detach_s=round(t6 - t5, 3))))
    pipe = DepthToReconstructionPipeline(cfg)
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    t0 = clock()
    pts, _, _ = pipe.reconstruct(poses=poses)
    t1 = clock()
    print(json.dumps(dict(reconstruct_s=round(t1 - t0, 3), points=len(pts), blocks=pipe.stats["blocks"],
                          points_dropped=pipe.stats["points_dropped"], pool_refused=pipe.stats["pool_refused"],
                          mesh_vertices=pipe.stats.get("mesh_vertices"), mesh_triangles=pipe.stats.get("mesh_triangles"),
                          mesh_weld=cfg.mesh_weld, timings=pipe.timings)))


if __name__ == "__main__":
    main()
