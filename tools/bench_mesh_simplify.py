"""Vertex-clustering simplification of the headline mesh (DESIGN.md sections 4.2.2 and 7.7).

Fuses the headline orbit as tools/bench_mesh.py does (synth.HEADLINE: 512 frames of 1080x1920 into 512^3 voxels at 5 mm), extracts
the mesh into device buffers, then times, with device events after two warm-ups, one complete tl3d_mesh_simplify_clusters (device
buffers in, device buffers out, origin (0, 0, 0)) at cells of --cells voxels, median of --reps calls each, and one complete
tl3d_mesh_filter_components of the same mesh for scale.  Prints vertices and triangles in and out and the ms per cell size, beside
the extraction figure of DESIGN.md section 7.7, and whether the result equals the numpy restatement of the rules
(tests/mesh_simplify_reference.py) on the host.  --placement quadric times tl3d_mesh_simplify_quadric (reg 2^-10) instead, against
tests/mesh_simplify_quadric_reference.py; --placement both times the two calls of one build side by side, cell by cell.

    python tools/bench_mesh_simplify.py [--reps 20] [--frames 512] [--cells 2,4,8] [--placement mean|quadric|both] [--no-check]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MESH_EXTRACT_MS = 3.73          # tl3d_extract_mesh of the same grid (tools/bench_mesh.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--group", type=int, default=64, help="frames resident at once")
    ap.add_argument("--cells", type=str, default="2,4,8", help="cell sizes in voxels")
    ap.add_argument("--min-triangles", type=int, default=100, help="threshold of the component filter timed for scale")
    ap.add_argument("--placement", choices=("mean", "quadric", "both"), default="mean", help="which call(s) to time")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the restatement on the host")
    args = ap.parse_args()
    import numpy as np
    import torch
    import tl3d
    from tl3d import _cabi as abi
    from tl3d import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mesh_simplify_quadric_reference as mqr
    import mesh_simplify_reference as msr

    hl = synth.HEADLINE
    W, H = hl["width"], hl["height"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    scene = synth.object_scene(with_room=True)
    poses = synth.orbit_poses(args.frames, hl["radius"], 360.0 / args.frames)
    spec = tl3d.GridSpec.cube(hl["grid"], hl["voxel"], centre=(0.0, -0.1, 0.0), channels=tl3d.CH_TSDF | tl3d.CH_CENTROID)
    G = min(args.group, args.frames)
    ctx = tl3d.FusionContext(W, H, hl["fx"], hl["fy"], hl["cx"], hl["cy"], min_depth=0.1, max_depth=50.0, n_slots=G, grid=spec,
                             device=0, stream=stream.cuda_stream)
    lib = abi.load()
    with ctx:
        for g0 in range(0, args.frames, G):
            ks = list(range(g0, min(args.frames, g0 + G)))
            for s, k in enumerate(ks):
                d, c = synth.render(scene, poses[k], W, H, hl["fx"], hl["fy"], hl["cx"], hl["cy"], xp=torch, device=dev)
                ctx.upload(s, d.contiguous(), c.contiguous())
                stream.synchronize()
                del d, c
            ctx.fuse_frames(list(range(len(ks))), [poses[k] for k in ks], centroid_subsample=2)
        ctx.sync()
        mxyz, mrgb, mtri = (torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in ctx.extract_mesh())
        nv, nt = len(mxyz), len(mtri)
        oxyz, orgb, otri = torch.empty_like(mxyz), torch.empty_like(mrgb), torch.empty_like(mtri)
        cnt = [C.c_int64(0) for _ in range(7)]

        def timed(fn):
            ms = []
            for r in range(args.reps + 2):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                if r >= 2:
                    ms.append(a.elapsed_time(b))
            return float(np.median(ms)), float(np.min(ms))

        def run_filter():
            abi.check(lib.tl3d_mesh_filter_components(ctx._h, abi.ptr(mxyz), abi.ptr(mrgb), nv, abi.ptr(mtri), nt, args.min_triangles, 0,
                                                      abi.ptr(oxyz), abi.ptr(orgb), nv, abi.ptr(otri), nt, None, *[C.byref(c) for c in cnt[:4]]))
        t_filter = timed(run_filter)
        host = [a.cpu().numpy() for a in (mxyz, mrgb, mtri)]
        host[2] = host[2].view(np.uint32)
        rows = []
        for vox in [float(v) for v in args.cells.split(",")]:
            cell = vox * hl["voxel"]

            def run_mean():
                abi.check(lib.tl3d_mesh_simplify_clusters(ctx._h, abi.ptr(mxyz), abi.ptr(mrgb), nv, abi.ptr(mtri), nt, cell, None, abi.ptr(oxyz),
                                                          abi.ptr(orgb), nv, abi.ptr(otri), nt, None, *[C.byref(c) for c in cnt[:4]]))

            def run_quadric():
                abi.check(lib.tl3d_mesh_simplify_quadric(ctx._h, abi.ptr(mxyz), abi.ptr(mrgb), nv, abi.ptr(mtri), nt, cell, None, mqr.REG,
                                                         abi.ptr(oxyz), abi.ptr(orgb), nv, abi.ptr(otri), nt, None, *[C.byref(c) for c in cnt]))
            mean = None
            for placement in ("mean", "quadric"):
                if args.placement not in (placement, "both"):
                    continue
                t = timed(run_mean if placement == "mean" else run_quadric)
                kv, kt = cnt[0].value, cnt[1].value
                row = dict(cell_voxels=vox, cell_m=cell, placement=placement, vertices_out=kv, triangles_out=kt, degenerate_dropped=cnt[2].value,
                           duplicates_dropped=cnt[3].value, simplify_ms_median=round(t[0], 3), simplify_ms_min=round(t[1], 3),
                           simplify_over_mesh_extract=round(t[0] / MESH_EXTRACT_MS, 3))
                if placement == "quadric":
                    row.update(quadric_placed=cnt[4].value, clamped=cnt[5].value, corners_skipped=cnt[6].value)
                if not args.no_check:
                    t0 = time.perf_counter()
                    mean = mean if mean is not None else msr.simplify(*host, cell)
                    want = mean if placement == "mean" else mqr.simplify(*host, cell, mean=mean)
                    t_host = time.perf_counter() - t0
                    equal = (kv == len(want[0]) and kt == len(want[2]) and np.array_equal(oxyz[:kv].cpu().numpy(), want[0])
                             and np.array_equal(orgb[:kv].cpu().numpy(), want[1])
                             and np.array_equal(otri[:kt].cpu().numpy().view(np.uint32), want[2])
                             and (placement == "mean" or [c.value for c in cnt[4:]] == [want[3][k] for k in ("quadric_placed", "clamped",
                                                                                                            "corners_skipped")]))
                    row.update(host_reference_ms=round(1e3 * t_host, 1), equals_host_reference=bool(equal))
                rows.append(row)
    print(json.dumps(dict(grid=spec.dims, voxel=spec.voxel_size, frames=args.frames, vertices_in=nv, triangles_in=nt, reps=args.reps,
                          mesh_extract_ms_design_7_7=MESH_EXTRACT_MS, filter_components_ms_median=round(t_filter[0], 3),
                          filter_components_ms_min=round(t_filter[1], 3), cells=rows)))


if __name__ == "__main__":
    main()
