"""Mesh extraction against TSDF-mode point extraction on the headline grid.

Fuses the headline orbit (synth.HEADLINE: 512 frames of 1080x1920 into 512^3 voxels at 5 mm, TSDF + centroid channels), then
times, with device events after a warm-up, one complete tl3d_extract(TL3D_EXTRACT_TSDF) and one complete tl3d_extract_mesh
(size query + fill into device buffers, as a caller makes them), median of --reps calls each.  Prints V, T, both times and the
algorithmic bytes of the three mesh passes over the mesh time as a fraction of 8 TB/s.

    python tools/bench_mesh.py [--reps 20] [--frames 512] [--components]

--components adds the mesh component filter: one complete tl3d_mesh_filter_components of the extracted
mesh (device buffers in, device buffers out, threshold --min-triangles) timed the same way beside the extraction it follows, and
the scipy restatement of the same filter (tests/mesh_components_reference.py) on the host, wall clock.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--group", type=int, default=64, help="frames resident at once")
    ap.add_argument("--components", action="store_true", help="also time the component filter on the extracted mesh, and its host reference")
    ap.add_argument("--min-triangles", type=int, default=100)
    args = ap.parse_args()
    import numpy as np
    import torch
    import tl3d
    from tl3d import _cabi as abi
    from tl3d import synth

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

        def tsdf_points():
            n = C.c_int64(0)
            abi.check(lib.tl3d_extract(ctx._h, abi.EXTRACT_TSDF, 1, 0, 1.0, None, None, 0, C.byref(n)))
            return n.value

        def mesh_counts():
            nv, nt = C.c_int64(0), C.c_int64(0)
            abi.check(lib.tl3d_extract_mesh(ctx._h, 0, None, None, 0, None, 0, C.byref(nv), C.byref(nt)))
            return nv.value, nt.value

        n_pts = tsdf_points()
        nv, nt = mesh_counts()
        pxyz = torch.empty((max(1, n_pts), 3), dtype=torch.float32, device=dev)
        prgb = torch.empty((max(1, n_pts), 3), dtype=torch.uint8, device=dev)
        mxyz = torch.empty((max(1, nv), 3), dtype=torch.float32, device=dev)
        mrgb = torch.empty((max(1, nv), 3), dtype=torch.uint8, device=dev)
        mtri = torch.empty((max(1, nt), 3), dtype=torch.int32, device=dev)
        n = C.c_int64(0)
        ov, ot = C.c_int64(0), C.c_int64(0)

        def run_tsdf():
            abi.check(lib.tl3d_extract(ctx._h, abi.EXTRACT_TSDF, 1, 0, 1.0, None, None, 0, C.byref(n)))
            abi.check(lib.tl3d_extract(ctx._h, abi.EXTRACT_TSDF, 1, 0, 1.0, abi.ptr(pxyz), abi.ptr(prgb), n.value, C.byref(n)))

        def run_mesh():
            abi.check(lib.tl3d_extract_mesh(ctx._h, 0, None, None, 0, None, 0, C.byref(ov), C.byref(ot)))
            abi.check(lib.tl3d_extract_mesh(ctx._h, 0, abi.ptr(mxyz), abi.ptr(mrgb), ov.value, abi.ptr(mtri), ot.value, C.byref(ov),
                                            C.byref(ot)))

        def timed(fn, invalidate):
            ms = []
            for r in range(args.reps + 2):
                invalidate()                      # each call counts again, as a fresh size query does after new frames
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                if r >= 2:
                    ms.append(a.elapsed_time(b))
            return float(np.median(ms)), float(np.min(ms))

        # the count caches are keyed on the grid epoch: a grid pointer hand-out bumps it without touching the records
        def invalidate():
            p = C.c_void_p(0)
            nb = C.c_size_t(0)
            abi.check(lib.tl3d_grid_device_ptr(ctx._h, abi.CH_TSDF, C.byref(p), C.byref(nb)))
        t_tsdf = timed(run_tsdf, invalidate)
        t_mesh = timed(run_mesh, invalidate)
        a = ctx.extract_mesh()
        b = ctx.extract_mesh()
        same = all(np.array_equal(x, y) for x, y in zip(a, b))
        comp = None
        if args.components:
            import time
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import mesh_components_reference as mcr
            run_mesh()                                              # mxyz / mrgb / mtri hold the mesh
            fxyz, frgb, ftri = torch.empty_like(mxyz), torch.empty_like(mrgb), torch.empty_like(mtri)
            cnt = [C.c_int64(0) for _ in range(4)]

            def run_filter():
                abi.check(lib.tl3d_mesh_filter_components(ctx._h, abi.ptr(mxyz), abi.ptr(mrgb), nv, abi.ptr(mtri), nt, args.min_triangles, 0,
                                                          abi.ptr(fxyz), abi.ptr(frgb), nv, abi.ptr(ftri), nt, None,
                                                          *[C.byref(c) for c in cnt]))
            t_filter = timed(run_filter, lambda: None)
            t0 = time.perf_counter()
            want = mcr.filter_mesh(*a, args.min_triangles)
            t_host = time.perf_counter() - t0
            kv, kt = cnt[0].value, cnt[1].value
            equal = (kv == len(want[0]) and kt == len(want[2]) and np.array_equal(fxyz[:kv].cpu().numpy(), want[0])
                     and np.array_equal(frgb[:kv].cpu().numpy(), want[1]) and np.array_equal(ftri[:kt].cpu().numpy().view(np.uint32), want[2]))
            comp = dict(min_triangles=args.min_triangles, components=cnt[2].value, components_kept=cnt[3].value, vertices_kept=kv,
                        triangles_kept=kt, filter_ms_median=round(t_filter[0], 3), filter_ms_min=round(t_filter[1], 3),
                        filter_over_mesh_extract=round(t_filter[0] / t_mesh[0], 3), host_reference_ms=round(1e3 * t_host, 1),
                        host_over_filter=round(1e3 * t_host / t_filter[0], 1), equals_host_reference=bool(equal))
    nvox = spec.nvox
    # algorithmic bytes of the three mesh passes: every TSDF record read once per pass, the vertex / triangle outputs, the
    # first-id scratch written once per vertex owner (<= V) and read three times per triangle, colour records (two per vertex at most)
    bytes_mesh = 3 * nvox * 8 + nv * 15 + nt * 12 + nv * 4 + nt * 3 * 4 + nv * 2 * 32
    bytes_tsdf = 2 * nvox * 8 + n_pts * 15 + n_pts * 2 * 32
    res = dict(grid=spec.dims, voxel=spec.voxel_size, frames=args.frames, tsdf_points=n_pts, mesh_vertices=nv, mesh_triangles=nt,
               tsdf_extract_ms_median=round(t_tsdf[0], 3), tsdf_extract_ms_min=round(t_tsdf[1], 3),
               mesh_extract_ms_median=round(t_mesh[0], 3), mesh_extract_ms_min=round(t_mesh[1], 3),
               mesh_over_tsdf=round(t_mesh[0] / t_tsdf[0], 3),
               mesh_alg_bytes=bytes_mesh, mesh_frac_of_8TBps=round(bytes_mesh / (t_mesh[0] * 1e-3) / 8e12, 4),
               tsdf_alg_bytes=bytes_tsdf, tsdf_frac_of_8TBps=round(bytes_tsdf / (t_tsdf[0] * 1e-3) / 8e12, 4),
               repeat_identical=bool(same), reps=args.reps)
    if comp is not None:
        res["components"] = comp
    print(json.dumps(res))


if __name__ == "__main__":
    main()
