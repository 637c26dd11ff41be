"""Taubin smoothing and vertex normals of the headline mesh (DESIGN.md sections 4.2.3 and 7.7).

Fuses the headline orbit as tools/bench_mesh.py does (synth.HEADLINE: 512 frames of 1080x1920 into 512^3 voxels at 5 mm), extracts
the mesh into device buffers, then times complete calls with device events after two warm-ups, median of --reps calls each, device
buffers in and out:
  tl3d_mesh_smooth_taubin at iterations 0 (validation, edge table, valences), 1 and 11, from which
      one step            = (t(11) - t(1)) / 20
      the adjacency build = t(1) - 2 steps   (validation, edge table, valences, row scan, row fill)
  tl3d_mesh_vertex_normals (validation, corner count, row scan, corner fill, the gather).
Prints them beside the extraction's and the clustering's figures of section 7.7 and beside the bytes each pass must move at least,
and whether one iteration and the normals equal the Python-integer restatement of the rules (tests/mesh_smooth_reference.py; --no-check
skips it: it takes the host a minute).

The three parts are differences of whole calls (each call includes its waits for the stream), from the medians and, beside
them, from the smallest times.  --out FILE also writes the result there, behind a two-line header (profiles/mesh_smooth.txt is made
that way).

    python tools/bench_mesh_smooth.py [--reps 20] [--frames 512] [--no-check] [--out profiles/mesh_smooth.txt]
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
SIMPLIFY_MS = (0.76, 0.82)      # tl3d_mesh_simplify_clusters of the same mesh at cells of 2..8 voxels (tools/bench_mesh_simplify.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--group", type=int, default=64, help="frames resident at once")
    ap.add_argument("--no-check", action="store_true", help="skip the comparison with the host reference")
    ap.add_argument("--out", type=str, default=None, help="also write the result to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import tl3d
    from tl3d import _cabi as abi
    from tl3d import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mesh_smooth_reference as ref

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
        hxyz, _, htri = ctx.extract_mesh()
        mxyz, mtri = torch.from_numpy(hxyz).to(dev), torch.from_numpy(htri.view(np.int32)).to(dev)
        nv, nt = len(mxyz), len(mtri)
        oxyz, onrm, oval = torch.empty_like(mxyz), torch.empty_like(mxyz), torch.empty(nv, dtype=torch.int32, device=dev)
        ne, nz = C.c_int64(0), C.c_int64(0)

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

        def smooth(it):
            def run():
                abi.check(lib.tl3d_mesh_smooth_taubin(ctx._h, abi.ptr(mxyz), nv, abi.ptr(mtri), nt, it, 0.5, -0.53, abi.ptr(oxyz), abi.ptr(oval),
                                                      C.byref(ne)))
            return run

        def normals():
            abi.check(lib.tl3d_mesh_vertex_normals(ctx._h, abi.ptr(mxyz), nv, abi.ptr(mtri), nt, abi.ptr(onrm), C.byref(nz)))
        t0, t1, t11, tn = timed(smooth(0)), timed(smooth(1)), timed(smooth(11)), timed(normals)
        step = (t11[0] - t1[0]) / 20.0
        build = t1[0] - 2.0 * step
        step_min = (t11[1] - t1[1]) / 20.0                          # the same from the smallest times of the calls
        build_min = t1[1] - 2.0 * step_min
        E = ne.value
        val = oval.cpu().numpy()
        # what each pass must move at least, every array once (a gathered array counts once: the rest is the caches' business)
        b_edges = 12 * nt + 8 * E + 2 * 4 * nv                     # the triangles, a key per edge, the valences (cleared, then added to)
        b_build = b_edges + 12 * nv + 2 * (4 + 8) * nv + 8 * E + 2 * 4 * E      # + validation of xyz, rows and cursors, keys again, the rows
        b_step = (4 + 8) * nv + 2 * 4 * E + 2 * 12 * nv            # valence, row, the row's entries, positions in and out
        b_norm = 12 * nv + 2 * 12 * nt + (4 + 4 + 8) * nv + 2 * 12 * nt + 12 * nt + 2 * 12 * nv   # validate, count + fill, rows, gather, out
        out = dict(grid=spec.dims, voxel=spec.voxel_size, frames=args.frames, vertices=nv, triangles=nt, edges=E, max_valence=int(val.max()),
                   mean_valence=round(float(val.mean()), 3), zero_normals=nz.value, reps=args.reps,
                   smooth_0_iterations_ms=[round(v, 3) for v in t0], smooth_1_iteration_ms=[round(v, 3) for v in t1],
                   smooth_11_iterations_ms=[round(v, 3) for v in t11], normals_ms=[round(v, 3) for v in tn],
                   step_ms=round(step, 4), adjacency_build_ms=round(build, 3), smooth_10_iterations_ms_derived=round(build + 20 * step, 3),
                   step_ms_from_min=round(step_min, 4), adjacency_build_ms_from_min=round(build_min, 3),
                   min_bytes=dict(edge_table=b_edges, adjacency_build=b_build, step=b_step, normals=b_norm),
                   step_GBps_of_min_bytes=round(b_step / (step * 1e-3) / 1e9, 1) if step > 0 else None,
                   mesh_extract_ms_design_7_7=MESH_EXTRACT_MS, simplify_ms_design_7_7=list(SIMPLIFY_MS),
                   dominant="adjacency build" if build > max(20 * step, tn[0]) else ("steps (10 iterations)" if 20 * step > tn[0] else "normals"))
        if not args.no_check:
            smooth(1)()
            normals()
            t = time.perf_counter()
            want, info = ref.smooth(hxyz, htri, 1)
            wn, wz = ref.normals(hxyz, htri)
            out["host_reference_s"] = round(time.perf_counter() - t, 1)
            out["equals_host_reference"] = bool(np.array_equal(oxyz.cpu().numpy().view(np.uint8), want.view(np.uint8)) and E == info["edges"]
                                                and np.array_equal(oval.cpu().numpy().view(np.uint32), info["valence"])
                                                and np.array_equal(onrm.cpu().numpy().view(np.uint8), wn.view(np.uint8)) and nz.value == wz)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"# python tools/bench_mesh_smooth.py --reps {args.reps} --frames {args.frames}  (one MI355X; device buffers, device events,\n"
                    f"# [median, min] of {args.reps} calls after two warm-ups; times in ms)\n{line}\n")


if __name__ == "__main__":
    main()
