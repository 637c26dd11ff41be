"""Planar regions of a cloud on the GPU (tl3d_segment_planes) against the normal estimation that feeds it and
against a k-d tree with scipy's connected components on the host.

A synthetic corridor: n points on the floor, the ceiling and the two walls of a corridor 2 m x 2.4 m, 8 m long, uniformly spread
with a depth noise of a tenth of the point spacing v = sqrt(area / n) (the density of a cloud fused at a voxel of v).  Normals and
curvature are the GPU's own (estimate_normals, k = 30, turned towards the corridor's axis).  The parameters are the pipeline's
defaults for a voxel of v: radius 2.5 v, 10 degrees, offset v, curvature 0.05, 200 points, rms 0.5 v; the search cell is the radius.
Times complete calls (device tensors in and out, device events, median and min of --reps after one warm-up):
  segment_planes        the whole call; and its passes by device events, from a child process that loads the experiments flavour of
                        the library with TL3D_PLANES_TRACE (median over the same number of calls)
  estimate_normals      k = 30 with curvature on the same points
  host                  cKDTree.query_pairs + the exact predicate (tests/plane_segments_reference.py) + scipy's connected_components,
                        wall clock, once (query_pairs takes no worker count; the rest is numpy)
and checks the GPU's partition against the host's.  Prints one JSON line; --out FILE also writes it there behind a header
(profiles/cloud_planes.txt is made that way).

    python tools/bench_cloud_planes.py [--sizes 1000000 4000000] [--reps 5] [--out profiles/cloud_planes.txt]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, L = 2.0, 2.4, 8.0
AREA = 2 * (W + H) * L


def corridor(np, n, seed):
    """(points f32 [n,3], the spacing v): x across, y up, z along"""
    r = np.random.default_rng(seed)
    v = math.sqrt(AREA / n)
    s = r.uniform(0.0, 2 * (W + H), n)                        # where on the cross-section's perimeter
    z = r.uniform(0.0, L, n)
    d = r.normal(0.0, 0.1 * v, n)
    x = np.where(s < W, s, np.where(s < W + H, W + d, np.where(s < 2 * W + H, 2 * W + H - s, d)))
    y = np.where(s < W, d, np.where(s < W + H, s - W, np.where(s < 2 * W + H, H + d, 2 * (W + H) - s)))
    return np.stack([x, y, z], axis=1).astype(np.float32), v


def parameters(v):
    return dict(radius=2.5 * v, max_angle_deg=10.0, max_offset=v, max_curvature=0.05, min_points=200, max_rms=0.5 * v)


def axis_viewpoints(np):
    return np.stack([np.full(17, W / 2), np.full(17, H / 2), np.linspace(0.0, L, 17)], axis=1)


def trace_child(args):
    """the experiments flavour: --reps + 1 calls per size; the library appends the passes' times to TL3D_PLANES_TRACE"""
    import numpy as np
    import torch
    import tl3d
    dev = torch.device("cuda", 0)
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as ctx:
        for n in args.sizes:
            pts, v = corridor(np, n, 1)
            tp = torch.from_numpy(pts).to(dev)
            nrm, cur = ctx.estimate_normals(tp, 30, cell_size=2 * v, viewpoints=axis_viewpoints(np), curvature=True)
            for _ in range(args.reps + 1):
                ctx.segment_planes(tp, nrm, cur, **parameters(v))


def passes(args):
    """{size: {pass: median ms}} from a child process, or None when the experiments flavour is not built"""
    lib = os.path.join(ROOT, "textureless-3d-reconstruction_amd", "libtl3d_exp.so")
    if not os.path.exists(lib):
        return None
    import numpy as np
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "trace.txt")
        env = dict(os.environ, TL3D_LIB=lib, TL3D_PLANES_TRACE=path)
        cmd = [sys.executable, os.path.abspath(__file__), "--trace-child", "--reps", str(args.reps), "--sizes", *map(str, args.sizes)]
        if subprocess.run(cmd, env=env, timeout=600).returncode != 0 or not os.path.exists(path):
            return None
        lines = [ln.split() for ln in open(path).read().splitlines()]
    per = args.reps + 1
    out = {}
    for k, n in enumerate(args.sizes):
        calls = lines[k * per + 1:(k + 1) * per]                # without the warm-up
        names = calls[0][0::2]
        out[n] = {nm: round(float(np.median([float(c[2 * j + 1]) for c in calls])), 3) for j, nm in enumerate(names)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 4_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args)
    import numpy as np
    import torch
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    import plane_segments_reference as pr
    import tl3d

    dev = torch.device("cuda", 0)

    def timed(fn):
        ms = []
        for r in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            if r >= 1:
                ms.append(a.elapsed_time(b))
        return [round(float(np.median(ms)), 3), round(float(np.min(ms)), 3)], out

    rows = []
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as ctx:
        for n in args.sizes:
            pts, v = corridor(np, n, 1)
            prm = parameters(v)
            tp = torch.from_numpy(pts).to(dev)
            row = dict(points=n, spacing=round(v, 6), **{k: (round(x, 6) if isinstance(x, float) else x) for k, x in prm.items()})
            row["estimate_normals_ms"], (nrm, cur) = timed(lambda: ctx.estimate_normals(tp, 30, cell_size=2 * v, viewpoints=axis_viewpoints(np), curvature=True))
            row["segment_planes_ms"], (ids, planes, counts) = timed(lambda: ctx.segment_planes(tp, nrm, cur, **prm))
            row.update(counts=counts, largest=[int(c) for c in sorted(planes["count"].tolist(), reverse=True)[:6]],
                       planes_over_normals=round(row["segment_planes_ms"][0] / row["estimate_normals_ms"][0], 3))
            # the host: pairs, predicate, components (the labels alone: no moments, no planes)
            ref = pr.Params(radius=prm["radius"], min_cos=math.cos(math.radians(10.0)), max_offset=prm["max_offset"], max_curvature=0.05,
                            min_points=200, max_rms=prm["max_rms"])
            n32, c32 = nrm.cpu().numpy(), cur.cpu().numpy()
            p, nn = pts.astype(np.float64), n32.astype(np.float64)
            t0 = time.perf_counter()
            ok = pr.eligible(n32, c32, ref)
            el = np.flatnonzero(ok)
            pairs = cKDTree(p[el]).query_pairs(ref.radius * (1 + 1e-9), output_type="ndarray")
            t1 = time.perf_counter()
            i, j = el[pairs[:, 0]], el[pairs[:, 1]]
            keep = np.zeros(len(i), bool)
            for s in range(0, len(i), 4_000_000):
                keep[s:s + 4_000_000] = pr.linked(p, nn, np.maximum(i[s:s + 4_000_000], j[s:s + 4_000_000]), np.minimum(i[s:s + 4_000_000], j[s:s + 4_000_000]), ref)
            t2 = time.perf_counter()
            _, comp = connected_components(coo_matrix((np.ones(int(keep.sum()), np.int8), (i[keep], j[keep])), shape=(n, n)), directed=False)
            t3 = time.perf_counter()
            # the same partition: GPU plane ids against the host's components, both ways, over the points that have a plane
            got = ids.cpu().numpy()
            on = got >= 0
            both = np.unique(np.stack([got[on], comp[on]], axis=1), axis=0)
            size = np.bincount(comp, weights=ok.astype(np.float64))
            same = len(both) == len(np.unique(both[:, 0])) == len(np.unique(both[:, 1])) and bool(np.all(size[both[:, 1]] == planes["count"][both[:, 0]]))
            host = 1e3 * (t3 - t0)
            row.update(pairs_in_reach=int(len(i)), links=int(keep.sum()), host_query_pairs_ms=round(1e3 * (t1 - t0), 1), host_predicate_ms=round(1e3 * (t2 - t1), 1),
                       host_connected_components_ms=round(1e3 * (t3 - t2), 1), same_partition=bool(same),
                       speedup_over_host=round(host / row["segment_planes_ms"][0], 1))
            rows.append(row)
            del tp, nrm, cur, ids
    tr = passes(args)
    for row in rows:
        row["passes_ms"] = tr[row["points"]] if tr else None
    line = json.dumps(dict(reps=args.reps, sizes=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"# python tools/bench_cloud_planes.py --sizes {' '.join(map(str, args.sizes))} --reps {args.reps}  (one MI355X; device tensors, device\n"
                    f"# events, [median, min] of {args.reps} whole calls after one warm-up; passes_ms: medians from the experiments flavour; the host: wall clock; ms)\n{line}\n")


if __name__ == "__main__":
    main()
