"""Cloud-to-cloud and cloud-to-mesh nearest-neighbour search on the GPU against a 16-worker k-d tree.

A synthetic surface: n points on a wavy height field over [0, 4]^2 m (the density of a fused cloud: a sheet, not a volume), and the
same points jittered by 2 mm in shuffled order as the queries; the mesh is the height field's own triangle grid (2 (m - 1)^2
triangles, m^2 ~ n / 2 vertices).  Times complete calls (device tensors in and out, device events, median and min of --reps after one
warm-up):
  nearest_points    n queries against n points, queries in cell order (the default) and in input order
  nearest_triangles n queries against the mesh, both orders
  cKDTree(points).query(queries, workers=16) on the same arrays, build and query apart (host, wall clock, once)
for every size in --sizes.  Checks that both orders give the same bytes and that the distances equal the tree's to 1e-12 relative.
Prints one JSON line; --out FILE also writes it there behind a two-line header (profiles/cloud_distance.txt is made that way).

    python tools/bench_cloud_distance.py [--sizes 1000000 4000000] [--reps 5] [--out profiles/cloud_distance.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def surface(np, n, seed):
    r = np.random.default_rng(seed)
    xy = r.uniform(0.0, 4.0, (n, 2))
    z = 0.3 * np.sin(2.0 * xy[:, 0]) * np.cos(1.5 * xy[:, 1])
    return np.concatenate([xy, z[:, None]], axis=1).astype(np.float32)


def grid_mesh(np, m):
    g = np.linspace(0.0, 4.0, m)
    x, y = np.meshgrid(g, g, indexing="ij")
    z = 0.3 * np.sin(2.0 * x) * np.cos(1.5 * y)
    idx = np.arange(m * m, dtype=np.int64).reshape(m, m)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(np.uint32)
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32), tris


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 4_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from scipy.spatial import cKDTree
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
            target = surface(np, n, 1)
            r = np.random.default_rng(2)
            query = (target + r.normal(scale=0.002, size=target.shape).astype(np.float32))[r.permutation(n)]
            m = int(round((n / 2) ** 0.5))
            vxyz, tris = grid_mesh(np, m)
            tq, tt = torch.from_numpy(query).to(dev), torch.from_numpy(target).to(dev)
            tv, ti = torch.from_numpy(vxyz).to(dev), torch.from_numpy(tris.view(np.int32)).to(dev)
            row = dict(points=n, mesh_vertices=len(vxyz), mesh_triangles=len(tris))
            res = {}
            for name, cell_order in (("cell_order", True), ("input_order", False)):
                ctx.set_nearest_query_order(cell_order)
                row[f"nearest_points_{name}_ms"], res["p" + name] = timed(lambda: ctx.nearest_points(tq, tt))
                row[f"nearest_triangles_{name}_ms"], res["t" + name] = timed(lambda: ctx.nearest_triangles(tq, tv, ti))
            ctx.set_nearest_query_order(True)
            same = all(torch.equal(res[k + "cell_order"][j], res[k + "input_order"][j]) for k in "pt" for j in (0, 1))
            t0 = time.perf_counter()
            tree = cKDTree(target.astype(np.float64))
            t1 = time.perf_counter()
            kd, _ = tree.query(query.astype(np.float64), workers=args.workers)
            t2 = time.perf_counter()
            gd = res["pcell_order"][0].cpu().numpy()
            row.update(ckdtree_build_ms=round(1e3 * (t1 - t0), 1), ckdtree_query_ms=round(1e3 * (t2 - t1), 1), ckdtree_workers=args.workers,
                       orders_give_same_bytes=bool(same), max_rel_diff_to_ckdtree=float(np.max(np.abs(gd - kd) / np.maximum(kd, 1e-300))),
                       mean_point_distance=float(gd.mean()), mean_surface_distance=float(res["tcell_order"][0].mean().item()))
            q = row["nearest_points_cell_order_ms"][0]
            row["points_speedup_over_ckdtree_query"] = round(row["ckdtree_query_ms"] / q, 1)
            row["cell_order_gain_points"] = round(row["nearest_points_input_order_ms"][0] / q, 2)
            row["cell_order_gain_triangles"] = round(row["nearest_triangles_input_order_ms"][0] / row["nearest_triangles_cell_order_ms"][0], 2)
            rows.append(row)
            del tq, tt, tv, ti, res
    line = json.dumps(dict(reps=args.reps, sizes=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"# python tools/bench_cloud_distance.py --sizes {' '.join(map(str, args.sizes))} --reps {args.reps}  (one MI355X; device tensors,\n"
                    f"# device events, [median, min] of {args.reps} whole calls after one warm-up; the k-d tree on the host, wall clock; ms)\n{line}\n")


if __name__ == "__main__":
    main()
