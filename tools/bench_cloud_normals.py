"""Normals and curvature of a cloud on the GPU (tl3d_estimate_normals) against the k-NN stage it
contains and against a 16-worker k-d tree with a batched eigen-solver on the host.

A synthetic surface: n points on a wavy height field over [0, 4]^2 m (the density of a fused cloud: a sheet, not a volume).  Times
complete calls (device tensors in and out, device events, median and min of --reps after one warm-up), k = 30 neighbours, the search
cell twice the mean point spacing (what 2 x voxel_size is to a fused cloud):
  estimate_normals      without viewpoints, and with 512 of them (camera centres 1.5 m above the sheet)
  knn_mean_distance     the same n, k and cell: the nearest existing kernel (kernels_sor.hip), a k-NN without indices
  cKDTree(points).query(points, k, workers=16) + numpy.linalg.eigh of the n covariances, on the host (wall clock, once, in slices)
for every size in --sizes.  Checks the GPU normals against the host's by the bar of tests/cloud_normals_common.py on the points
whose k-th distance is no tie.  Prints one JSON line; --out FILE also writes it there behind a two-line header
(profiles/cloud_normals.txt is made that way).

    python tools/bench_cloud_normals.py [--sizes 1000000 4000000] [--reps 5] [--out profiles/cloud_normals.txt]
"""
import argparse
import ctypes as C
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


def viewpoints(np, m):
    g = int(round(m ** 0.5 + 0.5))
    x, y = np.meshgrid(np.linspace(0.2, 3.8, g), np.linspace(0.2, 3.8, g), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(g * g, 1.5)], axis=1)[:m].astype(np.float64)


def host_normals(np, cKDTree, p32, k, workers, step=500_000):
    """(normals, lambda, k-th and (k+1)-th distance, seconds of the tree's build, of its queries, of the covariances and eigh)"""
    p = p32.astype(np.float64)
    n = len(p)
    t0 = time.perf_counter()
    tree = cKDTree(p)
    t_build = time.perf_counter() - t0
    nrm, lam, dk = np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 2))
    t_query = t_eig = 0.0
    for s in range(0, n, step):
        t0 = time.perf_counter()
        d, idx = tree.query(p[s:s + step], k=k + 1, workers=workers)
        t1 = time.perf_counter()
        e = p[idx[:, :k]] - p[s:s + step, None, :]
        e -= e.mean(axis=1, keepdims=True)
        w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", e, e))
        t2 = time.perf_counter()
        nrm[s:s + step], lam[s:s + step], dk[s:s + step] = v[:, :, 0], w, d[:, k - 1:k + 1]
        t_query += t1 - t0
        t_eig += t2 - t1
    return nrm, lam, dk, t_build, t_query, t_eig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 4_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--neighbors", type=int, default=30)
    ap.add_argument("--viewpoints", type=int, default=512)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from scipy.spatial import cKDTree
    import tl3d
    from tl3d import _cabi as abi

    dev = torch.device("cuda", 0)
    k = args.neighbors

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
    vp = viewpoints(np, args.viewpoints)
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as ctx:
        for n in args.sizes:
            pts = surface(np, n, 1)
            cell = 2.0 * (16.0 / n) ** 0.5
            tp = torch.from_numpy(pts).to(dev)
            mean = torch.empty(n, dtype=torch.float64, device=dev)

            def knn():                                     # the binding's knn_mean_distance takes host arrays; the C call takes both
                abi.check(ctx._lib.tl3d_knn_mean_distance(ctx._h, abi.ptr(tp), n, k, cell, abi.ptr(mean)))
                return mean
            row = dict(points=n, neighbors=k, cell=round(cell, 6), viewpoints=len(vp))
            row["estimate_normals_ms"], plain = timed(lambda: ctx.estimate_normals(tp, k, cell_size=cell, curvature=True))
            row["estimate_normals_viewpoints_ms"], seen = timed(lambda: ctx.estimate_normals(tp, k, cell_size=cell, viewpoints=vp, curvature=True))
            row["knn_mean_distance_ms"], _ = timed(knn)
            row["degenerate"] = ctx.last_normals_degenerate
            hn, lam, dk, t_build, t_query, t_eig = host_normals(np, cKDTree, pts, k, args.workers)
            g = plain[0].cpu().numpy().astype(np.float64)
            gap = lam[:, 1] - lam[:, 0]
            ok = (dk[:, 0] < dk[:, 1]) & (gap > 0)
            bound = 2.0 ** -22 + 1024 * 2.0 ** -52 * lam[ok, 2] / gap[ok]
            sin = np.linalg.norm(np.cross(g[ok], hn[ok]), axis=1)
            up = seen[0].cpu().numpy()[:, 2]
            e = row["estimate_normals_ms"][0]
            row.update(ckdtree_build_ms=round(1e3 * t_build, 1), ckdtree_query_ms=round(1e3 * t_query, 1), host_covariance_eigh_ms=round(1e3 * t_eig, 1),
                       ckdtree_workers=args.workers, compared=int(ok.sum()), over_the_bar=int((sin > bound).sum()),
                       max_sin_over_bound=float((sin / bound).max()), towards_the_viewpoints=bool((up > 0).all()),
                       normals_over_knn_stage=round(e / row["knn_mean_distance_ms"][0], 2),
                       viewpoints_cost_ms=round(row["estimate_normals_viewpoints_ms"][0] - e, 3),
                       speedup_over_host=round(1e3 * (t_query + t_eig) / e, 1))
            rows.append(row)
            del tp, mean, plain, seen
    line = json.dumps(dict(reps=args.reps, sizes=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"# python tools/bench_cloud_normals.py --sizes {' '.join(map(str, args.sizes))} --reps {args.reps}  (one MI355X; device tensors,\n"
                    f"# device events, [median, min] of {args.reps} whole calls after one warm-up; the k-d tree and eigh on the host, wall clock; ms)\n{line}\n")


if __name__ == "__main__":
    main()
