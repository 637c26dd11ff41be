"""Registration of two unorganised clouds on the GPU (tl3d_cloud_register) against one nearest_points call of the
same sizes and against a k-d tree ICP in numpy.

A synthetic surface: n target points on a wavy height field over [0, 4]^2 m with its analytic normals (the density of a fused cloud:
a sheet, not a volume); the source is the same points jittered by 2 mm, in shuffled order, moved by 1 degree and 1 cm.  Times whole
calls (device tensors in, device events, median and min of --reps after one warm-up), for every size in --sizes and for queries in
cell order (the default: re-bucketed once per level) and in input order:
  setup_ms          a level of 0 iterations: the two bounds passes and their wait, the target's index, one search + reduce + step
  iteration_ms      (a level of --iters iterations that never converges (eps = 0) - setup) / --iters; point-to-plane, and
                    point-to-point (three rows per pair)
  default_ms        the default two levels (10 iterations of every 4th point at 20 cm, then 15 of all at 5 cm)
  nearest_points_ms one call of the same sizes on the same arrays: it builds the index every time
  ckdtree_*         cKDTree(target) once, then per iteration query(moved source, workers=16) and the normal equations in numpy
Checks that both orders give the same pose bytes and that the GPU's pose equals the k-d tree ICP's to 1e-9 after the same iterations.
Prints one JSON line; --out FILE also writes it there behind a header.  --once N: one default run at N points and nothing else (the
run to put under a kernel trace for the split between search, reduce and step).

    python tools/bench_cloud_register.py [--sizes 1000000 4000000] [--reps 3] [--iters 10] [--out FILE]
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
    x, y = r.uniform(0.0, 4.0, n), r.uniform(0.0, 4.0, n)
    z = 0.3 * np.sin(2.0 * x) * np.cos(1.5 * y)
    nrm = np.stack([-0.6 * np.cos(2.0 * x) * np.cos(1.5 * y), 0.45 * np.sin(2.0 * x) * np.sin(1.5 * y), np.ones(n)], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.stack([x, y, z], axis=1).astype(np.float32), nrm.astype(np.float32)


def planted(np):
    a = np.radians(1.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = (0.006, -0.006, 0.005)
    return T


def kd_icp(np, tree, src, tgt, nrm, iters, max_dist, workers, se3_apply, solve):
    """Point-to-plane ICP with the same update rule, neighbours from the tree: (T, seconds per iteration)."""
    T = np.eye(4)
    p = src.astype(np.float64)
    t64, n64 = tgt.astype(np.float64), nrm.astype(np.float64)
    t0 = time.perf_counter()
    for _ in range(iters):
        q = p @ T[:3, :3].T + T[:3, 3]
        d, i = tree.query(q, workers=workers, distance_upper_bound=max_dist)
        ok = np.isfinite(d)
        q, y, n = q[ok], t64[i[ok]], n64[i[ok]]
        r = np.einsum("ij,ij->i", n, q - y)
        J = np.concatenate([np.cross(q, n), n], axis=1)
        A = J.T @ J
        A7 = np.zeros((7, 7))
        A7[:6, :6] = A
        b7 = np.zeros(7)
        b7[:6] = J.T @ r
        x, _ = solve(A7[np.triu_indices(7)], b7, 6, 1e-6, 1e-4)
        T = se3_apply(x, T)
    return T, (time.perf_counter() - t0) / max(iters, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 4_000_000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kd-iters", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from scipy.spatial import cKDTree
    import tl3d
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cloud_register_reference as cr

    dev = torch.device("cuda", 0)

    def timed(fn, reps=args.reps):
        ms = []
        for r in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            if r >= 1:
                ms.append(a.elapsed_time(b))
        return [round(float(np.median(ms)), 3), round(float(np.min(ms)), 3)], out

    def clouds(n):
        tgt, nrm = surface(np, n, 1)
        r = np.random.default_rng(2)
        moved = (tgt + r.normal(scale=0.002, size=tgt.shape).astype(np.float32))[r.permutation(n)].astype(np.float64)
        P = planted(np)
        src = ((moved - P[:3, 3]) @ P[:3, :3]).astype(np.float32)          # P maps the source onto the target
        return src, tgt, nrm

    rows = []
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as ctx:
        if args.once:
            src, tgt, nrm = clouds(args.once)
            ts, tt, tn = (torch.from_numpy(a).to(dev) for a in (src, tgt, nrm))
            ctx.register_clouds(ts, tt, tn)
            res = ctx.register_clouds(ts, tt, tn)
            print(json.dumps(dict(points=args.once, status=res["status"], iters_run=res["iters_run"], rmse=res["rmse"])))
            return
        for n in args.sizes:
            src, tgt, nrm = clouds(n)
            ts, tt, tn = (torch.from_numpy(a).to(dev) for a in (src, tgt, nrm))
            row = dict(points=n)
            poses = {}
            for name, cell_order in (("cell_order", True), ("input_order", False)):
                ctx.set_nearest_query_order(cell_order)
                lv0 = [dict(iters=0, stride=1, max_dist=0.05)]
                lvk = [dict(iters=args.iters, stride=1, max_dist=0.05, eps=0.0)]
                t_0, _ = timed(lambda: ctx.register_clouds(ts, tt, tn, levels=lv0))
                t_k, res = timed(lambda: ctx.register_clouds(ts, tt, tn, levels=lvk))
                t_p, _ = timed(lambda: ctx.register_clouds(ts, tt, None, levels=lvk))
                t_d, dres = timed(lambda: ctx.register_clouds(ts, tt, tn))
                t_n, _ = timed(lambda: ctx.nearest_points(ts, tt))
                assert res["iters_run"] == args.iters and res["status"] == 0
                poses[name] = (res["T"].tobytes(), dres["T"].tobytes())
                row[name] = dict(setup_ms=t_0, level_ms=t_k, iteration_plane_ms=round((t_k[0] - t_0[0]) / args.iters, 3),
                                 iteration_point_ms=round((t_p[0] - t_0[0]) / args.iters, 3), default_ms=t_d, nearest_points_ms=t_n,
                                 default_status=dres["status"], default_iters_last_level=dres["iters_run"], default_rmse=dres["rmse"],
                                 default_pose_error=float(np.linalg.norm(dres["T"] - planted(np))))
                if cell_order:
                    gpu_T = ctx.register_clouds(ts, tt, tn, levels=[dict(iters=args.kd_iters, stride=1, max_dist=0.05, eps=0.0)])["T"]
            ctx.set_nearest_query_order(True)
            t0 = time.perf_counter()
            tree = cKDTree(tgt.astype(np.float64))
            build = time.perf_counter() - t0
            kd_T, per_iter = kd_icp(np, tree, src, tgt, nrm, args.kd_iters, 0.05, args.workers, cr.se3_apply, cr.solve)
            row.update(orders_give_same_bytes=poses["cell_order"] == poses["input_order"], ckdtree_build_ms=round(1e3 * build, 1),
                       ckdtree_icp_iteration_ms=round(1e3 * per_iter, 1), ckdtree_workers=args.workers,
                       pose_diff_to_ckdtree_icp=float(np.linalg.norm(gpu_T - kd_T)),
                       iteration_over_nearest_points=round(row["cell_order"]["iteration_plane_ms"] / row["cell_order"]["nearest_points_ms"][0], 3),
                       speedup_over_ckdtree_iteration=round(1e3 * per_iter / row["cell_order"]["iteration_plane_ms"], 1))
            rows.append(row)
            del ts, tt, tn
    line = json.dumps(dict(reps=args.reps, iters=args.iters, sizes=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"# python tools/bench_cloud_register.py --sizes {' '.join(map(str, args.sizes))} --reps {args.reps} --iters {args.iters}  (one MI355X; device\n"
                    f"# tensors, device events, [median, min] of {args.reps} whole calls after one warm-up; the k-d tree on the host, wall clock; ms)\n{line}\n")


if __name__ == "__main__":
    main()
