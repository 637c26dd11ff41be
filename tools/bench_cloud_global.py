"""The global registration front end on the GPU (tl3d_cloud_voxel_subsample, tl3d_cloud_fpfh, tl3d_feature_match, tl3d_cloud_ransac and
the recipe metrics.global_align_clouds) beside the same recipe in numpy + cKDTree on the host.

The four-solids scene of tests/cloud_global_common.py at --sizes points per cloud (two independent samplings, the source un-moved by
130 degrees and 1.4 m), subsampled at --voxel.  Whole calls on device tensors, device events, [median, min] of --reps after one
warm-up, each call on what the recipe feeds it:
  subsample_ms      both clouds at full size
  normals_ms        estimate_normals of both subsamples (k = 30 within the feature radius, the centroid as the viewpoint)
  fpfh_ms           compute_fpfh of both subsamples (k = 48 within 5 voxels); fpfh_full_ms: of the source at FULL size with k = 32 and
                    k = 64 within the same radius (the two instantiations at a size where the index matters)
  match_ms          match_features both ways
  ransac_ms         ransac_register over the mutual pairs, --hypotheses samples
  recipe_ms         metrics.global_align_clouds, host arrays in (it indexes the subsamples on the host), wall clock around it too
  host              the numpy restatement (tests/cloud_global_reference.py; neighbours by brute force, normals by
                    tests/cloud_normals_common.py's cKDTree PCA), wall clock, once; features matched through cKDTree
                    (match_ckdtree_ms, what recipe_ms counts) and by the restatement's brute force (match_ms, for the winner check)
Checks that the GPU recipe's winner is the host's.  Prints one JSON line; --out FILE also writes it there behind a header.

    python tools/bench_cloud_global.py [--sizes 20000 200000] [--voxel 0.03] [--hypotheses 100000] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20_000, 200_000])
    ap.add_argument("--voxel", type=float, default=0.03)
    ap.add_argument("--hypotheses", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from scipy.spatial import cKDTree
    import tl3d
    from tl3d import metrics
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cloud_global_common as cc
    import cloud_global_reference as gr
    import cloud_normals_common as cn

    dev = torch.device("cuda", 0)
    voxel, radius, gate = args.voxel, 5 * args.voxel, 1.5 * args.voxel

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

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        return round(1e3 * (time.perf_counter() - t0), 1), out

    rows = []
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as ctx:
        for n in args.sizes:
            s = cc.scene(0.0, n / 2600.0)
            src, tgt = np.array(s["src"]), np.array(s["tgt"])
            ts, tt = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
            row = dict(points=[len(src), len(tgt)], voxel=voxel, hypotheses=args.hypotheses)
            row["subsample_ms"], (ia, ib) = timed(lambda: (ctx.voxel_subsample(ts, voxel), ctx.voxel_subsample(tt, voxel)))
            pa, pb = ts[ia.long()].contiguous(), tt[ib.long()].contiguous()
            row["subsampled"] = [len(pa), len(pb)]
            ca, cb = (p.double().mean(dim=0).cpu().numpy()[None] for p in (pa, pb))
            row["normals_ms"], (na, nb) = timed(lambda: (ctx.estimate_normals(pa, 30, radius, ca, radius / 2),
                                                         ctx.estimate_normals(pb, 30, radius, cb, radius / 2)))
            row["fpfh_ms"], (fa, fb) = timed(lambda: (ctx.compute_fpfh(pa, na, 48, radius, radius / 2), ctx.compute_fpfh(pb, nb, 48, radius, radius / 2)))
            full_n = torch.from_numpy(np.array(s["src_normals"])).to(dev)
            row["fpfh_full_ms"] = {f"k{k}": timed(lambda: ctx.compute_fpfh(ts, full_n, k, radius, radius / 2))[0] for k in (32, 64)}
            row["match_ms"], (ab, ba) = timed(lambda: (ctx.match_features(fa, fb), ctx.match_features(fb, fa)))
            ab_h, ba_h = ab.cpu().numpy(), ba.cpu().numpy()
            has, mut = gr.mutual_pairs(ab_h, ba_h)
            corr = np.stack([np.arange(len(ab_h))[mut], ab_h[mut]], axis=1).astype(np.int32)
            tc = torch.from_numpy(corr).to(dev)
            row["mutual_pairs"] = len(corr)
            row["ransac_ms"], res = timed(lambda: ctx.ransac_register(pa, pb, tc, hypotheses=args.hypotheses, max_dist=gate))
            row["ransac"] = dict(inliers=res["inliers"], scored=res["n_passed"], best_h=res["best_h"])
            kw = dict(voxel=voxel, hypotheses=args.hypotheses)
            row["recipe_ms"], got = timed(lambda: metrics.global_align_clouds(ctx, src, tgt, **kw))
            row["recipe_wall_ms"] = wall(lambda: metrics.global_align_clouds(ctx, src, tgt, **kw))[0]
            row["displacement_m"] = round(cc.displacement(got["T"], s["T"], src), 5)
            if not args.no_host:
                host = {}
                host["subsample_ms"], (ha, hb) = wall(lambda: (src[gr.voxel_subsample(src, voxel)], tgt[gr.voxel_subsample(tgt, voxel)]))
                host["normals_ms"], (hna, hnb) = wall(lambda: tuple(
                    cn.ref(p, 30, radius, p.astype(np.float64).mean(axis=0)[None]).normals.astype(np.float32) for p in (ha, hb)))
                # the GPU's normals from here on, so that the host's winner can be compared with the GPU's
                hna, hnb = na.cpu().numpy(), nb.cpu().numpy()
                host["fpfh_ms"], (hfa, hfb) = wall(lambda: (gr.fpfh(ha, hna, 48, radius)["fpfh"], gr.fpfh(hb, hnb, 48, radius)["fpfh"]))
                # (flat regions give many EXACTLY equal descriptors: a tree answers such ties as it likes, so it is timed, and the
                # winner check goes through the restatement's brute force, which has the contract's tie rule)
                host["match_ckdtree_ms"] = wall(lambda: (cKDTree(hfb.astype(np.float64)).query(hfa.astype(np.float64))[1],
                                                         cKDTree(hfa.astype(np.float64)).query(hfb.astype(np.float64))[1]))[0]
                host["match_ms"], (hab, hba) = wall(lambda: (gr.match_features(hfa, hfb)[0], gr.match_features(hfb, hfa)[0]))
                _, hmut = gr.mutual_pairs(hab, hba)
                hcorr = np.stack([np.arange(len(hab))[hmut], hab[hmut]], axis=1).astype(np.int32)
                host["ransac_ms"], hres = wall(lambda: gr.ransac(ha, hb, hcorr, args.hypotheses, gate))
                host["recipe_ms"] = round(sum(v for k, v in host.items() if k.endswith("_ms") and k != "match_ms"), 1)
                host["same_winner"] = bool(hres["best_h"] == got["best_h"] and hres["inliers"] == got["inliers"])
                row["host"] = host
                row["recipe_speedup_over_host"] = round(host["recipe_ms"] / row["recipe_wall_ms"], 1)
            rows.append(row)
            del ts, tt
    line = json.dumps(dict(reps=args.reps, sizes=rows))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(f"# python tools/bench_cloud_global.py --sizes {' '.join(map(str, args.sizes))} --voxel {args.voxel} --hypotheses {args.hypotheses} "
                    f"--reps {args.reps}  (one MI355X;\n# device tensors, device events, [median, min] of {args.reps} whole calls after one warm-up; "
                    f"host_*: numpy + cKDTree, wall clock, once; ms)\n{line}\n")


if __name__ == "__main__":
    main()
