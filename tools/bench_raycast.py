"""Ray casting of the headline grid.

Fuses the headline orbit (synth.HEADLINE: 1080x1920 frames into 512^3 voxels at 5 mm) into a dense grid (TSDF + centroid
channels, as the headline runs) and into a sparse TSDF grid of the same frames, then renders 1080x1920 views into device
buffers at fused poses and at poses half-way between them.  Times each view with device events (median over the views,
after warm-up calls), checks that the sparse grid renders the dense grid's depth and normals, and counts the samples per ray
with the numpy restatement (tests/raycast_reference.py) on every 16th pixel of two views.

    python tools/bench_raycast.py [--frames 512] [--views 16]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--views", type=int, default=16, help="views of each kind (fused poses, poses in between)")
    ap.add_argument("--group", type=int, default=64, help="frames resident at once")
    ap.add_argument("--no-count", action="store_true", help="skip the sample count of the numpy restatement")
    args = ap.parse_args()
    import numpy as np
    import torch
    import tl3d
    from tl3d import synth

    hl = synth.HEADLINE
    W, H = hl["width"], hl["height"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    scene = synth.object_scene(with_room=True)
    step = 360.0 / args.frames
    poses = synth.orbit_poses(args.frames, hl["radius"], step)
    half = synth.orbit_poses(2 * args.frames, hl["radius"], step / 2.0)[1::2]        # half-way between fused cameras
    spec = tl3d.GridSpec.cube(hl["grid"], hl["voxel"], centre=(0.0, -0.1, 0.0), channels=tl3d.CH_TSDF | tl3d.CH_CENTROID)
    G = min(args.group, args.frames)

    def context(grid):
        return tl3d.FusionContext(W, H, hl["fx"], hl["fy"], hl["cx"], hl["cy"], min_depth=0.1, max_depth=50.0, n_slots=G,
                                  grid=grid, device=0, stream=stream.cuda_stream)

    def fuse(ctx, centroid):
        for g0 in range(0, args.frames, G):
            ks = list(range(g0, min(args.frames, g0 + G)))
            for s, k in enumerate(ks):
                d, c = synth.render(scene, poses[k], W, H, hl["fx"], hl["fy"], hl["cx"], hl["cy"], xp=torch, device=dev)
                ctx.upload(s, d.contiguous(), c.contiguous())
                stream.synchronize()
                del d, c
            ctx.fuse_frames(list(range(len(ks))), [poses[k] for k in ks], centroid_subsample=2 if centroid else 0)
        ctx.sync()

    idx = np.linspace(0, args.frames - 1, args.views).astype(int)
    views = [("fused", poses[i]) for i in idx] + [("between", half[i]) for i in idx]
    out = (torch.empty((H, W), dtype=torch.float32, device=dev), torch.empty((H, W, 3), dtype=torch.float32, device=dev),
           torch.empty((H, W, 3), dtype=torch.uint8, device=dev))

    def timed(ctx):
        for _ in range(3):
            ctx.raycast(views[0][1], out=out)
        ms = {"fused": [], "between": []}
        for kind, pose in views:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            a.record(stream)
            ctx.raycast(pose, out=out)
            b.record(stream)
            b.synchronize()
            ms[kind].append(a.elapsed_time(b))
        return ms

    res = dict(grid=spec.dims, voxel=spec.voxel_size, frames=args.frames, image=[H, W], views_per_kind=args.views)
    dense = context(spec)
    with dense:
        fuse(dense, True)
        ms = timed(dense)
        allms = ms["fused"] + ms["between"]
        res.update(dense_ms_median=round(float(np.median(allms)), 4), dense_ms_min=round(float(np.min(allms)), 4),
                   dense_ms_fused_median=round(float(np.median(ms["fused"])), 4),
                   dense_ms_between_median=round(float(np.median(ms["between"])), 4),
                   rays_per_s=round(W * H / (float(np.median(allms)) * 1e-3), 0))
        ref = []
        hits = []
        for _, pose in views[:: max(1, len(views) // 4)]:
            d, n, _ = dense.raycast(pose)
            ref.append((pose, d, n))
            hits.append(float((d > 0).mean()))
        res["hit_fraction_mean"] = round(float(np.mean(hits)), 4)
        st = dense.stats()
        tsdf = dense.download_grid(tl3d.CH_TSDF).reshape(-1, 512, 2)
        occupied = int((tsdf[:, :, 1] > 0).any(axis=1).sum())
        if args.no_count:
            tsdf = None
    torch.cuda.empty_cache()
    sp_spec = tl3d.GridSpec(spec.dims, spec.origin, spec.voxel_size, spec.sdf_trunc, tl3d.CH_TSDF,
                            pool_tsdf=min(int(occupied * 1.5) + 64, spec.nvox // 512 - 1))    # (bricks that saw free space only take slots too)
    sparse = context(sp_spec)
    with sparse:
        fuse(sparse, False)
        sst = sparse.stats()
        ms = timed(sparse)
        allms = ms["fused"] + ms["between"]
        res.update(sparse_pool_bricks=sp_spec.pool_tsdf, sparse_slots_used=sst["pool_slots_tsdf"], sparse_refused=sst["pool_refused"],
                   sparse_ms_median=round(float(np.median(allms)), 4), sparse_ms_min=round(float(np.min(allms)), 4))
        same = True
        for pose, d, n in ref:
            d2, n2, _ = sparse.raycast(pose)
            same = same and np.array_equal(d, d2) and np.array_equal(n, n2)
        res["sparse_equals_dense"] = bool(same)
    if tsdf is not None:
        import raycast_reference as rr
        cam = dict(width=W, height=H, fx=hl["fx"], fy=hl["fy"], cx=hl["cx"], cy=hl["cy"])
        vv, uu = np.mgrid[0:H:16, 0:W:16]
        counts = []
        for pose, d, _ in (ref[0], ref[-1]):
            z, _, _, nsamp = rr.raycast(tsdf, spec.dims, spec.origin, spec.voxel_size, spec.sdf_trunc, cam, pose, z_near=0.1,
                                        z_far=50.0, pixels=(uu.ravel(), vv.ravel()))
            assert np.array_equal(z, d[vv.ravel(), uu.ravel()]), "restatement and device disagree"
            counts.append(nsamp)
        spr = float(np.mean(np.concatenate(counts)))
        # every sample gathers 8 TSDF records (8 B each) and its brick's table entry (4 B, once per brick change); the hit adds
        # 8 records for the normal and one centroid record (32 B)
        recs = W * H * (spr * 8 + 8 * res["hit_fraction_mean"])
        res.update(samples_per_ray_mean=round(spr, 2), samples_per_ray_max=int(np.max(np.concatenate(counts))),
                   records_per_view=int(recs), record_bytes_per_view=int(recs * 8),
                   gather_GBps_at_median=round(recs * 8 / (res["dense_ms_median"] * 1e-3) / 1e9, 1),
                   ns_per_sample=round(res["dense_ms_median"] * 1e6 / (W * H * spr), 5))
    res["tsdf_launches"] = st["tsdf_launches"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
