#!/usr/bin/env python3
"""Drop-in command line for the reference's depth_enhanced_reconstruction.py (its __main__ block, :1418-1467).

    python depth_enhanced_reconstruction.py --input ./input_folder/buddha_images --output ./output --fx ... 

--output is a DIRECTORY; the result is <output>/reconstruction.ply (DER:1247).  The reference computes depth with
Depth-Anything fetched by model name (DER:114-118).  That network stays upstream PyTorch-ROCm (it is not part of this back
end); two ways to get depth here:
  --depth-model DIR   a LOCAL checkpoint directory: the upstream transformers classes run it on the GPU (same call sequence
                      as DER:139-165) and the depth tensors go straight into the frame slots, no host copy;
  (default)           depth files written by the reference's depth_processor.py (`<stem>_depth.npy|png`), looked for in
                      --depth-folder, else <input>/depth, <input>_depth, <input>/depth_images, <input>.
--per-frame-ply additionally writes <output>/pointclouds/<stem>.ply per frame, as depth_processor.py does (DP:923-934).
DER's dense defaults are used: depth limits 0.1 / 100 m, subsample 4, voxel 5 mm, no outlier filter.
"""
import argparse
import os
import sys
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    parser = argparse.ArgumentParser(description="Depth-Enhanced 3D Reconstruction")
    parser.add_argument("--input", type=str, default="./input_folder/buddha_images", help="Input folder with images")
    parser.add_argument("--output", type=str, default="./output", help="Output directory")
    parser.add_argument("--fx", type=float, default=1719.0, help="Focal length X")
    parser.add_argument("--fy", type=float, default=1719.0, help="Focal length Y")
    parser.add_argument("--cx", type=float, default=540.0, help="Principal point X")
    parser.add_argument("--cy", type=float, default=960.0, help="Principal point Y")
    parser.add_argument("--no-depth", action="store_true", help="Disable depth estimation")
    parser.add_argument("--no-hybrid", action="store_true", help="Disable hybrid features")
    # additive
    parser.add_argument("--depth-folder", type=str, default=None)
    parser.add_argument("--depth-model", type=str, default=None,
                        help="local Depth-Anything checkpoint directory (save_pretrained layout); never downloaded")
    parser.add_argument("--depth-scale", type=float, default=1.0, help="metric scale of the (relative) depth")
    parser.add_argument("--per-frame-ply", action="store_true", help="also write <output>/pointclouds/<stem>.ply per frame (DP:923-934)")
    parser.add_argument("--grid", type=int, default=1024, help="fusion volume budget: at most GRID^3 voxels in total")
    parser.add_argument("--loop-closure", action="store_true",
                        help="find revisits among the registered poses, register them too and optimise every pose over the resulting graph before fusing")
    parser.add_argument("--model-tracking", action="store_true",
                        help="after the registration, register every kept frame against the TSDF fused from the frames before it and fuse at those poses")
    parser.add_argument("--compare-to", type=str, default=None, metavar="REF.ply",
                        help="score the fused cloud against the vertices of this PLY on the GPU: prints "
                             "one line with the mean Chamfer distance and precision / recall / F-score at the thresholds")
    parser.add_argument("--compare-threshold", type=float, action="append", default=None, metavar="M",
                        help="a distance threshold of --compare-to, in metres (repeatable, at most 8; default 0.005 0.01 0.02)")
    parser.add_argument("--compare-max-dist", type=float, default=None, metavar="M",
                        help="points with no neighbour within this distance count as unmatched (default: no limit)")
    parser.add_argument("--compare-align", action="store_true",
                        help="register the fused cloud onto the --compare-to scan on the GPU first (point-to-plane ICP) and score it "
                             "in the scan's frame; the written files are not moved.  A local method: a scan more than 20 cm away "
                             "needs --compare-align-init")
    parser.add_argument("--compare-align-scale", action="store_true",
                        help="with --compare-align: estimate the scale too (needs a closed or bounded scene: open geometry observes "
                             "the scale weakly)")
    parser.add_argument("--compare-align-init", type=str, default=None, metavar="FILE",
                        help="with --compare-align: a 4x4 matrix (.npy or text) mapping reconstruction to scan, where the registration starts")
    parser.add_argument("--compare-align-global", action="store_true",
                        help="with --compare-align: find the start on the GPU (FPFH features + RANSAC), so the scan may lie anywhere; "
                             "rigid only: not with --compare-align-scale or --compare-align-init")
    parser.add_argument("--compare-align-global-voxel", type=float, default=None, metavar="M",
                        help="with --compare-align-global: the subsampling voxel in metres (default 5 x the voxel size)")
    parser.add_argument("--cloud-normals", action="store_true",
                        help="give the fused cloud per-point normals on the GPU (PCA over the nearest neighbours, turned towards the "
                             "nearest camera) and write them as nx ny nz")
    parser.add_argument("--cloud-normals-neighbors", type=int, default=30, metavar="K",
                        help="neighbours of --cloud-normals, the point itself included (3..64; default 30)")
    parser.add_argument("--cloud-normals-radius", type=float, default=0.0, metavar="M",
                        help="neighbours further than this many metres are left out (default 0: no limit)")
    parser.add_argument("--cloud-curvature", action="store_true",
                        help="with --cloud-normals: also write the surface variation l0 / (l0 + l1 + l2) as `curvature`")
    parser.add_argument("--cloud-planes", action="store_true",
                        help="with --cloud-normals: segment the fused cloud into planar regions on the GPU (walls, floors, ceilings) and "
                             "write each point's plane number as `plane` (-1: none)")
    parser.add_argument("--cloud-planes-angle", type=float, default=10.0, metavar="DEG",
                        help="largest angle between the normals of two linked points (default 10)")
    parser.add_argument("--cloud-planes-min-points", type=int, default=200, metavar="N",
                        help="smallest region that can be a plane (default 200)")
    parser.add_argument("--cloud-planes-max-curvature", type=float, default=0.05, metavar="C",
                        help="points with a surface variation above this take no part (creases; 0: no bound; default 0.05)")
    parser.add_argument("--cloud-planes-report", default=None, metavar="FILE.json",
                        help="with --cloud-planes: write the plane table (normal, d, centroid, rms, count) as JSON")
    parser.add_argument("--depth-filter", action="store_true",
                        help="drop flying pixels and small regions from every depth frame on the GPU before anything reads it "
                             "(registration, tracking, fusion); pixels are only ever invalidated, never altered")
    parser.add_argument("--depth-filter-jump", type=float, default=0.05, metavar="REL",
                        help="two pixels are linked when their depths differ by at most REL times the smaller one (default 0.05)")
    parser.add_argument("--depth-filter-radius", type=int, default=1, metavar="R",
                        help="the support window is (2R+1)^2 pixels (1..3; default 1)")
    parser.add_argument("--depth-filter-min-support", type=int, default=4, metavar="N",
                        help="a pixel with fewer than N linked pixels in its window goes (0..(2R+1)^2-1; default 4)")
    parser.add_argument("--depth-filter-min-region", type=int, default=0, metavar="N",
                        help="a 4-connected region of linked pixels smaller than N goes too (default 0: no such stage)")
    parser.add_argument("--photometric", action="store_true",
                        help="register with colour too: a photometric term beside the point-to-plane one observes the motion geometry "
                             "cannot see (along a tunnel, across a wall)")
    parser.add_argument("--photo-weight", type=float, default=0.1, metavar="W",
                        help="weight of the photometric system beside the geometric one (default 0.1; too small a weight falls under "
                             "the solver's eigenvalue cutoff)")
    parser.add_argument("--photo-gate", type=float, default=0.2, metavar="G",
                        help="largest intensity difference (0..1) of a photometric correspondence (default 0.2)")
    parser.add_argument("--photo-smooth-radius", type=int, default=1, metavar="R",
                        help="the intensity is averaged over (2R+1)^2 pixels on one side of depth edges (0..7; default 1)")
    parser.add_argument("--device", type=int, default=0)
    args = parser.parse_args(argv)

    if args.cloud_curvature and not args.cloud_normals:
        parser.error("--cloud-curvature comes out of the normal estimation: it needs --cloud-normals")
    if not 3 <= args.cloud_normals_neighbors <= 64:
        parser.error("--cloud-normals-neighbors must lie in [3, 64]")
    if (args.cloud_planes or args.cloud_planes_report) and not (args.cloud_planes and args.cloud_normals):
        parser.error("--cloud-planes segments the cloud by its normals: it needs --cloud-normals (and --cloud-planes-report needs --cloud-planes)")
    if args.cloud_planes_min_points < 3:
        parser.error("--cloud-planes-min-points must be 3 at the least")
    if args.depth_filter:
        from tl3d.pipeline import check_depth_filter_options
        try:
            check_depth_filter_options(argparse.Namespace(depth_filter=True, depth_filter_jump=args.depth_filter_jump,
                                                          depth_filter_radius=args.depth_filter_radius,
                                                          depth_filter_min_support=args.depth_filter_min_support,
                                                          depth_filter_min_region=args.depth_filter_min_region))
        except ValueError as e:
            parser.error("--depth-filter: " + str(e))
    if args.compare_threshold and len(args.compare_threshold) > 8:
        parser.error("--compare-threshold: at most 8 thresholds")
    if (args.compare_align or args.compare_align_scale or args.compare_align_init or args.compare_align_global
            or args.compare_align_global_voxel is not None):
        from tl3d.pipeline import check_compare_options
        try:
            check_compare_options(argparse.Namespace(compare_to=args.compare_to, compare_align=args.compare_align,
                                                     compare_align_scale=args.compare_align_scale, compare_align_init=args.compare_align_init,
                                                     compare_align_global=args.compare_align_global,
                                                     compare_align_global_voxel=args.compare_align_global_voxel))
        except ValueError as e:
            parser.error("--compare-align: " + str(e))
    if args.photometric:
        from tl3d.pipeline import check_photometric_options
        try:
            check_photometric_options(argparse.Namespace(photometric=True, photo_weight=args.photo_weight, photo_gate=args.photo_gate,
                                                         photo_smooth_radius=args.photo_smooth_radius, photo_depth_jump=0.05,
                                                         loop_closure=args.loop_closure))
        except ValueError as e:
            parser.error("--photometric: " + str(e))
    from tl3d import fileio
    from tl3d.config import ReconstructionConfig
    from tl3d.pipeline import DepthToReconstructionPipeline

    inp = Path(args.input)
    n_images = len([f for f in inp.iterdir() if f.suffix.lower() in fileio.IMAGE_SUFFIXES]) if inp.is_dir() else 0
    if n_images < 2:
        print("Need at least 2 images for reconstruction")
        return 1
    if args.no_depth:
        print("--no-depth: the sparse-only path of the reference (SIFT/ORB/LSD structure from motion) is out of scope "
              "of the device back end")
        return 1
    config = ReconstructionConfig(fx=args.fx, fy=args.fy, cx=args.cx, cy=args.cy, min_depth=0.1, max_depth=100.0,
                                  voxel_size=0.005, subsample_factor=4, grid_dim=args.grid, device=args.device,
                                  depth_scale=args.depth_scale, loop_closure=args.loop_closure, model_tracking=args.model_tracking,
                                  depth_filter=args.depth_filter, depth_filter_jump=args.depth_filter_jump,
                                  depth_filter_radius=args.depth_filter_radius, depth_filter_min_support=args.depth_filter_min_support,
                                  depth_filter_min_region=args.depth_filter_min_region,
                                  photometric=args.photometric, photo_weight=args.photo_weight, photo_gate=args.photo_gate,
                                  photo_smooth_radius=args.photo_smooth_radius,
                                  cloud_planes=args.cloud_planes, cloud_planes_angle_deg=args.cloud_planes_angle,
                                  cloud_planes_min_points=args.cloud_planes_min_points, cloud_planes_max_curvature=args.cloud_planes_max_curvature,
                                  cloud_normals=args.cloud_normals, cloud_normals_neighbors=args.cloud_normals_neighbors,
                                  cloud_normals_radius=args.cloud_normals_radius, cloud_curvature=args.cloud_curvature,
                                  compare_to=args.compare_to, compare_max_dist=args.compare_max_dist,
                                  compare_thresholds=tuple(args.compare_threshold) if args.compare_threshold else (0.005, 0.01, 0.02),
                                  compare_align=args.compare_align, compare_align_scale=args.compare_align_scale,
                                  compare_align_init=args.compare_align_init,
                                  compare_align_global=args.compare_align_global,
                                  compare_align_global_voxel=args.compare_align_global_voxel,
                                  outlier_filter=False)                   # DER's merge_pointclouds has no outlier filter (DER:615-645)
    pipeline = DepthToReconstructionPipeline(config)
    if args.depth_model:
        from tl3d.depthnet import LocalDepthEstimator
        try:
            net = LocalDepthEstimator(args.depth_model, device=args.device)
        except FileNotFoundError as e:
            print(e)
            return 1
        files = sorted(f for f in inp.iterdir() if f.suffix.lower() in fileio.IMAGE_SUFFIXES)
        print(f"Found {len(files)} images")
        images, names = [], []
        for f in files:
            img = fileio.read_image_bgr(f)
            if img is not None:
                images.append(img)
                names.append(f.name)
        print("\n--- Step 1: Estimating depth maps ---")                  # DER:1081
        depths = []
        for i, img in enumerate(images):
            depths.append(net.estimate(img))                              # float32 [H, W] on the GPU
            print(f"  Depth {i + 1}/{len(images)}")
        pipeline.set_frames(images, depths, names)
        loaded = len(images)
        del net
    else:
        cands = [args.depth_folder] if args.depth_folder else [inp / "depth", Path(str(inp) + "_depth"), inp / "depth_images", inp]
        loaded = 0
        for c in cands:
            if c is not None and Path(c).is_dir():
                # per-frame clouds are exported from host arrays; otherwise the frames stream from the files to the GPU
                loaded = (pipeline.load_data if args.per_frame_ply else pipeline.load_data_streaming)(str(inp), str(c))
                if loaded >= 2:
                    break
        if loaded < 2:
            print("No depth maps found next to the images. Pass --depth-model <local Depth-Anything checkpoint directory> to "
                  "estimate them here (upstream PyTorch-ROCm), or run the reference's depth_processor.py (or any producer of "
                  "<stem>_depth.npy / .png) first and pass --depth-folder.")
            return 1
    if loaded < 2:
        print("Need at least 2 images for reconstruction")
        return 1
    out_dir = Path(args.output)
    if args.per_frame_ply:
        k = pipeline.export_frame_clouds(out_dir, subsample=config.subsample_factor)
        print(f"Saved {k} per-frame clouds to {out_dir / 'pointclouds'}")
    result = pipeline.reconstruct()
    if result[0] is None or len(result[0]) == 0:
        print("Reconstruction failed")
        return 0
    points, colors, poses = result
    out_dir.mkdir(parents=True, exist_ok=True)
    fileio.save_reconstruction(points, colors, out_dir / "reconstruction.ply", normals=pipeline.cloud_normals,
                               curvature=pipeline.cloud_curvature, planes=pipeline.cloud_plane_ids)
    if args.cloud_planes_report:
        fileio.write_plane_report(args.cloud_planes_report, pipeline.cloud_planes)
    print(f"Saved {len(points)} points to {out_dir / 'reconstruction.ply'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
