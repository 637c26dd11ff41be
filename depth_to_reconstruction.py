#!/usr/bin/env python3
"""Drop-in command line for the reference's depth_to_reconstruction.py, running its dense back end on an MI355X.

    python depth_to_reconstruction.py --rgb-folder R --depth-folder D --output out.ply --fx 525 --fy 525 --cx 320 --cy 240

Same flags and defaults as the reference's main() (depth_to_reconstruction.py:770-786) and the same .ply out.
Poses come from on-device point-to-plane ICP (the reference used SIFT + essential matrix), fusion is on-device
voxel accumulation (the reference used np.vstack + Open3D).  Additive flags configure those two stages.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _spawn_ranks(n, argv):
    """--gpus N outside torchrun: start N copies of this command line, one per GPU, BEFORE anything touches a GPU here
    (children are fresh processes; the parent only watches them: the first rank that fails -- by a signal too -- ends the group
    with a non-zero status, the wait is bounded).  Rendezvous on 127.0.0.1."""
    import importlib.util
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("tl3d_launch", os.path.join(here, "textureless-3d-reconstruction_amd", "launch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.spawn_ranks(os.path.abspath(__file__), list(argv), n)


def _init_rank(args):
    """This process is one rank: bind it to its GPU and join the group (backend "nccl" = RCCL over xGMI; TL3D_DIST_BACKEND=gloo
    and TL3D_SHARE_DEVICE=1 let several ranks share one GPU for tests)."""
    import tl3d  # noqa: F401  (GPU_MAX_HW_QUEUES before the first HIP call)
    import torch
    import torch.distributed as dist
    local = int(os.environ.get("LOCAL_RANK", "0"))
    args.device = 0 if os.environ.get("TL3D_SHARE_DEVICE") == "1" else local
    torch.cuda.set_device(args.device)
    backend = os.environ.get("TL3D_DIST_BACKEND", "nccl")
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", args.device))
    else:
        dist.init_process_group(backend)
    return dist


def main(argv=None):
    parser = argparse.ArgumentParser(description="Depth to 3D Reconstruction")
    parser.add_argument("--rgb-folder", type=str, required=True, help="Folder with RGB images")
    parser.add_argument("--depth-folder", type=str, required=True, help="Folder with depth images")
    parser.add_argument("--output", type=str, default="./output/reconstruction.ply", help="Output PLY file path")
    parser.add_argument("--fx", type=float, default=1719.0)
    parser.add_argument("--fy", type=float, default=1719.0)
    parser.add_argument("--cx", type=float, default=540.0)
    parser.add_argument("--cy", type=float, default=960.0)
    parser.add_argument("--voxel-size", type=float, default=0.005)
    parser.add_argument("--subsample", type=int, default=2)
    parser.add_argument("--no-vis", action="store_true")
    # additive
    parser.add_argument("--grid", type=int, default=1024,
                        help="fusion volume budget: at most GRID^3 voxels in total, spread over the axes as the scene needs")
    parser.add_argument("--sdf-trunc", type=float, default=4.0, help="TSDF truncation in voxels")
    parser.add_argument("--icp-iters", type=int, default=15)
    parser.add_argument("--icp-stride", type=int, default=2)
    parser.add_argument("--icp-max-dist", type=float, default=0.05)
    parser.add_argument("--depth-scale", type=float, default=1.0, help="metric scale of the depth files")
    parser.add_argument("--anchors", type=str, default=None,
                        help=".npz of sparse metric anchors (p3_<i>: [n,3], p2_<i>: [n,2] per frame i) for relative depth")
    parser.add_argument("--estimate-scale", action="store_true",
                        help="relative depth without anchors: every view's metric scale is estimated inside its registration (Sim(3) "
                             "point-to-plane ICP) and chained with the reference's 0.7 / 0.3 rule (D2R:650); view 0 keeps --depth-scale")
    parser.add_argument("--scale-update-weight", type=float, default=0.3, help="weight of a view's own scale estimate in the running scale")
    parser.add_argument("--tsdf-min-weight", type=int, default=0, help="> 0: keep only voxels the TSDF saw this often")
    parser.add_argument("--ascii", action="store_true", help="write the reference's ASCII fallback PLY instead of binary")
    parser.add_argument("--mesh-output", type=str, default=None,
                        help="also write the marching-cubes triangle mesh of the fused TSDF to this PLY (binary, or ASCII with --ascii)")
    parser.add_argument("--mesh-min-component", type=int, default=0, metavar="N",
                        help="drop the mesh's connected components with fewer than N triangles (needs --mesh-output)")
    parser.add_argument("--mesh-largest-component", action="store_true",
                        help="keep only the mesh's connected component with the most triangles (needs --mesh-output)")
    parser.add_argument("--mesh-simplify-cell", type=float, default=0.0, metavar="M",
                        help="merge the mesh's vertices per cell of M metres (vertex clustering, after the component filter; needs --mesh-output)")
    parser.add_argument("--mesh-simplify-placement", choices=("mean", "quadric"), default="mean",
                        help="where --mesh-simplify-cell puts a merged vertex: at the mean of its members (default), or by quadric error, "
                             "which keeps the creases and corners of planar scenes (needs --mesh-simplify-cell)")
    parser.add_argument("--mesh-smooth", type=int, default=0, metavar="N",
                        help="smooth the mesh with N Taubin iterations (after the component filter and the simplification; needs --mesh-output)")
    parser.add_argument("--mesh-normals", action="store_true",
                        help="write area-weighted vertex normals (nx ny nz) into the mesh PLY (needs --mesh-output)")
    parser.add_argument("--mesh-weld", choices=("host", "device"), default="host",
                        help="where the meshes of a scene fused block by block are welded: in numpy on the host (default), or on the "
                             "GPU, the same bytes (needs --mesh-output)")
    parser.add_argument("--render-output", type=str, default=None,
                        help="also render the fused model at every kept camera into this folder: <stem>_model_depth.npy / .png "
                             "(metres / u16 millimetres) and <stem>_model_color.png (one GPU only)")
    parser.add_argument("--loop-closure", action="store_true",
                        help="find revisits among the registered poses, register them too and optimise every pose over the resulting "
                             "graph before fusing (one GPU only; not with --estimate-scale)")
    parser.add_argument("--model-tracking", action="store_true",
                        help="after the registration, register every kept frame against the TSDF fused from the frames before it "
                             "(point-to-SDF) and fuse at those poses (one GPU only; not with --estimate-scale)")
    parser.add_argument("--compare-to", type=str, default=None, metavar="REF.ply",
                        help="score the fused cloud (and the mesh, with --mesh-output) against the vertices of this PLY on the GPU: prints "
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
                             "cannot see (along a tunnel, across a wall); needs colour images and a single GPU")
    parser.add_argument("--photo-weight", type=float, default=0.1, metavar="W",
                        help="weight of the photometric system beside the geometric one (default 0.1; too small a weight falls under "
                             "the solver's eigenvalue cutoff)")
    parser.add_argument("--photo-gate", type=float, default=0.2, metavar="G",
                        help="largest intensity difference (0..1) of a photometric correspondence (default 0.2)")
    parser.add_argument("--photo-smooth-radius", type=int, default=1, metavar="R",
                        help="the intensity is averaged over (2R+1)^2 pixels on one side of depth edges (0..7; default 1)")
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--stream", dest="stream", action="store_true", default=True,
                        help="(default) decode on worker threads into pinned buffers with asynchronous uploads; host RAM never holds the sequence")
    parser.add_argument("--no-stream", dest="stream", action="store_false",
                        help="decode every frame into host memory first, as the reference does (D2R:434-437)")
    parser.add_argument("--gpus", type=int, default=1,
                        help="one process per GPU: frames shard across ranks, the per-GPU grids are summed with one RCCL all-reduce "
                             "(also honoured under torchrun: RANK / WORLD_SIZE in the environment)")
    args = parser.parse_args(argv)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.render_output and (args.gpus > 1 or world > 1):
        parser.error("--render-output needs a single GPU: with --gpus > 1 rank 0 does not hold the other ranks' frames")
    if (args.mesh_min_component > 0 or args.mesh_largest_component) and not args.mesh_output:
        parser.error("--mesh-min-component / --mesh-largest-component filter the mesh: they need --mesh-output")
    if args.mesh_simplify_cell != 0.0 and not args.mesh_output:
        parser.error("--mesh-simplify-cell simplifies the mesh: it needs --mesh-output")
    if args.mesh_simplify_placement != "mean" and not args.mesh_simplify_cell > 0.0:
        parser.error("--mesh-simplify-placement places the simplified mesh's vertices: it needs --mesh-simplify-cell")
    if (args.mesh_smooth != 0 or args.mesh_normals) and not args.mesh_output:
        parser.error("--mesh-smooth / --mesh-normals work on the mesh: they need --mesh-output")
    if args.mesh_weld != "host" and not args.mesh_output:
        parser.error("--mesh-weld device welds the mesh: it needs --mesh-output")
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
    if args.depth_filter and (args.gpus > 1 or world > 1):
        parser.error("--depth-filter needs a single GPU: the shards upload their frames in several places, and the filter is not wired into them")
    if args.loop_closure and (args.gpus > 1 or world > 1):
        parser.error("--loop-closure needs a single GPU: every kept frame must be resident where the revisits are registered")
    if args.loop_closure and args.estimate_scale:
        parser.error("--loop-closure does not go with --estimate-scale: the pose graph's edges carry no scale")
    if args.model_tracking and (args.gpus > 1 or world > 1):
        parser.error("--model-tracking needs a single GPU: every kept frame is registered against one model, in order")
    if args.model_tracking and args.estimate_scale:
        parser.error("--model-tracking does not go with --estimate-scale: tracking against the model estimates no scale")
    if args.photometric:
        from tl3d.pipeline import check_photometric_options
        try:
            check_photometric_options(argparse.Namespace(photometric=True, photo_weight=args.photo_weight, photo_gate=args.photo_gate,
                                                         photo_smooth_radius=args.photo_smooth_radius, photo_depth_jump=0.05,
                                                         loop_closure=args.loop_closure),
                                      estimate_scale=args.estimate_scale, sharded=args.gpus > 1 or world > 1)
        except ValueError as e:
            parser.error("--photometric: " + str(e))
    if args.gpus > 1 and world == 1:
        return _spawn_ranks(args.gpus, sys.argv[1:] if argv is None else list(argv))
    dist = None
    if world > 1:
        dist = _init_rank(args)

    from tl3d.config import ReconstructionConfig
    from tl3d.pipeline import DepthToReconstructionPipeline

    config = ReconstructionConfig(fx=args.fx, fy=args.fy, cx=args.cx, cy=args.cy, voxel_size=args.voxel_size,
                                  subsample_factor=args.subsample, depth_scale=args.depth_scale, grid_dim=args.grid,
                                  sdf_trunc_voxels=args.sdf_trunc, icp_iters=args.icp_iters, icp_stride=args.icp_stride,
                                  icp_max_dist=args.icp_max_dist, tsdf_min_weight=args.tsdf_min_weight, device=args.device,
                                  scale_update_weight=args.scale_update_weight, extract_mesh=args.mesh_output is not None,
                                  render_dir=args.render_output, loop_closure=args.loop_closure,
                                  model_tracking=args.model_tracking, mesh_min_component_triangles=max(0, args.mesh_min_component),
                                  mesh_largest_component=args.mesh_largest_component, mesh_simplify_cell=args.mesh_simplify_cell,
                                  mesh_simplify_placement=args.mesh_simplify_placement,
                                  mesh_smooth_iterations=args.mesh_smooth, mesh_normals=args.mesh_normals, mesh_weld=args.mesh_weld,
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
                                  compare_align_init=args.compare_align_init, compare_align_global=args.compare_align_global,
                                  compare_align_global_voxel=args.compare_align_global_voxel)
    pipeline = DepthToReconstructionPipeline(config)
    # a rank decodes every frame on its host (pose chain and scale rule run over the whole sequence) and uploads its share
    streaming = args.stream and dist is None
    if dist is not None and dist.get_rank() != 0:
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            num_loaded = pipeline.load_data(args.rgb_folder, args.depth_folder)
    else:
        num_loaded = (pipeline.load_data_streaming if streaming else pipeline.load_data)(args.rgb_folder, args.depth_folder)
    if num_loaded < 2:
        if dist is None or dist.get_rank() == 0:
            print("Failed to load sufficient data")
        if dist is not None:
            dist.destroy_process_group()
        return 0
    anchors = None
    if args.anchors:
        import numpy as np
        z = np.load(args.anchors)
        anchors = {int(k[3:]): (z[k], z["p2_" + k[3:]]) for k in z.files if k.startswith("p3_")}
    if dist is not None:
        points, colors, poses = pipeline.reconstruct_sharded(dist, anchors=anchors, estimate_scale=args.estimate_scale)
        rank = dist.get_rank()
        dist.barrier()
        dist.destroy_process_group()
        if rank != 0:                                   # rank 0 holds the merged cloud and writes the file
            return 0
    else:
        points, colors, poses = pipeline.reconstruct(anchors=anchors, estimate_scale=args.estimate_scale)
    if points is not None and len(points) > 0:
        pipeline.save_reconstruction(points, colors, args.output, ascii=args.ascii, normals=pipeline.cloud_normals,
                                     curvature=pipeline.cloud_curvature, planes=pipeline.cloud_plane_ids)
        if args.cloud_planes_report:
            from tl3d import fileio
            fileio.write_plane_report(args.cloud_planes_report, pipeline.cloud_planes)
        if args.mesh_output:
            pipeline.save_mesh(args.mesh_output, ascii=args.ascii)
        if not args.no_vis:
            print("(interactive Plotly viewer of the reference is not part of the device path; pass --no-vis to silence)")
    else:
        print("Reconstruction failed")
    return 0


if __name__ == "__main__":
    sys.exit(main())
