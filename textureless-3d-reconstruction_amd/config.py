"""Configuration objects with the reference's names and defaults.

ReconstructionConfig mirrors depth_to_reconstruction.py:45-73; CameraIntrinsics mirrors
depth_enhanced_reconstruction.py:57-80.  Fields the SfM front end used (match_ratio,
ransac_threshold) are kept so existing call sites keep constructing the object; the
additive fields at the end configure the device grid and the ICP pose source.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np


@dataclass
class ReconstructionConfig:
    # camera intrinsics (D2R:49-52)
    fx: float = 1719.0
    fy: float = 1719.0
    cx: float = 540.0
    cy: float = 960.0
    # depth processing (D2R:55-57)
    depth_scale: float = 1.0
    min_depth: float = 0.1
    max_depth: float = 50.0
    # feature matching (D2R:60-61) -- unused by the ICP pose source, kept for signature compatibility
    match_ratio: float = 0.75
    ransac_threshold: float = 3.0
    # point cloud (D2R:64-65)
    voxel_size: float = 0.005
    subsample_factor: int = 2

    # ---- additive: device fusion ------------------------------------------------------------------
    grid_dim: int = 1024                # fusion volume budget: at most grid_dim^3 voxels IN TOTAL, spread over the axes as
                                        # the scene needs (a corridor gets 400 x 480 x 2500, not a clipped cube)
    sdf_trunc_voxels: float = 4.0       # TSDF truncation in voxels
    icp_coarse: tuple = ((10, 4, 0.20),)   # levels before the final one: (iterations, pixel stride, gate in metres)
    icp_iters: int = 15
    icp_stride: int = 2
    icp_max_dist: float = 0.05
    icp_damping: float = 1e-6
    icp_eps: float = 1e-7               # a level stops once the largest component of its pose update is below this (rad / m)
    icp_eig_rel: float = 1e-4           # relative eigenvalue cutoff: unobservable DOFs keep the motion prior
    icp_smooth_radius: int = 1          # normals (and the registration's source depth) from the depth averaged over a (2 r + 1)^2 window; 0 = raw
    scale_update_weight: float = 0.3    # estimate_scale runs: avg = (1 - w) avg + w scale_i (D2R:650 uses 0.3); 1 = each view's own estimate
    tsdf_min_weight: int = 0            # > 0: gate the emitted centroids by the TSDF (outlier suppression)
    tsdf_max_abs: float = 1.0
    # statistical outlier removal after the voxel merge: D2R's merge_pointclouds runs it (20 neighbours, 2 sigma,
    # D2R:412-415); DER's merge_pointclouds has none (DER:615-645) -- the DER command line switches it off
    outlier_filter: bool = True
    outlier_nb_neighbors: int = 20
    outlier_std_ratio: float = 2.0
    device: int = 0
    # marching-cubes mesh of the TSDF after the fusion (DepthToReconstructionPipeline.mesh / save_mesh)
    extract_mesh: bool = False
    # drop the mesh's small connected components (both need extract_mesh): components with fewer
    # triangles than this go (0: none does), and / or only the component with the most triangles stays
    mesh_min_component_triangles: int = 0
    mesh_largest_component: bool = False
    # vertex-clustering simplification of the mesh (needs extract_mesh): the vertices of one cell of this
    # size, in metres, become one vertex (0: off); applied after the component filter when both are on
    mesh_simplify_cell: float = 0.0
    # where a merged vertex is put: "mean" (of its members), or "quadric" (where the planes of the triangles around it meet: keeps
    # creases and corners of planar scenes, gains nothing on smooth surfaces; needs mesh_simplify_cell > 0).  Smoothing afterwards
    # (mesh_smooth_iterations) rounds the creases again.
    mesh_simplify_placement: str = "mean"
    # Taubin smoothing of the mesh's positions and area-weighted vertex normals (all need extract_mesh):
    # iterations of a step with lambda and a step with mu (0: off), after the component filter and the simplification; the normals
    # (DepthToReconstructionPipeline.mesh_normals, written by save_mesh) come last, from the final positions
    mesh_smooth_iterations: int = 0
    mesh_smooth_lambda: float = 0.5
    mesh_smooth_mu: float = -0.53
    mesh_normals: bool = False
    # where the meshes of a blocked run's blocks are welded ("device" needs extract_mesh): "host" is
    # lattice.weld_meshes (numpy), "device" FusionContext.weld_meshes, the same bytes.  No effect on a run of one block (nothing to
    # weld) or in reconstruct_sharded (never blocked).
    mesh_weld: str = "host"
    # folder for renders of the fused model at every kept camera (DepthToReconstructionPipeline.reconstruct)
    render_dir: Optional[str] = None
    # loop closure: revisits found from the chain's poses, registered with the same ICP, and every pose
    # optimised over the resulting graph before bounding and fusing.  Off: nothing changes.
    loop_closure: bool = False
    loop_min_gap: int = 30              # kept frames between the two ends of a candidate
    loop_max_dist: float = 0.3          # metres between the camera centres, at the chain's poses
    loop_max_angle_deg: float = 20.0    # between the view axes
    loop_edges_per_frame: int = 2       # candidates registered per (later) frame: the best by correspondences
    loop_min_fitness: float = 0.5       # of a candidate at the chain-relative pose, and of a closure at its registered pose
    loop_max_residual: float = 0.05     # metres of residual translation at the optimum above which a closure is dropped
    # model tracking: after the chain (and the loop closure), every kept frame is registered against the
    # TSDF fused from the frames before it (point-to-SDF) and its pose replaces the chain's.  Off: nothing changes.
    model_tracking: bool = False
    track_voxel_size: Optional[float] = None   # voxel of the tracking grid; None: voxel_size.  Doubled until the grid is one block and fits in memory
    track_margin: float = 0.05          # metres added around the bounds of the frames at the chain's poses
    track_min_weight: int = 1           # a voxel takes part once this many frames saw it
    track_min_fitness: float = 0.5      # below it (or with status 2) a frame is lost: it keeps the chain-relative pose
    track_levels: Optional[tuple] = None   # ((iterations, stride, gate in metres), ...) coarse to fine; None: the chain's levels
    # score the result against a reference scan: a PLY file whose vertices are the reference cloud.  After
    # reconstruct() stats["compare"] holds metrics.compare_clouds(fused cloud, reference) -- Chamfer, precision / recall / F-score at
    # the thresholds (metres) -- and, with extract_mesh, metrics.compare_cloud_to_mesh(reference, final mesh) under "mesh".
    # compare_max_dist: points with no neighbour within it count as unmatched.  None: nothing changes.
    compare_to: Optional[str] = None
    compare_thresholds: tuple = (0.005, 0.01, 0.02)
    compare_max_dist: Optional[float] = None
    # compare_align: a reference scan is never in the reconstruction's frame (the first camera's), so the
    # fused cloud is first registered onto it on the GPU (FusionContext.register_clouds: point-to-plane ICP against the scan's
    # unoriented normals, the frame ICP's gate schedule) and the cloud, and the mesh's vertices for the mesh comparison, are moved by
    # the result before they are scored; the written files are not moved.  stats["compare"]["alignment"] = {T, scale, fitness, rmse,
    # n_corr, iters_run, status}.  A local method: a scan further than a gate (20 cm) away needs compare_align_init, a 4 x 4
    # matrix (or a .npy / text file of one) mapping reconstruction to scan.  compare_align_scale also estimates the scale (a
    # reconstruction from relative depth is not in the scan's units); it needs a closed or bounded scene -- open geometry (a wall, a
    # corner) observes the scale weakly and the estimate can collapse.  Needs compare_to.  Off: nothing changes.
    compare_align: bool = False
    compare_align_scale: bool = False
    compare_align_init: Optional[object] = None
    # compare_align_global: the registration's start comes from the global front end on the GPU
    # (metrics.global_align_clouds: voxel subsample, FPFH, mutual nearest features, RANSAC), so the scan may lie ANYWHERE: no
    # compare_align_init is needed, and none may be given with it.  compare_align_global_voxel: the subsampling voxel in metres
    # (None: 5 x voxel_size).  stats["compare"]["alignment"]["global"] = {T, inliers, n_corr, n_passed, hypotheses, voxel, mutual}.
    # Rigid only: refused together with compare_align_scale (the RANSAC's edge-length test assumes one scale).  Needs geometric
    # features: on a single plane or a bare wall no sample passes and the local method starts from the identity as before.
    # Needs compare_align.  Off: nothing changes.
    compare_align_global: bool = False
    compare_align_global_voxel: Optional[float] = None
    # normals (and surface variation) of the fused cloud: PCA over each point's cloud_normals_neighbors
    # nearest neighbours (Open3D's max_nn), none further than cloud_normals_radius metres (0: no limit), turned towards the nearest
    # kept camera; once over the whole cloud, after the outlier filter.  DepthToReconstructionPipeline.cloud_normals /
    # .cloud_curvature, written by save_reconstruction as nx ny nz / curvature.  cloud_curvature needs cloud_normals.  Off: nothing changes.
    cloud_normals: bool = False
    cloud_normals_neighbors: int = 30
    cloud_normals_radius: float = 0.0
    cloud_curvature: bool = False
    # planar regions of the cloud with normals: points are linked within cloud_planes_radius when their normals
    # lie within cloud_planes_angle_deg and each within cloud_planes_offset of the other's tangent plane; points with a surface
    # variation above cloud_planes_max_curvature (0: no bound) take no part; a region of at least cloud_planes_min_points points whose
    # plane fits with rms <= cloud_planes_max_rms is a plane.  A length of 0 means 2.5 voxels (radius), 1 voxel (offset), 0.5 voxel (rms).
    # DepthToReconstructionPipeline.cloud_plane_ids / .cloud_planes, written by save_reconstruction as `plane`.  Needs cloud_normals.
    # Off: nothing changes.
    cloud_planes: bool = False
    cloud_planes_radius: float = 0.0
    cloud_planes_angle_deg: float = 10.0
    cloud_planes_offset: float = 0.0
    cloud_planes_max_curvature: float = 0.05
    cloud_planes_min_points: int = 200
    cloud_planes_max_rms: float = 0.0
    # depth-frame filter: once over all resident frames, behind the upload and the per-frame scales and in
    # front of the registration, so everything downstream reads the filtered frames.  Two valid pixels (finite, > 0) are linked when
    # their depths differ by at most depth_filter_jump times the smaller one; a pixel with fewer than depth_filter_min_support
    # linked pixels in its (2 depth_filter_radius + 1)^2 window is set to 0 (flying pixels), then every 4-connected region of
    # linked survivors smaller than depth_filter_min_region (0: no such stage).  Pixels are only invalidated, never altered.
    # stats["depth_filter"].  Not on a sharded run.  Off: nothing changes.
    depth_filter: bool = False
    depth_filter_jump: float = 0.05
    depth_filter_radius: int = 1
    depth_filter_min_support: int = 4
    depth_filter_min_region: int = 0
    # photometric term in the frame-to-frame registration: beside the point-to-plane residual every
    # correspondence contributes the difference of the smoothed intensities of its two pixels, which observes the in-surface motion
    # geometry cannot (a tube's axis, a wall's plane).  The joint system is A_g + photo_weight A_p; a weight too small leaves the
    # photometric directions under icp_eig_rel (0.01 does on the open tube).  photo_gate bounds |r_I| (intensities in 0..1);
    # the intensity is averaged over a (2 photo_smooth_radius + 1)^2 window of pixels linked by photo_depth_jump (the depth filter's
    # rule).  Needs colour with every frame; not with estimate_scale, loop_closure or a sharded run.  icp_log entries and
    # stats["photometric"] carry n_photo and the photometric rmse.  Off: nothing changes.
    photometric: bool = False
    photo_weight: float = 0.1
    photo_gate: float = 0.2
    photo_smooth_radius: int = 1
    photo_depth_jump: float = 0.05

    @property
    def K(self) -> np.ndarray:
        return np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]], dtype=np.float64)


@dataclass
class CameraIntrinsics:
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int

    def to_matrix(self) -> np.ndarray:
        return np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]], dtype=np.float64)

    @classmethod
    def from_matrix(cls, K: np.ndarray, width: int, height: int) -> "CameraIntrinsics":
        return cls(fx=float(K[0, 0]), fy=float(K[1, 1]), cx=float(K[0, 2]), cy=float(K[1, 2]),
                   width=int(width), height=int(height))
