"""Where the two placements of the mesh simplification put their vertices (DESIGN.md sections 4.2.2 and 7.7).

Renders 12 VGA frames down synth.py's rectangular corridor (config 3; the shape of the block tests: 2 cm voxels, subsample 2),
fuses and meshes them, simplifies the mesh at a cell of --cell-voxels voxels with mean and with quadric placement, and prints, per
placement, the mean and the largest distance of the output vertices to the analytic surface (the room's box and the two spheres),
for all vertices and for those within one cell of an edge of the box (a wall / floor, wall / ceiling or end-wall crease).
Vertices of clusters no triangle names are left out (they are no part of the surface).  The same four figures for the
centroids of the output triangles: a vertex can lie on a wall while the triangle it ends cuts the corner.  One JSON line per
placement.

    python tools/mesh_simplify_quality.py [--cell-voxels 4] [--frames 12]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell-voxels", type=float, default=4.0)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--voxel", type=float, default=0.02)
    args = ap.parse_args()
    import numpy as np
    from tl3d import synth
    from tl3d.config import ReconstructionConfig
    from tl3d.pipeline import DepthToReconstructionPipeline

    W, H = 640, 480
    cam = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0)
    scene = synth.corridor_scene()
    poses = synth.dolly_poses(args.frames, (0.0, 0.0, 0.0), (0.0, 0.0, 0.1))
    frames = [synth.render(scene, p, W, H, **cam) for p in poses]
    lo, hi = (np.array(v, np.float64) for v in scene.room)
    cell = args.cell_voxels * args.voxel

    def to_box(p):
        """distance to the box's boundary, from inside or outside"""
        inside = np.minimum(p - lo, hi - p).min(axis=1)
        outside = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0.0), axis=1)
        return np.where(inside >= 0.0, inside, outside)

    def to_surface(p):
        d = to_box(p)
        for c, r in scene.spheres:
            d = np.minimum(d, np.abs(np.linalg.norm(p - np.array(c), axis=1) - r))
        return d

    def to_edges(p):
        """distance to the nearest of the box's 12 edges: the two smallest of the three distances to the planes' pairs"""
        q = np.clip(p, lo, hi)
        gap = np.sort(np.minimum(np.abs(q - lo), np.abs(q - hi)), axis=1)[:, :2]         # along the two nearest axes
        return np.sqrt((gap ** 2).sum(axis=1) + ((p - q) ** 2).sum(axis=1))

    for placement in ("mean", "quadric"):
        cfg = ReconstructionConfig(**cam, voxel_size=args.voxel, subsample_factor=2, grid_dim=512, outlier_filter=False, extract_mesh=True,
                                   mesh_simplify_cell=cell, mesh_simplify_placement=placement)
        pipe = DepthToReconstructionPipeline(cfg)
        pipe.set_frames([c for d, c in frames], [d for d, c in frames])
        with open(os.devnull, "w") as null:
            out, sys.stdout = sys.stdout, null
            try:
                pipe.reconstruct(poses=poses)
            finally:
                sys.stdout = out
        xyz, _, tris = pipe.mesh
        used = np.zeros(len(xyz), bool)
        used[np.asarray(tris, np.int64).reshape(-1)] = True
        p = np.asarray(xyz, np.float64)[used]
        d, near = to_surface(p), to_edges(p) <= cell
        row = dict(placement=placement, cell_m=cell, voxel_m=args.voxel, frames=args.frames, vertices=int(len(xyz)), vertices_on_triangles=int(used.sum()),
                   triangles=int(len(tris)), mean_dist_mm=round(1e3 * float(d.mean()), 3), max_dist_mm=round(1e3 * float(d.max()), 3),
                   near_crease_vertices=int(near.sum()), near_crease_mean_dist_mm=round(1e3 * float(d[near].mean()), 3),
                   near_crease_max_dist_mm=round(1e3 * float(d[near].max()), 3),
                   near_crease_mean_dist_to_edge_mm=round(1e3 * float(to_edges(p)[near].mean()), 3))
        c = np.asarray(xyz, np.float64)[np.asarray(tris, np.int64)].mean(axis=1)
        dc, cnear = to_surface(c), to_edges(c) <= cell
        row.update(centroid_mean_dist_mm=round(1e3 * float(dc.mean()), 3), centroid_max_dist_mm=round(1e3 * float(dc.max()), 3),
                   near_crease_centroids=int(cnear.sum()), near_crease_centroid_mean_dist_mm=round(1e3 * float(dc[cnear].mean()), 3),
                   near_crease_centroid_max_dist_mm=round(1e3 * float(dc[cnear].max()), 3))
        row.update({k: v for k, v in pipe.stats["mesh_simplify"].items() if k in ("quadric_placed", "clamped", "corners_skipped")})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
