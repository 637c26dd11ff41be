"""Surface distances between what the pipeline produces and a reference scan, on the GPU: cloud to cloud
(Chamfer, precision / recall / F-score at thresholds) and cloud to mesh.  Everything goes through FusionContext.nearest_points /
nearest_triangles / distance_summary; nothing here imports the oracle."""
from __future__ import annotations


def _side(ctx, dist, thresholds):
    s = ctx.distance_summary(dist, thresholds)
    return dict(n=s["n"], within=s["within"], mean=s["mean"], rms=s["rms"], max=s["max"], below=s["below"])


def _rates(a_side, b_side, thresholds):
    out = []
    for j, t in enumerate(thresholds):
        p = a_side["below"][j] / a_side["n"] if a_side["n"] else float("nan")
        r = b_side["below"][j] / b_side["n"] if b_side["n"] else float("nan")
        out.append(dict(threshold=float(t), precision=p, recall=r, fscore=2 * p * r / (p + r) if p + r > 0 else 0.0))
    return out


def compare_clouds(ctx, a, b, thresholds=(), max_dist=None) -> dict:
    """Distances from every point of cloud a to its nearest point of cloud b and back.  a_to_b / b_to_a: {n, within (points with a
    neighbour inside max_dist), mean, rms, max over those, below (per threshold the points with distance <= it)};
    chamfer_mean = 0.5 * (mean_ab + mean_ba); at: per threshold {threshold, precision = the share of a within it of b,
    recall = the share of b within it of a, fscore = their harmonic mean}.  a, b: numpy arrays or device tensors, [n, 3]."""
    thresholds = tuple(float(t) for t in thresholds)
    d_ab, _ = ctx.nearest_points(a, b, max_dist=max_dist)
    d_ba, _ = ctx.nearest_points(b, a, max_dist=max_dist)
    ab, ba = _side(ctx, d_ab, thresholds), _side(ctx, d_ba, thresholds)
    return dict(a_to_b=ab, b_to_a=ba, chamfer_mean=0.5 * (ab["mean"] + ba["mean"]), at=_rates(ab, ba, thresholds))


def compare_cloud_to_mesh(ctx, points, xyz, tris, thresholds=(), max_dist=None) -> dict:
    """A cloud against a triangle mesh: points_to_surface, every point to the nearest point of the mesh's surface
    (nearest_triangles), and vertices_to_points, every mesh vertex to its nearest point of the cloud (nearest_points); the sides as
    compare_clouds gives them.  at: per threshold precision = the share of the mesh's vertices within it of the cloud, recall = the
    share of the cloud within it of the surface, and fscore."""
    thresholds = tuple(float(t) for t in thresholds)
    d_ps, _ = ctx.nearest_triangles(points, xyz, tris, max_dist=max_dist)
    d_vp, _ = ctx.nearest_points(xyz, points, max_dist=max_dist)
    ps, vp = _side(ctx, d_ps, thresholds), _side(ctx, d_vp, thresholds)
    return dict(points_to_surface=ps, vertices_to_points=vp, at=_rates(vp, ps, thresholds))


def move_points(points, T, scale=1.0):
    """scale * R p + t for every point, on the host in fp64, rounded to float32 once."""
    import numpy as np
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    return (float(scale) * (p @ T[:3, :3].T) + T[:3, 3]).astype(np.float32)


def align_clouds(ctx, a, b, b_normals=None, **kw):
    """Register cloud a onto cloud b (FusionContext.register_clouds; kw: T_init, scale_init, levels, estimate_scale, cell_size) and
    return (the result, a moved into b's frame: scale * R a + t, float32 on the host).  A local method: a must start within a gate
    of b (T_init); estimate_scale needs a closed or bounded scene."""
    res = ctx.register_clouds(a, b, b_normals, **kw)
    if hasattr(a, "data_ptr"):
        a = a.detach().cpu().numpy()
    return res, move_points(a, res["T"], res["scale"])


def format_alignment(al: dict) -> str:
    """One line for the drivers, beside format_line."""
    t = al["T"][:3, 3] if hasattr(al["T"], "shape") else [row[3] for row in al["T"][:3]]
    return (f"Align: status {al['status']}, {al['iters_run']} iterations, fitness {al['fitness']:.4f}, rmse {al['rmse']:.6g} m, "
            f"scale {al['scale']:.6g}, t ({t[0]:.4f}, {t[1]:.4f}, {t[2]:.4f})")


def format_line(cmp: dict) -> str:
    """One line for the drivers: Chamfer and the F-scores."""
    parts = [f"chamfer {cmp['chamfer_mean']:.6g} m"]
    parts += [f"F@{r['threshold']:g} {r['fscore']:.4f} (P {r['precision']:.4f} R {r['recall']:.4f})" for r in cmp["at"]]
    return "Compare: " + ", ".join(parts)
