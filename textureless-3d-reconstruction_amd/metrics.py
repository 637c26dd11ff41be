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


def format_line(cmp: dict) -> str:
    """One line for the drivers: Chamfer and the F-scores."""
    parts = [f"chamfer {cmp['chamfer_mean']:.6g} m"]
    parts += [f"F@{r['threshold']:g} {r['fscore']:.4f} (P {r['precision']:.4f} R {r['recall']:.4f})" for r in cmp["at"]]
    return "Compare: " + ", ".join(parts)
