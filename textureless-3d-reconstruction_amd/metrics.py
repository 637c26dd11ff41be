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


def _host_points(a):
    import numpy as np
    if hasattr(a, "data_ptr"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


def global_align_clouds(ctx, a, b, voxel, nb_neighbors=48, feature_radius=None, normal_neighbors=30, max_dist=None,
                        hypotheses=100_000, seed=0, mutual=True) -> dict:
    """A pose of cloud a in cloud b's frame from ANY start: the standard global front end, every stage on the
    GPU.  In order: (1) voxel_subsample both clouds at `voxel`; (2) estimate_normals of each subsample (normal_neighbors, within
    feature_radius) with the subsample's own fp64 centroid as the one viewpoint; (3) compute_fpfh (nb_neighbors within
    feature_radius, default 5 voxels); (4) match_features both ways; (5) keep the pairs that choose each other, or with mutual off,
    or when fewer than 3 % of a's points have such a partner, all pairs a -> b; (6) ransac_register (max_dist default 1.5 voxels).
    The normals are estimated here, not taken from the caller, because the pair feature depends on each normal's SIGN, so both
    clouds need one orientation rule that moves with the cloud: "towards the cloud's own centroid" is a function of the point set
    alone, while normals turned towards a sensor, or signed arbitrarily, are not.
    Returns ransac_register's dict (T, status, best_h, inliers, n_passed, m) with n_a and n_b (points after subsampling), n_corr,
    n_mutual, mutual (whether the mutual pairs were used), hypotheses and voxel beside it.  status 2 and T = identity: no sample of
    three correspondences kept its edge lengths -- a scene without geometric features (a single plane, a bare corridor wall) gives
    the features nothing to tell its points apart by; symmetric objects have several answers; partial overlap moves the centroid
    rule; rigid only (one scale)."""
    import numpy as np
    voxel = float(voxel)
    radius = float(feature_radius) if feature_radius is not None else 5.0 * voxel
    gate = float(max_dist) if max_dist is not None else 1.5 * voxel
    feats, pts = [], []
    for cloud in (a, b):
        p = _host_points(cloud)
        p = p[ctx.voxel_subsample(p, voxel)]
        if len(p) >= 3:
            c = p.astype(np.float64).mean(axis=0)
            nrm = ctx.estimate_normals(p, nb_neighbors=int(normal_neighbors), max_radius=radius, viewpoints=c[None], cell_size=radius / 2)
            f = ctx.compute_fpfh(p, nrm, nb_neighbors=int(nb_neighbors), max_radius=radius, cell_size=radius / 2)
        else:
            f = np.zeros((len(p), 33), np.float32)
        pts.append(p)
        feats.append(f)
    ab = ctx.match_features(feats[0], feats[1])
    ba = ctx.match_features(feats[1], feats[0])
    ia = np.arange(len(ab), dtype=np.int32)
    has = ab >= 0
    is_mutual = has.copy()
    is_mutual[has] = ba[ab[has]] == ia[has]
    n_mutual = int(is_mutual.sum())
    use_mutual = bool(mutual) and n_mutual >= 0.03 * len(ab)
    keep = is_mutual if use_mutual else has
    corr = np.ascontiguousarray(np.stack([ia[keep], ab[keep]], axis=1), dtype=np.int32)
    res = ctx.ransac_register(pts[0], pts[1], corr, hypotheses=hypotheses, max_dist=gate, seed=seed)
    res.update(n_a=len(pts[0]), n_b=len(pts[1]), n_corr=len(corr), n_mutual=n_mutual, mutual=use_mutual, hypotheses=int(hypotheses),
               voxel=voxel)
    return res


def align_clouds(ctx, a, b, b_normals=None, global_kw=None, **kw):
    """Register cloud a onto cloud b (FusionContext.register_clouds; kw: T_init, scale_init, levels, estimate_scale, cell_size) and
    return (the result, a moved into b's frame: scale * R a + t, float32 on the host).  A local method: a must start within a gate
    of b (T_init); estimate_scale needs a closed or bounded scene.  T_init="global": the start comes from global_align_clouds
    (global_kw: its keywords; `voxel` is required), whose dict is returned as the result's "global" entry."""
    glob = None
    if isinstance(kw.get("T_init"), str):
        assert kw["T_init"] == "global", f"T_init {kw['T_init']!r}: a 4 x 4 matrix or \"global\""
        assert global_kw and "voxel" in global_kw, "T_init=\"global\" needs global_kw with a voxel"
        glob = global_align_clouds(ctx, a, b, **global_kw)
        kw = dict(kw, T_init=glob["T"])
    res = ctx.register_clouds(a, b, b_normals, **kw)
    if glob is not None:
        res["global"] = glob
    if hasattr(a, "data_ptr"):
        a = a.detach().cpu().numpy()
    return res, move_points(a, res["T"], res["scale"])


def format_alignment(al: dict) -> str:
    """One line for the drivers, beside format_line."""
    t = al["T"][:3, 3] if hasattr(al["T"], "shape") else [row[3] for row in al["T"][:3]]
    start = ""
    if "global" in al:
        g = al["global"]
        start = f"global start ({g['inliers']} of {g['n_corr']} feature pairs, {g['n_passed']} of {g['hypotheses']} samples scored), "
    return (f"Align: {start}status {al['status']}, {al['iters_run']} iterations, fitness {al['fitness']:.4f}, rmse {al['rmse']:.6g} m, "
            f"scale {al['scale']:.6g}, t ({t[0]:.4f}, {t[1]:.4f}, {t[2]:.4f})")


def format_line(cmp: dict) -> str:
    """One line for the drivers: Chamfer and the F-scores."""
    parts = [f"chamfer {cmp['chamfer_mean']:.6g} m"]
    parts += [f"F@{r['threshold']:g} {r['fscore']:.4f} (P {r['precision']:.4f} R {r['recall']:.4f})" for r in cmp["at"]]
    return "Compare: " + ", ".join(parts)
