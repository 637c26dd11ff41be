"""numpy restatement of the cloud registration's contract (include/tl3d.h at tl3d_cloud_evaluate), the
reference of tests/test_gpu_cloud_register.py; tests/test_cloud_register_reference_cpu.py holds it to finite differences, to
cKDTree and to planted poses.  Elementwise fp64 expressions in the contract's order, no matmul: every TERM of a sum is the value the
kernels compute, bit for bit; only the order of the additions is free, so the sums are returned correctly rounded (math.fsum)
together with sum |term|, which prices any other order:  |any order - fsum| <= n_terms * 2^-52 * sum |term|  (n - 1 roundings of
at most 2^-53 of a partial sum that never exceeds sum |term|, and fsum's own)."""
import math

import numpy as np

UPPER = [(i, j) for i in range(7) for j in range(i, 7)]           # tl3d_cloud_eval::A: the upper triangle, row-major


def transform(src, T, scale):
    """(w, q) of every source point: m = R p, w = scale * m, q = w + t."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(src, np.float32).astype(np.float64).reshape(-1, 3)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    w = np.empty_like(p)
    q = np.empty_like(p)
    for a in range(3):
        m = (T[a, 0] * px + T[a, 1] * py) + T[a, 2] * pz
        w[:, a] = np.float64(scale) * m
        q[:, a] = w[:, a] + T[a, 3]
    return w, q


def nearest_brute(q, tgt, chunk=256):
    """(d2, index) minimising the pair (d2, index) over the target, by fp64 brute force: d = y - q, d2 = (dx dx + dy dy) + dz dz;
    argmin returns the first minimum, which is the smaller index of an exact tie."""
    t = np.asarray(tgt, np.float32).astype(np.float64).reshape(-1, 3)
    idx = np.empty(len(q), np.int64)
    d2 = np.empty(len(q))
    for s in range(0, len(q), chunk):
        qq = q[s:s + chunk]
        dx, dy, dz = (t[None, :, a] - qq[:, None, a] for a in range(3))
        dd = (dx * dx + dy * dy) + dz * dz
        i = np.argmin(dd, axis=1)
        idx[s:s + chunk] = i
        d2[s:s + chunk] = dd[np.arange(len(qq)), i]
    return d2, idx


def nearest_kdtree(q, tgt):
    """The same from scipy's cKDTree (no tie rule: for inputs without exact ties); d2 is recomputed in the contract's order."""
    from scipy.spatial import cKDTree
    t = np.asarray(tgt, np.float32).astype(np.float64).reshape(-1, 3)
    _, idx = cKDTree(t).query(q, k=1)
    dx, dy, dz = (t[idx, a] - q[:, a] for a in range(3))
    return (dx * dx + dy * dy) + dz * dz, idx.astype(np.int64)


def rows(n, e, q, w, with_scale):
    """r [m] and J [m, 7] of one row per correspondence: r = n . e, J = [q x n, n, n . w]."""
    r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
    J = np.zeros((len(r), 7))
    J[:, 0] = q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1]
    J[:, 1] = q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2]
    J[:, 2] = q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0]
    J[:, 3:6] = n
    if with_scale:
        J[:, 6] = (n[:, 0] * w[:, 0] + n[:, 1] * w[:, 1]) + n[:, 2] * w[:, 2]
    return r, J


def _fsum_abs(terms):
    return math.fsum(terms.tolist()), math.fsum(np.abs(terms).tolist())


def evaluate(src, tgt, normals=None, T=np.eye(4), scale=1.0, stride=1, max_dist=0.05, with_scale=False, nearest=nearest_brute):
    """One pass.  A [28], b [7], e: correctly rounded sums; A_abs, b_abs, e_abs: sum |term|; n_rows: terms per sum; index int32
    [n_src]; the counts."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    n = len(src)
    sampled = np.arange(0, n, stride)
    index = np.full(n, -1, np.int32)
    out = dict(A=np.zeros(28), b=np.zeros(7), e=0.0, A_abs=np.zeros(28), b_abs=np.zeros(7), e_abs=0.0, n_rows=0, n_corr=0,
               n_src=len(sampled), n_no_normal=0, index=index)
    if len(tgt) == 0 or len(sampled) == 0:
        return out
    w, q = transform(src[sampled], T, scale)
    d2, idx = nearest(q, tgt)
    keep = np.sqrt(d2) <= (max_dist if max_dist is not None and max_dist > 0 else np.inf)
    index[sampled[keep]] = idx[keep]
    w, q, idx = w[keep], q[keep], idx[keep]
    e = q - tgt[idx].astype(np.float64)
    if normals is not None:
        nn = np.asarray(normals, np.float32).reshape(-1, 3)[idx].astype(np.float64)
        has = ~np.all(nn == 0.0, axis=1)
        out["n_no_normal"] = int((~has).sum())
        out["n_corr"] = int(has.sum())
        r, J = rows(nn[has], e[has], q[has], w[has], with_scale)
    else:
        out["n_corr"] = len(e)
        parts = [rows(np.tile(np.eye(3)[a], (len(e), 1)), e, q, w, with_scale) for a in range(3)]
        r = np.concatenate([p[0] for p in parts])
        J = np.concatenate([p[1] for p in parts])
    out["n_rows"] = len(r)
    for k, (i, j) in enumerate(UPPER):
        out["A"][k], out["A_abs"][k] = _fsum_abs(J[:, i] * J[:, j])
    for i in range(7):
        out["b"][i], out["b_abs"][i] = _fsum_abs(J[:, i] * r)
    out["e"], out["e_abs"] = _fsum_abs(r * r)
    return out


def full(A28):
    A = np.zeros((7, 7))
    for k, (i, j) in enumerate(UPPER):
        A[i, j] = A[j, i] = A28[k]
    return A


def solve(A28, b7, k, damping, eig_rel):
    """x [7] (x[6] = 0 for k = 6) of (A + damping tr(A) / k I) x = -b over the eigen-directions with eigenvalue > eig_rel * largest,
    and the number kept; None when nothing is solvable."""
    A = full(A28)[:k, :k]
    tr = float(np.trace(A))
    if not tr > 0.0:
        return None, 0
    lam, V = np.linalg.eigh(A + damping * (tr / k) * np.eye(k))
    lmax = lam.max()
    if not lmax > 0.0:
        return None, 0
    keep = (lam > eig_rel * lmax) & (lam > 0.0)
    if not keep.any():
        return None, 0
    x = np.zeros(7)
    for e in np.nonzero(keep)[0]:
        x[:k] += -(V[:, e] @ b7[:k]) / lam[e] * V[:, e]
    return x, int(keep.sum())


def se3_apply(x, T):
    """T <- exp(x) T as reg_solve.h's se3_apply has it: x = (w, v), the rotation is Rodrigues' exp([w]x) and v is ADDED to the
    rotated translation (the update is dR T + [0 v], not the screw motion of the se(3) exponential)."""
    wx, wy, wz = x[0], x[1], x[2]
    th2 = wx * wx + wy * wy + wz * wz
    th = math.sqrt(th2)
    a, bq = (1.0, 0.5) if th < 1e-12 else (math.sin(th) / th, (1.0 - math.cos(th)) / th2)
    K = np.array([[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]], np.float64)
    dR = np.eye(3) + a * K + bq * (K @ K)
    Tn = np.eye(4)
    Tn[:3, :] = dR @ np.asarray(T, np.float64)[:3, :]
    Tn[:3, 3] += x[3:6]
    return Tn


DEFAULTS = dict(iters=10, stride=1, max_dist=0.05, damping=1e-6, eps=1e-9, eig_rel=1e-4, estimate_scale=False)
DEFAULT_LEVELS = (dict(iters=10, stride=4, max_dist=0.20), dict(iters=15, stride=1, max_dist=0.05))


def register(src, tgt, normals=None, T_init=np.eye(4), scale_init=1.0, levels=DEFAULT_LEVELS, estimate_scale=False, nearest=nearest_brute):
    """The run of tl3d_cloud_register, level by level with the rules of the step kernel.  The dict of icp(), plus kept: the eigen-
    directions each solve kept."""
    T, s = np.array(T_init, np.float64).reshape(4, 4), float(scale_init)
    kept = []
    E, status, iters_run = None, 0, 0
    for li, level in enumerate(levels):
        lv = dict(DEFAULTS, estimate_scale=estimate_scale)
        lv.update(level)
        k = 7 if lv["estimate_scale"] else 6
        done, status, iters_run = False, 0, 0
        for _ in range(lv["iters"]):
            if done:
                break
            E = evaluate(src, tgt, normals, T, s, lv["stride"], lv["max_dist"], k == 7, nearest)
            x = None
            if E["n_corr"] >= 6:
                x, nk = solve(E["A"], E["b"], k, lv["damping"], lv["eig_rel"])
            if x is None:
                done, status = True, 2
                break
            kept.append(nk)
            T = se3_apply(x, T)
            s = s * math.exp(x[6])
            iters_run += 1
            if np.abs(x).max() < lv["eps"]:
                done, status = True, 1
        E = evaluate(src, tgt, normals, T, s, lv["stride"], lv["max_dist"], k == 7, nearest)
        if li == len(levels) - 1 or status == 2 or E["n_corr"] < 8:
            break
    nc, ns = E["n_corr"], E["n_src"]
    return dict(T=T, scale=s, fitness=nc / ns if ns else 0.0, rmse=math.sqrt(E["e"] / nc) if nc else 0.0, n_corr=nc, n_src=ns,
                iters_run=iters_run, status=status, kept=kept)


def residuals(x, src, tgt_points, normals, T, scale):
    """r of FIXED correspondences (source point i with tgt_points[i] and normals[i]) at the pose moved by x: T <- exp(x) T,
    scale <- scale exp(x[6]).  What the finite differences of the CPU test differentiate."""
    w, q = transform(src, se3_apply(x, T), scale * math.exp(x[6]))
    e = q - np.asarray(tgt_points, np.float64)
    n = np.asarray(normals, np.float64)
    return (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
