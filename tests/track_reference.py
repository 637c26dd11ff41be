"""numpy restatement of point-to-SDF tracking (kernels_track.hip) over a record-ordered TSDF array ({sum,
weight} per record, as orc.tsdf or a downloaded grid holds it).  Not a test.

sums() is one pass: every per-sample quantity is f32 and every operation is the kernel's, in its order, so the gate decisions --
and hence n_src and n_corr -- are the device's exactly, and every summand is the device's bit for bit.  The sums themselves are
exactly rounded sums (math.fsum) of the exact fp64 products; the device adds the same terms in another order, so it may differ
from them by at most (n_corr - 1) 2^-53 sum|term| per sum: sums() returns sum|term| for that bound.
track() runs the levels with a plain fp64 solve (eigen-decomposition, same damping and eigenvalue cutoff)."""
import math

import numpy as np

from raycast_reference import _cell, _lerp, _trilinear

F32 = np.float32


def pose_matrix(pose):
    T = np.eye(4)
    T[:3, :3] = np.asarray(pose[0], np.float64).reshape(3, 3)
    T[:3, 3] = np.asarray(pose[1], np.float64).reshape(3)
    return T


def se3_apply(y, T):
    """[exp(w) | v] T, the pose update of the ICP kernels (oracle/tl3d_oracle.c: se3_apply)"""
    w, v = np.asarray(y[:3], np.float64), np.asarray(y[3:], np.float64)
    th2 = float(w @ w)
    th = math.sqrt(th2)
    a, b = (1.0, 0.5) if th < 1e-12 else (math.sin(th) / th, (1.0 - math.cos(th)) / th2)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    dR = np.eye(3) + a * K + b * (K @ K)
    out = np.eye(4)
    out[:3, :] = dR @ T[:3, :]
    out[:3, 3] += v
    return out


def pose_f32(T):
    """(R as f32, camera centre -R^T t from fp64 as f32): what a pass uses (track_pose_f32)"""
    R, t = T[:3, :3], T[:3, 3]
    c = np.array([-((float(R[0, i]) * float(t[0]) + float(R[1, i]) * float(t[1])) + float(R[2, i]) * float(t[2])) for i in range(3)])
    return R.astype(F32), c.astype(F32)


def sums(tsdf, dims, origin, voxel, trunc, cam, depth, pose, stride=2, max_dist=0.05, min_weight=1, min_depth=0.1, max_depth=50.0,
         scale=1.0, detail=False):
    """dict(A [21], b [6], e, n_corr, n_src, abs [28]: sum|term| of the 28 sums in the order A, b, e) of one pass at pose = (R, t)
    or a 4x4.  detail: also the per-correspondence arrays (u, v, p_c, cell corner ijk, tc, f, r, J)."""
    rec = np.asarray(tsdf).reshape(-1, 2)
    T = pose_matrix(pose) if isinstance(pose, (tuple, list)) and len(pose) == 2 else np.asarray(pose, np.float64).reshape(4, 4)
    r32, c32 = pose_f32(T)
    W, H = int(cam["width"]), int(cam["height"])
    depth = np.asarray(depth, F32).reshape(H, W)
    vv, uu = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    u, v = uu.ravel(), vv.ravel()
    d = depth[v, u] * F32(scale)
    valid = (d > F32(min_depth)) & (d < F32(max_depth))
    n_src = int(valid.sum())
    u, v, d = u[valid], v[valid], d[valid]
    xf = (u.astype(F32) - F32(cam["cx"])) / F32(cam["fx"])
    yf = (v.astype(F32) - F32(cam["cy"])) / F32(cam["fy"])
    p = np.stack([xf * d, yf * d, d], axis=1).astype(F32)
    org = np.asarray(origin, np.float64).astype(F32)
    ivs = F32(1.0 / float(voxel))
    trunc32 = F32(trunc)
    gate = min(F32(max_dist) / trunc32, F32(0.98))
    nk = trunc32 * ivs
    mw = max(1, int(min_weight))
    x = np.empty((len(u), 3), F32)
    for a in range(3):
        cg = (c32[a] - org[a]) * ivs - F32(0.5)
        w = (r32[0, a] * p[:, 0] + r32[1, a] * p[:, 1]) + r32[2, a] * p[:, 2]
        x[:, a] = cg + w * ivs
    ok, tc, f = _cell(rec, dims, mw, x)
    with np.errstate(invalid="ignore"):
        F = _trilinear(tc, f)
        corr = ok & (np.abs(F) <= gate)
    tc, f, F, p, x = tc[corr], f[corr], F[corr], p[corr], x[corr]
    dd = lambda a, b: tc[:, a] - tc[:, b]
    gx = _lerp(_lerp(dd(1, 0), dd(3, 2), f[:, 1]), _lerp(dd(5, 4), dd(7, 6), f[:, 1]), f[:, 2])
    gy = _lerp(_lerp(dd(2, 0), dd(3, 1), f[:, 0]), _lerp(dd(6, 4), dd(7, 5), f[:, 0]), f[:, 2])
    gz = _lerp(_lerp(dd(4, 0), dd(5, 1), f[:, 0]), _lerp(dd(6, 2), dd(7, 3), f[:, 0]), f[:, 1])
    res = F * trunc32
    gw = [gx * nk, gy * nk, gz * nk]
    n = [(r32[a, 0] * gw[0] + r32[a, 1] * gw[1]) + r32[a, 2] * gw[2] for a in range(3)]
    J = np.stack([p[:, 1] * n[2] - p[:, 2] * n[1], p[:, 2] * n[0] - p[:, 0] * n[2], p[:, 0] * n[1] - p[:, 1] * n[0], n[0], n[1], n[2]],
                 axis=1)
    assert J.dtype == F32 and res.dtype == F32 and x.dtype == F32
    Jd, rd = J.astype(np.float64), res.astype(np.float64)
    terms = [Jd[:, i] * Jd[:, j] for i in range(6) for j in range(i, 6)] + [Jd[:, i] * rd for i in range(6)] + [rd * rd]
    tot = np.array([math.fsum(t) for t in terms])
    mag = np.array([math.fsum(np.abs(t)) for t in terms])
    out = dict(A=tot[:21], b=tot[21:27], e=float(tot[27]), n_corr=int(corr.sum()), n_src=n_src, abs=mag)
    if detail:
        out.update(u=u[corr], v=v[corr], p=p, ijk=np.floor(x).astype(np.int64), tc=tc, f=f, r=res, J=J)
    return out


def sym6(a21):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = np.asarray(a21)[:21]
    return A + np.triu(A, 1).T


def solve(a21, b, damping, eig_rel):
    """x = -(A + lam I)^+ b over the eigen-directions with eigenvalue > eig_rel * largest; None when there is none"""
    A = sym6(a21)
    tr = float(np.trace(A))
    if not tr > 0.0:
        return None
    lam, V = np.linalg.eigh(A + damping * (tr / 6.0) * np.eye(6))
    lmax = float(lam.max())
    if not lmax > 0.0:
        return None
    keep = (lam > eig_rel * lmax) & (lam > 0.0)
    if not keep.any():
        return None
    return -(V[:, keep] @ ((V[:, keep].T @ np.asarray(b)) / lam[keep]))


def track(tsdf, dims, origin, voxel, trunc, cam, depth, pose_init, levels, min_weight=1, min_depth=0.1, max_depth=50.0, scale=1.0):
    """dict(T, pose, fitness, rmse, n_corr, n_src, iters_run, status) as tl3d_track_frame defines them; levels: dicts with iters,
    stride, max_dist, damping, eps, eig_rel."""
    T = pose_matrix(pose_init)
    kw = dict(min_weight=min_weight, min_depth=min_depth, max_depth=max_depth, scale=scale)
    s, status, iters_run = None, 0, 0
    for lv in levels:
        stride, gate = int(lv.get("stride", 4)), float(lv.get("max_dist", 0.05))
        status, iters_run = 0, 0
        for _ in range(int(lv.get("iters", 10))):
            s = sums(tsdf, dims, origin, voxel, trunc, cam, depth, T, stride, gate, **kw)
            x = solve(s["A"], s["b"], float(lv.get("damping", 1e-6)), float(lv.get("eig_rel", 1e-4))) if s["n_corr"] >= 8 else None
            if x is None:
                status = 2
                break
            T = se3_apply(-x, T)                           # J moves the point: the camera moves the other way
            iters_run += 1
            if np.abs(x).max() < float(lv.get("eps", 1e-9)):
                status = 1
                break
        s = sums(tsdf, dims, origin, voxel, trunc, cam, depth, T, stride, gate, **kw)
        if status == 2 or s["n_corr"] < 8:
            break
    nc, ns = s["n_corr"], s["n_src"]
    return dict(T=T, pose=(T[:3, :3].copy(), T[:3, 3].copy()), fitness=nc / ns if ns else 0.0, rmse=math.sqrt(s["e"] / nc) if nc else 0.0,
                n_corr=nc, n_src=ns, iters_run=iters_run, status=status)
