"""Pose-graph optimisation over ICP edges: the back end that closes loops ("Loop closure").

Nodes are the kept frames with poses T_k world -> camera; node 0 is fixed at the gauge it has (the reference's cam0 = (I, 0)).
An edge (i, j, Z, L) says X_j = Z X_i: Z is the registration of src = i against tgt = j (FusionContext.icp_batch) and L the 6 x 6
A = sum J J^T of the point-to-plane pass at Z (FusionContext.icp_evaluate), J = [p x n, n].  The registration perturbs its pose
from the left by exp(x) Z with x = (w, tau), exp(x) = [Exp(w) | tau] (se3_apply: rotation about the target camera's origin, then
a translation), and its cost near Z is x^T L x -- so the residual of an edge is

    x = Log(T_j T_i^-1 Z^-1) = (Log_SO3(R_e), t_e)        and the graph's cost      sum over edges of x^T L x.

Gauss-Newton with Levenberg damping and analytic Jacobians, on torch tensors in fp64 (cpu, or the device of the pipeline's
context).  A rank-deficient L (a plane slides, a cylinder spins) leaves directions of ITS edge free; the other edges and the
damping hold them, and the solve does not fail.  The normal equations are DENSE (6 (n - 1) squared doubles, Cholesky): 4096 nodes
are a 24 570^2 matrix of 4.8 GB, and larger graphs are refused (MAX_NODES) rather than solved worse.

numpy and torch only.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np
import torch

MAX_NODES = 4096                      # the dense normal equations of more nodes (> 4.8 GB) are refused


# ---- small-group helpers (batched, fp64) --------------------------------------------------------------------------------------
def _hat(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1),
                        torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def so3_exp(w):
    th2 = (w * w).sum(-1)
    th = torch.sqrt(th2)
    small = th < 1e-6
    ths = torch.where(small, torch.ones_like(th), th)
    a = torch.where(small, 1.0 - th2 / 6.0, torch.sin(ths) / ths)
    b = torch.where(small, 0.5 - th2 / 24.0, (1.0 - torch.cos(ths)) / (ths * ths))
    K = _hat(w)
    eye = torch.eye(3, dtype=w.dtype, device=w.device).expand(K.shape)
    return eye + a[..., None, None] * K + b[..., None, None] * (K @ K)


def so3_log(R):
    v = 0.5 * torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)    # sin(th) * axis
    s = torch.sqrt((v * v).sum(-1))
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1.0)
    th = torch.atan2(s, c)
    small = s < 1e-6
    k = torch.where(small, 1.0 + th * th / 6.0, th / torch.where(small, torch.ones_like(s), s))
    return v * k[..., None]


def _jl_inv(w):
    """Inverse of the left Jacobian of SO(3): Log(Exp(d) Exp(w)) = w + Jl^-1(w) d + O(d^2)."""
    th2 = (w * w).sum(-1)
    th = torch.sqrt(th2)
    small = th < 1e-4
    ths = torch.where(small, torch.ones_like(th), th)
    k = torch.where(small, 1.0 / 12.0 + th2 / 720.0, 1.0 / (ths * ths) - (1.0 + torch.cos(ths)) / (2.0 * ths * torch.sin(ths)))
    K = _hat(w)
    eye = torch.eye(3, dtype=w.dtype, device=w.device).expand(K.shape)
    return eye - 0.5 * K + k[..., None, None] * (K @ K)


def _inv(T):
    Rt = T[..., :3, :3].transpose(-1, -2)
    out = torch.zeros_like(T)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:4])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def poses_to_matrices(poses) -> np.ndarray:
    """[(R, t)] (the pipeline's camera_poses) or an [n, 4, 4] array -> [n, 4, 4] fp64."""
    if isinstance(poses, np.ndarray) and poses.ndim == 3:
        return np.array(poses, np.float64)
    T = np.tile(np.eye(4), (len(poses), 1, 1))
    for k, (R, t) in enumerate(poses):
        T[k, :3, :3] = np.asarray(R, np.float64)
        T[k, :3, 3] = np.asarray(t, np.float64).reshape(3)
    return T


def matrices_to_poses(T) -> List[Tuple[np.ndarray, np.ndarray]]:
    return [(np.array(M[:3, :3]), np.array(M[:3, 3]).reshape(3, 1)) for M in np.asarray(T)]


def relative_pose(T_i, T_j) -> np.ndarray:
    """The src = i -> tgt = j transform two absolute poses imply: T_j T_i^-1."""
    Ti = np.asarray(T_i, np.float64)
    Tinv = np.eye(4)
    Tinv[:3, :3] = Ti[:3, :3].T
    Tinv[:3, 3] = -Ti[:3, :3].T @ Ti[:3, 3]
    return np.asarray(T_j, np.float64) @ Tinv


# ---- candidates -----------------------------------------------------------------------------------------------------------------
def loop_candidates(poses, min_gap: int, max_dist: float, max_angle_deg: float) -> List[Tuple[int, int]]:
    """Pairs (i, j) of nodes with j - i >= min_gap whose camera centres are closer than max_dist and whose view axes are less than
    max_angle_deg apart, from the poses as they stand (the chain's).  Sorted by (j, i).  A dolly down a corridor has none."""
    T = poses_to_matrices(poses)
    n = len(T)
    if n == 0:
        return []
    R, t = T[:, :3, :3], T[:, :3, 3]
    centre = -np.einsum("nji,nj->ni", R, t)              # C = -R^T t
    axis = R[:, 2, :]                                    # the camera's +z in the world
    out = []
    cos_lim = math.cos(math.radians(max_angle_deg))
    for j in range(int(min_gap), n):
        i_hi = j - int(min_gap) + 1
        d = np.linalg.norm(centre[:i_hi] - centre[j], axis=1)
        c = axis[:i_hi] @ axis[j]
        for i in np.nonzero((d < max_dist) & (c > cos_lim))[0]:
            out.append((int(i), j))
    return out


def select_candidates(cands: Sequence[Tuple[int, int]], n_corr: Sequence[float], fitness: Sequence[float], per_frame: int,
                      min_fitness: float) -> List[int]:
    """Indices into `cands` of the ones kept: for every later frame j, the `per_frame` best by n_corr among those of its candidates
    (i, j) whose fitness is at least min_fitness (ties: the earlier i).  In the order of `cands`."""
    by_j = {}
    for k, (i, j) in enumerate(cands):
        if fitness[k] >= min_fitness:
            by_j.setdefault(j, []).append(k)
    keep = []
    for j, ks in by_j.items():
        ks.sort(key=lambda k: (-n_corr[k], cands[k][0]))
        keep.extend(ks[:max(0, int(per_frame))])
    return sorted(keep)


# ---- residuals and the solve ------------------------------------------------------------------------------------------------------
def _edge_tensors(edges, dtype, device):
    ii = torch.tensor([e[0] for e in edges], dtype=torch.long, device=device)
    jj = torch.tensor([e[1] for e in edges], dtype=torch.long, device=device)
    Z = torch.as_tensor(np.stack([np.asarray(e[2], np.float64).reshape(4, 4) for e in edges]), dtype=dtype, device=device)
    L = torch.as_tensor(np.stack([np.asarray(e[3], np.float64).reshape(6, 6) for e in edges]), dtype=dtype, device=device)
    return ii, jj, Z, 0.5 * (L + L.transpose(-1, -2))


def _residuals(T, ii, jj, Zinv):
    E = T[jj] @ _inv(T[ii]) @ Zinv
    return torch.cat([so3_log(E[:, :3, :3]), E[:, :3, 3]], -1), E


def _jacobians(x, E, Z):
    """d x / d delta_i and d x / d delta_j ([E, 6, 6] each) for the left perturbations T_k <- [Exp(dw_k) | dtau_k] T_k."""
    Re, te = E[:, :3, :3], E[:, :3, 3]
    Rz, tz = Z[:, :3, :3], Z[:, :3, 3]
    Ji_inv = _jl_inv(x[:, :3])
    n = x.shape[0]
    Jj = torch.zeros(n, 6, 6, dtype=x.dtype, device=x.device)
    Jj[:, :3, :3] = Ji_inv
    Jj[:, 3:, :3] = -_hat(te)
    Jj[:, 3:, 3:] = torch.eye(3, dtype=x.dtype, device=x.device)
    ReRz = Re @ Rz
    Ji = torch.zeros_like(Jj)
    Ji[:, :3, :3] = -Ji_inv @ ReRz
    Ji[:, 3:, :3] = -Re @ _hat(tz) @ Rz
    Ji[:, 3:, 3:] = -ReRz
    return Ji, Jj


def _cost(x, L):
    return float(torch.einsum("ea,eab,eb->", x, L, x))


def _apply(T, delta):
    """T_k <- [Exp(dw_k) | dtau_k] T_k for the free nodes 1 .. n - 1."""
    out = T.clone()
    dR = so3_exp(delta[:, :3])
    out[1:, :3, :3] = dR @ T[1:, :3, :3]
    out[1:, :3, 3] = (dR @ T[1:, :3, 3:4])[..., 0] + delta[:, 3:]
    return out


def edge_residuals(poses, edges) -> np.ndarray:
    """[E, 6] residuals (w, tau) of the edges at `poses`."""
    if not len(edges):
        return np.zeros((0, 6))
    T = torch.as_tensor(poses_to_matrices(poses))
    ii, jj, Z, _ = _edge_tensors(edges, T.dtype, T.device)
    return _residuals(T, ii, jj, _inv(Z))[0].numpy()


def optimise(poses, edges, device="cpu", max_iters: int = 50, step_tol: float = 1e-10, damping: float = 1e-6):
    """Minimise sum x_e^T L_e x_e over the poses of nodes 1 .. n - 1 (node 0 stays).  poses: [(R, t)] or [n, 4, 4], world ->
    camera; edges: [(i, j, Z, L)].  Returns (poses in the form they came in, info) with info = dict(iterations, cost_before,
    cost_after, converged, max_step).  Stops when the largest component of a step is below step_tol (rad / m) or after max_iters."""
    as_list = not (isinstance(poses, np.ndarray) and poses.ndim == 3)
    T0 = poses_to_matrices(poses)
    n = len(T0)
    if n > MAX_NODES:
        raise ValueError(f"pose graph of {n} nodes: the dense solve holds a {6 * (n - 1)}^2 fp64 matrix and is limited to {MAX_NODES} nodes "
                         f"({(6.0 * (MAX_NODES - 1)) ** 2 * 8 / 1e9:.1f} GB); a block-sparse solve does not exist here")
    info = dict(iterations=0, cost_before=0.0, cost_after=0.0, converged=True, max_step=0.0)
    if n < 2 or not len(edges):
        return (matrices_to_poses(T0) if as_list else T0), info
    for e in edges:
        if not (0 <= e[0] < n and 0 <= e[1] < n and e[0] != e[1]):
            raise ValueError(f"edge ({e[0]}, {e[1]}) does not join two of the {n} nodes")
    dev = torch.device(device)
    T = torch.as_tensor(T0, dtype=torch.float64, device=dev)
    ii, jj, Z, L = _edge_tensors(edges, torch.float64, dev)
    Zinv = _inv(Z)
    x, E = _residuals(T, ii, jj, Zinv)
    cost = _cost(x, L)
    info["cost_before"] = info["cost_after"] = cost
    m = 6 * n
    lam = float(damping)
    a6 = torch.arange(6, device=dev)
    converged = False
    for it in range(int(max_iters)):
        Ji, Jj = _jacobians(x, E, Z)
        LJi, LJj = L @ Ji, L @ Jj
        H = torch.zeros(m, m, dtype=torch.float64, device=dev)
        H4 = H.view(n, 6, n, 6)
        for (a, Ja), (b, LJb) in (((ii, Ji), (ii, LJi)), ((ii, Ji), (jj, LJj)), ((jj, Jj), (ii, LJi)), ((jj, Jj), (jj, LJj))):
            H4.index_put_((a[:, None, None], a6[None, :, None], b[:, None, None], a6[None, None, :]), Ja.transpose(-1, -2) @ LJb, accumulate=True)
        g = torch.zeros(n, 6, dtype=torch.float64, device=dev)
        Lx = (L @ x[..., None])[..., 0]
        g.index_add_(0, ii, (Ji.transpose(-1, -2) @ Lx[..., None])[..., 0])
        g.index_add_(0, jj, (Jj.transpose(-1, -2) @ Lx[..., None])[..., 0])
        Hf, gf = H[6:, 6:], g[1:].reshape(-1)
        diag = torch.diagonal(Hf).clone()
        floor = float(diag.max()) * 1e-12 + 1e-300          # a node no edge observes in some direction still gets a pivot
        accepted = False
        for _ in range(12):
            Hd = Hf.clone()
            torch.diagonal(Hd).add_(lam * diag + floor)
            Lc, bad = torch.linalg.cholesky_ex(Hd)
            if int(bad) == 0:
                delta = -torch.cholesky_solve(gf[:, None], Lc)[:, 0].reshape(n - 1, 6)
                Tn = _apply(T, delta)
                xn, En = _residuals(Tn, ii, jj, Zinv)
                cn = _cost(xn, L)
                if cn <= cost:
                    accepted = True
                    break
            lam = max(lam, 1e-9) * 10.0
        if not accepted:
            break
        step = float(delta.abs().max())
        T, x, E, cost = Tn, xn, En, cn
        lam = max(lam * 0.1, float(damping))
        info["iterations"] = it + 1
        info["max_step"] = step
        if step < step_tol:
            converged = True
            break
    info["cost_after"] = cost
    info["converged"] = converged
    out = T.cpu().numpy()
    return (matrices_to_poses(out) if as_list else out), info


def optimise_and_prune(poses, edges, is_loop: Sequence[bool], max_residual: float, **kw):
    """optimise(), then drop the LOOP edges (is_loop[k]) whose residual translation exceeds max_residual metres at the optimum --
    a wrong closure that the registration accepted pulls against every other edge and keeps most of its error as residual -- and
    optimise once more, from the original poses, if any were dropped.  Odometry edges are never dropped (the graph stays
    connected).  Returns (poses, info) with info gaining pruned = the indices dropped and residual_m = the loop edges' residual
    translations before pruning."""
    out, info = optimise(poses, edges, **kw)
    res = edge_residuals(out, edges)
    tau = np.linalg.norm(res[:, 3:], axis=1) if len(edges) else np.zeros(0)
    pruned = [k for k in range(len(edges)) if is_loop[k] and tau[k] > max_residual]
    info["residual_m"] = [float(tau[k]) for k in range(len(edges)) if is_loop[k]]
    if pruned:
        gone = set(pruned)
        first = info
        out, info = optimise(poses, [e for k, e in enumerate(edges) if k not in gone], **kw)
        info["iterations"] += first["iterations"]
        info["cost_before"] = first["cost_before"]
        info["residual_m"] = first["residual_m"]
    info["pruned"] = pruned
    return out, info


def largest_correction(before, after) -> Tuple[float, float]:
    """(millimetres, degrees): the largest camera-centre displacement and the largest rotation between two sets of poses."""
    A, B = poses_to_matrices(before), poses_to_matrices(after)
    ca = -np.einsum("nji,nj->ni", A[:, :3, :3], A[:, :3, 3])
    cb = -np.einsum("nji,nj->ni", B[:, :3, :3], B[:, :3, 3])
    mm = float(np.linalg.norm(ca - cb, axis=1).max()) * 1e3 if len(A) else 0.0
    tr = np.einsum("nij,nij->n", A[:, :3, :3], B[:, :3, :3])
    deg = float(np.degrees(np.arccos(np.clip(0.5 * (tr - 1.0), -1.0, 1.0))).max()) if len(A) else 0.0
    return mm, deg
