"""numpy reference of the joint point-to-plane + photometric registration (csrc/kernels_rgbd.hip).  Not a test.
This file is the NORMATIVE sequence of the photometric half: the kernels restate it.

intensity_map      (S, Sx, Sy, flag) per pixel, vectorised; intensity_map_brute: the same definition as a per-pixel loop
sums               one pass of both systems at a pose: f32 per-sample values (dtype=F32: bit for bit what the device computes per
                   sample) or everything in fp64 (dtype=F64: for derivative checks), fp64 sums of fp64 products
register           levels of iterations with the stop / failure / chaining rules of the batched ICP

The geometric half follows csrc/icp_sample.h (icp_accumulate_core): fmaf chains, the pixel-ray quotients ((float)u - cx) / fx, the
IEEE reciprocal of pz, nearest-pixel association, gate, residual, J = [q x n, n]."""
import math

import numpy as np

import track_reference as tr

F32, F64 = np.float32, np.float64


def fma(a, b, c, dtype=F32):
    """fmaf for dtype F32: the product of two floats is exact in a double; its sum with c is rounded to ODD there (53 >= 2 * 24 + 2
    bits make the second rounding harmless), then to float.  For F64: a * b + c (derivative checks do not need the single rounding)."""
    if dtype is F64:
        return np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)
    a, b, c = (np.asarray(x, F32).astype(F64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = np.asarray(p + c)
        t = s - p
        err = (p - (s - t)) + (c - t)                         # TwoSum: p + c = s + err exactly
        odd = (s.view(np.int64) & 1) == 1
        fix = np.isfinite(s) & (err != 0.0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(F32)


# ---- intensity maps ----------------------------------------------------------------------------------------------------------
def luma(bgr):
    c = np.asarray(bgr, np.int64)
    return 29 * c[..., 0] + 150 * c[..., 1] + 77 * c[..., 2]


def _valid(d):
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def _linked(a, b, jump):
    with np.errstate(invalid="ignore"):
        return np.abs((a - b).astype(F32)) <= (F32(jump) * np.minimum(a, b)).astype(F32)


def _shift(a, dv, du, fill):
    """a[v + dv, u + du] where that is in the image, else fill"""
    H, W = a.shape
    out = np.full_like(a, fill)
    vs, us = slice(max(0, -dv), min(H, H - dv)), slice(max(0, -du), min(W, W - du))
    vd, ud = slice(max(0, -dv) + dv, min(H, H - dv) + dv), slice(max(0, -du) + du, min(W, W - du) + du)
    out[vs, us] = a[vd, ud]
    return out


def intensity_map(depth, bgr, radius=1, jump=0.05):
    """[H, W, 4] float32: (S, Sx, Sy, flag)"""
    d = np.asarray(depth, F32)
    y = luma(bgr)
    H, W = d.shape
    ok = _valid(d)
    tot, cnt = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    dz = np.where(ok, d, F32(0))
    for dv in range(-radius, radius + 1):
        for du in range(-radius, radius + 1):
            dn, okn, yn = _shift(dz, dv, du, F32(0)), _shift(ok, dv, du, False), _shift(y, dv, du, 0)
            m = ok & okn & _linked(dn, dz, jump)
            tot += np.where(m, yn, 0)
            cnt += m
    S = np.zeros((H, W), F32)
    S[ok] = (tot[ok].astype(F32) / (cnt[ok] * 65280).astype(F32)).astype(F32)
    full = ok.copy()
    for dv, du in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        dn, okn = _shift(dz, dv, du, F32(0)), _shift(ok, dv, du, False)
        full &= okn & _linked(dn, dz, jump)
    out = np.zeros((H, W, 4), F32)
    out[..., 0] = S
    sx = (F32(0.5) * (_shift(S, 0, 1, F32(0)) - _shift(S, 0, -1, F32(0))).astype(F32)).astype(F32)
    sy = (F32(0.5) * (_shift(S, 1, 0, F32(0)) - _shift(S, -1, 0, F32(0))).astype(F32)).astype(F32)
    out[..., 1] = np.where(full, sx, F32(0))
    out[..., 2] = np.where(full, sy, F32(0))
    out[..., 3] = np.where(full, F32(2), np.where(ok, F32(1), F32(0)))
    return out


def intensity_map_brute(depth, bgr, radius=1, jump=0.05):
    """the definition, pixel by pixel in Python scalars of numpy's float32"""
    d = np.asarray(depth, F32)
    c = np.asarray(bgr)
    H, W = d.shape
    jump = F32(jump)

    def valid(v, u):
        return 0 <= v < H and 0 <= u < W and bool(np.isfinite(d[v, u])) and d[v, u] > 0

    def linked(a, b):
        return abs(F32(a - b)) <= F32(jump * min(a, b))
    S = np.zeros((H, W), F32)
    for v in range(H):
        for u in range(W):
            if not valid(v, u):
                continue
            tot = n = 0
            for vv in range(v - radius, v + radius + 1):
                for uu in range(u - radius, u + radius + 1):
                    if valid(vv, uu) and linked(d[vv, uu], d[v, u]):
                        tot += 29 * int(c[vv, uu, 0]) + 150 * int(c[vv, uu, 1]) + 77 * int(c[vv, uu, 2])
                        n += 1
            S[v, u] = F32(tot) / F32(n * 65280)
    out = np.zeros((H, W, 4), F32)
    for v in range(H):
        for u in range(W):
            if not valid(v, u):
                continue
            nb = ((v, u - 1), (v, u + 1), (v - 1, u), (v + 1, u))
            full = all(valid(*p) and linked(d[p], d[v, u]) for p in nb)
            out[v, u, 0] = S[v, u]
            out[v, u, 3] = 2 if full else 1
            if full:
                out[v, u, 1] = F32(0.5) * F32(S[v, u + 1] - S[v, u - 1])
                out[v, u, 2] = F32(0.5) * F32(S[v + 1, u] - S[v - 1, u])
    return out


# ---- one pass ------------------------------------------------------------------------------------------------------------------
def _cross_j(p, n, dtype):
    """[q x n, n] with the fmaf pattern of the kernels: fmaf(py, nz, -(pz * ny)), ..."""
    px, py, pz = p
    nx, ny, nz = n
    return [fma(py, nz, -(pz * ny), dtype), fma(pz, nx, -(px * nz), dtype), fma(px, ny, -(py * nx), dtype), nx, ny, nz]


def _system(J, r):
    """(a[21], b[6], e, abs[28]: sum |term| of each of the 28 sums) of per-sample J [6][n] and r [n], as fp64 sums of fp64 products"""
    J = [np.asarray(j, F64) for j in J]
    r = np.asarray(r, F64)
    terms = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * r for a in range(6)] + [r * r]
    s = np.array([t.sum() for t in terms])
    return s[:21], s[21:27], float(s[27]), np.array([np.abs(t).sum() for t in terms])


def sums(cam, src_map, nmap, imap_src, imap_tgt, T, stride=2, max_dist=0.05, photo_gate=0.2, min_depth=0.1, max_depth=50.0, scale=1.0,
         dtype=F32, detail=False):
    """One pass at T (4 x 4, source camera -> target camera).  src_map: the depth the pass reads of the source (row-major; the
    window-averaged one when normal smoothing is on), nmap: the target's normal map [H, W, 4], imap_*: intensity maps [H, W, 4].
    dict(A, b, e, abs: the geometric system; A_p, b_p, e_p, abs_p: the photometric one; n_corr, n_src, n_qualified, n_photo);
    detail: also per-sample arrays over ALL samples of the stride grid, row-major: u, v, ut, vt, the masks corr / qualified / photo,
    ri (r_I) and J_p (J_I, [6, n]); values outside their mask are meaningless."""
    W, H = int(cam["width"]), int(cam["height"])
    fx, fy, cx, cy = (dtype(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    T = np.asarray(T, F64).reshape(4, 4)
    r, t = T[:3, :3].astype(dtype), T[:3, 3].astype(dtype)
    vv, uu = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    u, v = uu.ravel(), vv.ravel()
    md = dtype(F32(max_dist))
    md2 = dtype(md * md)
    with np.errstate(all="ignore"):
        d = (np.asarray(src_map, F32)[v, u].astype(dtype) * dtype(scale)).astype(dtype)
        src_ok = (d > dtype(min_depth)) & (d < dtype(max_depth))
        p0 = ((u.astype(dtype) - cx) / fx).astype(dtype) * d
        p1 = ((v.astype(dtype) - cy) / fy).astype(dtype) * d
        px, py, pz = (fma(r[a, 0], p0, fma(r[a, 1], p1, fma(r[a, 2], d, t[a], dtype), dtype), dtype) for a in range(3))
        inv = (dtype(1.0) / pz).astype(dtype)
        uf = fma((fx * px).astype(dtype), inv, cx, dtype)
        vf = fma((fy * py).astype(dtype), inv, cy, dtype)
        reach = src_ok & (pz > 0) & (uf >= dtype(-0.5)) & (uf < dtype(W) - dtype(0.5)) & (vf >= dtype(-0.5)) & (vf < dtype(H) - dtype(0.5))
        ut = np.where(reach, np.minimum(np.floor(uf + dtype(0.5)), W - 1), 0).astype(np.int64)
        vt = np.where(reach, np.minimum(np.floor(vf + dtype(0.5)), H - 1), 0).astype(np.int64)
        nd = np.asarray(nmap, F32)[vt, ut].astype(dtype)
        nx, ny, nz, dt = (nd[:, i] for i in range(4))
        qx = ((ut.astype(dtype) - cx) / fx).astype(dtype) * dt
        qy = ((vt.astype(dtype) - cy) / fy).astype(dtype) * dt
        dx, dy, dz = px - qx, py - qy, pz - dt
        dist2 = fma(dx, dx, fma(dy, dy, dz * dz, dtype), dtype)
        corr = reach & (dt > 0) & (dist2 <= md2)
        res = fma(dx, nx, fma(dy, ny, dz * nz, dtype), dtype)
        Jg = _cross_j((px, py, pz), (nx, ny, nz), dtype)
        mt = np.asarray(imap_tgt, F32)[vt, ut].astype(dtype)
        ms = np.asarray(imap_src, F32)[v, u].astype(dtype)
        qual = corr & (mt[:, 3] == 2) & (ms[:, 3] >= 1)
        ri = (fma(mt[:, 1], uf - ut.astype(dtype), fma(mt[:, 2], vf - vt.astype(dtype), mt[:, 0], dtype), dtype) - ms[:, 0]).astype(dtype)
        photo = qual & (np.abs(ri) <= dtype(F32(photo_gate)))
        gx = ((mt[:, 1] * fx).astype(dtype) * inv).astype(dtype)
        gy = ((mt[:, 2] * fy).astype(dtype) * inv).astype(dtype)
        gz = (-fma(gx, px, gy * py, dtype) * inv).astype(dtype)
        Jp = _cross_j((px, py, pz), (gx, gy, gz), dtype)
    A, b, e, ab = _system([j[corr] for j in Jg], res[corr])
    A_p, b_p, e_p, ab_p = _system([j[photo] for j in Jp], ri[photo])
    out = dict(A=A, b=b, e=e, abs=ab, A_p=A_p, b_p=b_p, e_p=e_p, abs_p=ab_p, n_corr=int(corr.sum()), n_src=int(src_ok.sum()),
               n_qualified=int(qual.sum()), n_photo=int(photo.sum()))
    if detail:
        out.update(u=u, v=v, ut=ut, vt=vt, corr=corr, qualified=qual, photo=photo, ri=ri.astype(F64), J_p=np.stack([np.asarray(j, F64) for j in Jp]))
    return out


# ---- the registration ---------------------------------------------------------------------------------------------------------------
def joint(s, weight):
    """(a[21], b[6]) of A_g + weight A_p, b_g + weight b_p: a product, then a sum, in fp64"""
    return s["A"] + weight * s["A_p"], s["b"] + weight * s["b_p"]


def kept(a21, damping, eig_rel):
    """eigen-directions of the damped joint system above the cutoff"""
    A = tr.sym6(a21)
    lam = np.linalg.eigvalsh(A + damping * (np.trace(A) / 6.0) * np.eye(6))
    return int(((lam > eig_rel * lam.max()) & (lam > 0)).sum())


def register(cam, src_map, nmap, imap_src, imap_tgt, T_init, levels, min_depth=0.1, max_depth=50.0, scale=1.0):
    """dict(T, fitness, rmse, n_corr, n_src, iters_run, status, photo_rmse, n_photo, n_qualified, kept: directions kept by the last
    solve) as tl3d_rgbd_register_pairs defines them; levels: dicts with iters, stride, max_dist, damping, eps, eig_rel, photo_weight,
    photo_gate"""
    T = np.asarray(T_init, F64).reshape(4, 4).copy()
    s, status, iters_run, n_kept = None, 0, 0, 0
    for li, lv in enumerate(levels):
        kw = dict(stride=int(lv.get("stride", 4)), max_dist=float(lv.get("max_dist", 0.05)), photo_gate=float(lv.get("photo_gate", 0.2)),
                  min_depth=min_depth, max_depth=max_depth, scale=scale)
        w, damping, eig_rel = float(lv.get("photo_weight", 0.1)), float(lv.get("damping", 1e-6)), float(lv.get("eig_rel", 1e-4))
        status, iters_run = 0, 0
        for _ in range(int(lv.get("iters", 10))):
            s = sums(cam, src_map, nmap, imap_src, imap_tgt, T, **kw)
            a21, b = joint(s, w)
            x = tr.solve(a21, b, damping, eig_rel) if s["n_corr"] >= 6 else None
            if x is None:
                status = 2
                break
            n_kept = kept(a21, damping, eig_rel)
            T = tr.se3_apply(x, T)
            iters_run += 1
            if np.abs(x).max() < float(lv.get("eps", 1e-9)):
                status = 1
                break
        s = sums(cam, src_map, nmap, imap_src, imap_tgt, T, **kw)           # the final pass of the level
        if status == 2 or s["n_corr"] < 8:
            break
    return dict(T=T, fitness=s["n_corr"] / s["n_src"] if s["n_src"] else 0.0, rmse=math.sqrt(s["e"] / s["n_corr"]) if s["n_corr"] else 0.0,
                n_corr=s["n_corr"], n_src=s["n_src"], iters_run=iters_run, status=status, n_photo=s["n_photo"], n_qualified=s["n_qualified"],
                photo_rmse=math.sqrt(s["e_p"] / s["n_photo"]) if s["n_photo"] else 0.0, kept=n_kept)
