"""numpy ray casting that follows DESIGN.md section 4.3 literally, over a record-ordered TSDF array ({sum, weight} per record,
as orc.tsdf or a downloaded grid holds it) and an optional centroid array ([records][4] u64).  Every quantity is f32 and
every operation is the kernel's, in its order (kernels_raycast.hip), so the result is the device's bit for bit.  Vectorised
over rays, a loop over steps."""
import numpy as np

F32 = np.float32
MAX_STEPS = 4096


def rec_index(i, j, k, dims):
    """record index of voxel (i, j, k): brick-major, 4x4x4 sub-bricks inside a brick, x fastest"""
    nbx, nby = dims[0] // 8, dims[1] // 8
    b = ((k >> 3) * nby + (j >> 3)) * nbx + (i >> 3)
    l = ((k & 4) << 6) | ((j & 4) << 5) | ((i & 4) << 4) | ((k & 3) << 4) | ((j & 3) << 2) | (i & 3)
    return (b << 9) | l


def _cell(rec, dims, mw, x):
    """(defined [n], corner values [n][8], fractions [n][3]) of the cells around the points x [n][3]"""
    inside = np.ones(len(x), bool)
    for a in range(3):
        inside &= (x[:, a] >= F32(0.0)) & (x[:, a] < F32(dims[a] - 1))
    xi = np.where(inside[:, None], x, F32(0.0))
    ijk = xi.astype(np.int64)
    f = (xi - ijk.astype(F32)).astype(F32)
    tc = np.empty((len(x), 8), F32)
    ok = inside.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(8):
            idx = rec_index(ijk[:, 0] + (c & 1), ijk[:, 1] + ((c >> 1) & 1), ijk[:, 2] + ((c >> 2) & 1), dims)
            s, w = rec[idx, 0], rec[idx, 1]
            ok &= w >= mw
            tc[:, c] = s.astype(F32) / (w.astype(F32) * F32(32767.0))
    return ok, tc, f


def _lerp(a, b, t):
    return a + t * (b - a)


def _trilinear(tc, f):
    c00, c10 = _lerp(tc[:, 0], tc[:, 1], f[:, 0]), _lerp(tc[:, 2], tc[:, 3], f[:, 0])
    c01, c11 = _lerp(tc[:, 4], tc[:, 5], f[:, 0]), _lerp(tc[:, 6], tc[:, 7], f[:, 0])
    return _lerp(_lerp(c00, c10, f[:, 1]), _lerp(c01, c11, f[:, 1]), f[:, 2])


def raycast(tsdf, dims, origin, voxel, trunc, cam, pose, min_weight=0, z_near=0.1, z_far=50.0, centroid=None, pixels=None):
    """(depth f32 [H,W], normals f32 [H,W,3], bgr u8 [H,W,3], samples int [H,W]) as tl3d_raycast defines them.
    cam: dict(width, height, fx, fy, cx, cy); pose: (R, t) world->camera; z_near / z_far: the resolved range.
    pixels: optional (u, v) index arrays -- only those rays are cast, and the outputs are flat arrays over them."""
    rec = np.asarray(tsdf).reshape(-1, 2)
    W, H = int(cam["width"]), int(cam["height"])
    if pixels is None:
        vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        u, v = uu.ravel(), vv.ravel()
    else:
        u, v = (np.asarray(p, np.int64).ravel() for p in pixels)
    n = len(u)
    R = np.asarray(pose[0], np.float64).reshape(3, 3)
    t = np.asarray(pose[1], np.float64).reshape(3)
    r32 = R.astype(F32)
    c = np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)]).astype(F32)
    org = np.asarray(origin, np.float64).astype(F32)
    ivs = F32(1.0 / float(voxel))
    vs32 = F32(voxel)
    half_vs = F32(0.5) * vs32
    step_k = F32(0.8) * F32(trunc)
    mw = max(1, int(min_weight))

    xf = (u.astype(F32) - F32(cam["cx"])) / F32(cam["fx"])
    yf = (v.astype(F32) - F32(cam["cy"])) / F32(cam["fy"])
    cg = np.empty(3, F32)
    dg = np.empty((n, 3), F32)
    z0 = np.full(n, F32(z_near), F32)
    z1 = np.full(n, F32(z_far), F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(3):
            d = (r32[0, a] * xf + r32[1, a] * yf) + r32[2, a]
            cg[a] = (c[a] - org[a]) * ivs - F32(0.5)
            dg[:, a] = d * ivs
            hi = F32(dims[a] - 1)
            nz = dg[:, a] != F32(0.0)
            safe = np.where(nz, dg[:, a], F32(1.0))
            ta = (F32(0.0) - cg[a]) / safe
            tb = (hi - cg[a]) / safe
            z0 = np.where(nz, np.maximum(z0, np.minimum(ta, tb)), z0)
            z1 = np.where(nz, np.minimum(z1, np.maximum(ta, tb)), z1)
            if not (cg[a] >= F32(0.0) and cg[a] <= hi):
                z1 = np.where(nz, z1, F32(-1.0))

    z = z0.copy()
    zp = np.zeros(n, F32)
    dzp = np.zeros(n, F32)
    fp = np.zeros(n, F32)
    prev = np.zeros(n, bool)
    hit = np.zeros(n, F32)
    samples = np.zeros(n, np.int64)
    active = z <= z1
    for _ in range(MAX_STEPS):
        ids = np.nonzero(active)[0]
        if len(ids) == 0:
            break
        x = (cg[None, :] + z[ids, None] * dg[ids]).astype(F32)
        ok, tc, f = _cell(rec, dims, mw, x)
        F = np.where(ok, _trilinear(tc, f), F32(0.0)).astype(F32)
        samples[ids] += 1
        end = ok & (F <= F32(0.0))
        h = end & prev[ids]
        hi_ = ids[h]
        with np.errstate(divide="ignore", invalid="ignore"):
            hit[hi_] = zp[hi_] + (dzp[hi_] * fp[hi_]) / (fp[hi_] - F[h])
        dz = np.where(ok, np.maximum(half_vs, F * step_k), vs32).astype(F32)
        go = ~end
        gi = ids[go]
        prev[gi] = ok[go]
        fp[gi] = F[go]
        zp[gi] = z[gi]
        dzp[gi] = dz[go]
        z[gi] = z[gi] + dz[go]
        active[ids[end]] = False
        active[gi] = z[gi] <= z1[gi]
    active[:] = False

    nrm = np.zeros((n, 3), F32)
    bgr = np.full((n, 3), 128, np.uint8)
    hid = np.nonzero(hit > F32(0.0))[0]
    if len(hid):
        x = (cg[None, :] + hit[hid, None] * dg[hid]).astype(F32)
        ok, tc, f = _cell(rec, dims, mw, x)
        d = lambda a, b: tc[:, a] - tc[:, b]
        gx = _lerp(_lerp(d(1, 0), d(3, 2), f[:, 1]), _lerp(d(5, 4), d(7, 6), f[:, 1]), f[:, 2])
        gy = _lerp(_lerp(d(2, 0), d(3, 1), f[:, 0]), _lerp(d(6, 4), d(7, 5), f[:, 0]), f[:, 2])
        gz = _lerp(_lerp(d(4, 0), d(5, 1), f[:, 0]), _lerp(d(6, 2), d(7, 3), f[:, 0]), f[:, 1])
        with np.errstate(invalid="ignore", over="ignore"):
            len2 = (gx * gx + gy * gy) + gz * gz
            good = ok & (len2 > F32(1e-30))
            inv = F32(1.0) / np.sqrt(np.where(good, len2, F32(1.0)))
        nw = [gx * inv, gy * inv, gz * inv]
        nc = np.stack([(r32[a, 0] * nw[0] + r32[a, 1] * nw[1]) + r32[a, 2] * nw[2] for a in range(3)], axis=1).astype(F32)
        flip = (nc[:, 0] * xf[hid] + nc[:, 1] * yf[hid]) + nc[:, 2] > F32(0.0)
        nc = np.where(flip[:, None], -nc, nc)
        nrm[hid] = np.where(good[:, None], nc, F32(0.0))
        if centroid is not None:
            cen = np.asarray(centroid).reshape(-1, 4)
            xv = (x + F32(0.5)).astype(F32)
            ins = np.ones(len(hid), bool)
            for a in range(3):
                ins &= (xv[:, a] >= F32(0.0)) & (xv[:, a] < F32(dims[a]))
            vi = np.where(ins[:, None], xv, F32(0.0)).astype(np.int64)
            cr = cen[rec_index(vi[:, 0], vi[:, 1], vi[:, 2], dims)]
            cnt = cr[:, 1] >> np.uint64(32)
            has = ins & (cnt > 0)
            cn = np.maximum(cnt, 1)
            rgb = np.stack([(cr[:, 2] & np.uint64(0xffffffff)) // cn, (cr[:, 2] >> np.uint64(32)) // cn,
                            (cr[:, 3] & np.uint64(0xffffffff)) // cn], axis=1)
            bgr[hid] = np.where(has[:, None], rgb[:, ::-1], 128).astype(np.uint8)
    if pixels is not None:
        return hit, nrm, bgr, samples
    return hit.reshape(H, W), nrm.reshape(H, W, 3), bgr.reshape(H, W, 3), samples.reshape(H, W)


def records_from_volume(sums, weights):
    """record-ordered {sum, weight} array from dense [nx][ny][nz] volumes"""
    dims = sums.shape
    ii, jj, kk = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    out = np.empty((sums.size, 2), np.int32)
    idx = rec_index(ii.ravel(), jj.ravel(), kk.ravel(), dims)
    out[idx, 0] = sums.ravel()
    out[idx, 1] = weights.ravel()
    return out
