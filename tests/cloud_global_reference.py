"""numpy restatement of the global registration's contracts (include/tl3d.h): voxel subsample, FPFH, nearest
feature and RANSAC, each as the NORMATIVE sequence of fp64 operations -- one rounding per operation, dot products and squared
lengths as (a + b) + c, sums in list order -- so that the integer outputs of the GPU calls can be compared exactly.  numpy's
elementwise operations round once each and never fuse, which is what makes this file a restatement and not an approximation.

Every routine that takes a decision on a computed value also reports its UNDECIDED cases: inputs so close to the decision's edge
that a last-bit difference in a library function (atan2 is not correctly rounded everywhere) could move them.  The tests assert
there are none on the cases they compare exactly.
"""
import numpy as np

PI, TWO_PI = 3.14159265358979323846, 6.28318530717958647692
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
U64 = np.uint64


# ---- subsample -----------------------------------------------------------------------------------------------------------------
def voxel_subsample(xyz, voxel):
    """Ascending indices: per occupied cell floor(x / voxel) the member with the smallest index."""
    p = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    cell = np.floor(p / float(voxel)).astype(np.int64)
    if len(cell) and np.abs(cell).max() >= 1 << 20:
        raise ValueError("|cell| >= 2^20")
    seen, keep = set(), []
    for i, c in enumerate(map(tuple, cell)):
        if c not in seen:
            seen.add(c)
            keep.append(i)
    return np.array(keep, np.int32)


# ---- neighbourhoods ------------------------------------------------------------------------------------------------------------
def knn_lists(xyz, k, max_radius):
    """(index [n, k'] int64, d2 [n, k'] fp64) with k' = min(k, n): the k' smallest under (d2, index), -1 / inf where the radius
    cut removed a member.  Brute force."""
    p = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(p)
    k = min(int(k), n)
    md2 = float(max_radius) * float(max_radius) if max_radius > 0 else np.inf
    idx = np.empty((n, k), np.int64)
    d2o = np.empty((n, k), np.float64)
    for i in range(n):
        d = p - p[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        order = np.argsort(d2, kind="stable")[:k]                 # stable: an exact tie keeps the smaller index first
        idx[i], d2o[i] = order, d2[order]
    cut = d2o > md2
    idx[cut], d2o[cut] = -1, np.inf
    return idx, d2o


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _bin(u):
    return np.clip(np.floor(u), 0, 10).astype(np.int64)


def _near_edge(u, tol=1e-9):
    """u within tol of one of the ten inner bin edges 1 .. 10 (beyond them the clamp decides either way)"""
    r = np.rint(u)
    return (np.abs(u - r) < tol) & (r >= 1) & (r <= 10)


def fpfh(xyz, normals, k, max_radius):
    """dict: fpfh float32 [n, 33], spfh int32 [n, 34], members int64 [n, k'] (N(i) in list order, -1: none), bar float64 [n, 33] (the
    summation-order bound of the tests, see test_gpu_cloud_global.py), undecided (pairs whose scaled feature lies within 1e-9 of a
    bin edge)."""
    p = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    nr = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(p)
    idx, d2 = knn_lists(p, k, max_radius)
    kk = idx.shape[1]
    zero_n = (nr[:, 0] == 0) & (nr[:, 1] == 0) & (nr[:, 2] == 0)
    member = (idx >= 0) & (d2 > 0)
    member &= ~zero_n[np.where(idx >= 0, idx, 0)]
    idx = np.where(member, idx, -1)
    counts = np.zeros((n, 33), np.int64)
    m = np.zeros(n, np.int64)
    undecided = 0
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        for j in range(kk):
            jj = np.where(member[:, j], idx[:, j], 0)
            ok = member[:, j] & ~zero_n
            dx, dy, dz = p[jj, 0] - p[:, 0], p[jj, 1] - p[:, 1], p[jj, 2] - p[:, 2]
            L = np.sqrt((dx * dx + dy * dy) + dz * dz)
            nix, niy, niz = nr[:, 0], nr[:, 1], nr[:, 2]
            njx, njy, njz = nr[jj, 0], nr[jj, 1], nr[jj, 2]
            a1 = _dot(nix, niy, niz, dx, dy, dz) / L
            a2 = _dot(njx, njy, njz, dx, dy, dz) / L
            sw = np.abs(a1) < np.abs(a2)
            sx, sy, sz = np.where(sw, njx, nix), np.where(sw, njy, niy), np.where(sw, njz, niz)
            tx, ty, tz = np.where(sw, nix, njx), np.where(sw, niy, njy), np.where(sw, niz, njz)
            f3 = np.where(sw, -a2, a1)
            dx, dy, dz = np.where(sw, -dx, dx), np.where(sw, -dy, dy), np.where(sw, -dz, dz)
            vx, vy, vz = dy * sz - dz * sy, dz * sx - dx * sz, dx * sy - dy * sx
            vl = np.sqrt((vx * vx + vy * vy) + vz * vz)
            ok &= vl != 0
            vx, vy, vz = vx / vl, vy / vl, vz / vl
            wx, wy, wz = sy * vz - sz * vy, sz * vx - sx * vz, sx * vy - sy * vx
            f2 = _dot(vx, vy, vz, tx, ty, tz)
            f1 = np.arctan2(_dot(wx, wy, wz, tx, ty, tz), _dot(sx, sy, sz, tx, ty, tz))
            u1, u2, u3 = 11.0 * (f1 + PI) / TWO_PI, 11.0 * (f2 + 1.0) / 2.0, 11.0 * (f3 + 1.0) / 2.0
            for off, u in ((0, u1), (11, u2), (22, u3)):
                undecided += int((_near_edge(u) & ok).sum())
                np.add.at(counts, (rows[ok], off + _bin(u[ok])), 1)
            m += ok
        # the descriptor: S in list order, the groups scaled, the own SPFH added
        S = np.zeros((n, 33))
        S_abs_terms = np.zeros(n, np.int64)
        for j in range(kk):
            jj = np.where(member[:, j], idx[:, j], 0)
            ok = member[:, j] & (m[jj] > 0) & (m > 0)
            dx, dy, dz = p[jj, 0] - p[:, 0], p[jj, 1] - p[:, 1], p[jj, 2] - p[:, 2]
            dd = (dx * dx + dy * dy) + dz * dz
            term = (100.0 * counts[jj].astype(np.float64) / m[jj].astype(np.float64)[:, None]) / dd[:, None]
            S += np.where(ok[:, None], term, 0.0)
            S_abs_terms += ok
        F = np.zeros((n, 33))
        bar = np.zeros((n, 33))
        e = S_abs_terms[:, None] * 2.0 ** -52 * S                # terms are >= 0: sum |term| = S
        for g in range(3):
            sl = slice(11 * g, 11 * g + 11)
            tot = np.zeros(n)
            for b in range(11):
                tot = tot + S[:, 11 * g + b]
            pos = tot > 0
            f = np.where(pos, 100.0 / np.where(pos, tot, 1.0), 1.0)
            scaled = np.where(pos[:, None], S[:, sl] * f[:, None], S[:, sl])
            own = 100.0 * counts[:, sl].astype(np.float64) / np.where(m > 0, m, 1).astype(np.float64)[:, None]
            F[:, sl] = scaled + own
            e_tot = e[:, sl].sum(axis=1) + 11 * 2.0 ** -52 * tot
            rel = np.where(pos, e_tot / np.where(pos, tot, 1.0), 0.0)
            bar[:, sl] = f[:, None] * e[:, sl] + scaled * rel[:, None] + 4 * 2.0 ** -52 * np.abs(F[:, sl])
        F[m == 0] = 0.0
        bar[m == 0] = 0.0
        out = F.astype(np.float32)
        bar = bar + 2.0 ** -23 * np.abs(F)                        # one f32 rounding on either side
    spfh = np.concatenate([counts, m[:, None]], axis=1).astype(np.int32)
    return dict(fpfh=out, spfh=spfh, members=idx, bar=bar, undecided=undecided)


# ---- nearest feature -----------------------------------------------------------------------------------------------------------
def match_features(fa, fb):
    """(index int32 [n_a], d2 fp64 [n_a]): the minimum over (d2, index), d2 summed over the columns in order."""
    a = np.asarray(fa, np.float32).astype(np.float64)
    b = np.asarray(fb, np.float32).astype(np.float64)
    na, nb = len(a), len(b)
    if nb == 0:
        return np.full(na, -1, np.int32), np.full(na, np.inf)
    index = np.empty(na, np.int32)
    dist = np.empty(na, np.float64)
    step = max(1, (1 << 22) // max(nb, 1))
    for s in range(0, na, step):
        blk = a[s:s + step]
        d2 = np.zeros((len(blk), nb))
        for c in range(a.shape[1]):
            d = blk[:, c][:, None] - b[:, c][None, :]
            d2 += d * d
        j = np.argmin(d2, axis=1)                                  # the first minimum: the smaller index on a tie
        index[s:s + step] = j
        dist[s:s + step] = d2[np.arange(len(blk)), j]
    return index, dist


# ---- RANSAC --------------------------------------------------------------------------------------------------------------------
def mix(x):
    """the finaliser of MurmurHash3 on uint64 arrays (wrapping)"""
    x = np.asarray(x, U64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U64(33)
        x *= U64(0xFF51AFD7ED558CCD)
        x ^= x >> U64(33)
        x *= U64(0xC4CEB9FE1A85EC53)
        x ^= x >> U64(33)
    return x


def draws(seed, H, m):
    """int64 [H, 3]: the three correspondence numbers of every hypothesis"""
    h = np.arange(H, dtype=U64)
    out = np.empty((H, 3), np.int64)
    with np.errstate(over="ignore"):
        for j in range(3):
            out[:, j] = (mix(U64(int(seed) & (2 ** 64 - 1)) + GOLDEN * (U64(3) * h + U64(j + 1))) % U64(m)).astype(np.int64)
    return out


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def triad(p0, p1, p2):
    """(x, y, z [n, 3], ok): the frame of three points; ok false where it is degenerate"""
    with np.errstate(all="ignore"):
        e1, e2 = p1 - p0, p2 - p0
        x = e1 / np.sqrt(_dot3(e1, e1))[:, None]
        z = _cross(x, e2)
        lz = np.sqrt(_dot3(z, z))
        ok = lz > 0
        z = z / lz[:, None]
        y = _cross(z, x)
    return x, y, z, ok


def triad_pose(s, t):
    """s, t: [n, 3, 3] (hypothesis, point, axis).  (R [n, 3, 3], tr [n, 3], ok)"""
    xs, ys, zs, oks = triad(s[:, 0], s[:, 1], s[:, 2])
    xt, yt, zt, okt = triad(t[:, 0], t[:, 1], t[:, 2])
    with np.errstate(all="ignore"):
        R = (xt[:, :, None] * xs[:, None, :] + yt[:, :, None] * ys[:, None, :]) + zt[:, :, None] * zs[:, None, :]
        ms = ((s[:, 0] + s[:, 1]) + s[:, 2]) / 3.0
        mt = ((t[:, 0] + t[:, 1]) + t[:, 2]) / 3.0
        tr = mt - ((R[:, :, 0] * ms[:, None, 0] + R[:, :, 1] * ms[:, None, 1]) + R[:, :, 2] * ms[:, None, 2])
    return R, tr, oks & okt


def ransac(src, tgt, corr, hypotheses, max_dist, edge_ratio=0.9, seed=0):
    """dict: T, status, best_h, inliers, n_passed, m, counts int32 [H], undecided (scores within 1e-12 relative of max_dist^2, edge
    ratios within 1e-12 of the limit), on_threshold (scores exactly on it: they count and are decided)."""
    S = np.asarray(src, np.float32).astype(np.float64).reshape(-1, 3)
    G = np.asarray(tgt, np.float32).astype(np.float64).reshape(-1, 3)
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    m, H = len(corr), int(hypotheses)
    counts = np.full(H, -1, np.int32)
    out = dict(T=np.eye(4), status=2, best_h=-1, inliers=0, n_passed=0, m=m, counts=counts, undecided=0, on_threshold=0)
    if m == 0:
        return out
    a, b = S[corr[:, 0]], G[corr[:, 1]]
    d = draws(seed, H, m)
    ok = (d[:, 0] != d[:, 1]) & (d[:, 0] != d[:, 2]) & (d[:, 1] != d[:, 2])
    undecided = 0
    for u, v in ((0, 1), (1, 2), (2, 0)):
        es, et = a[d[:, v]] - a[d[:, u]], b[d[:, v]] - b[d[:, u]]
        ls, lt = np.sqrt(_dot3(es, es)), np.sqrt(_dot3(et, et))
        hi, lo = np.maximum(ls, lt), np.minimum(ls, lt)
        undecided += int((ok & (hi > 0) & (np.abs(lo - edge_ratio * hi) <= 1e-12 * hi)).sum())
        ok &= ~((hi == 0) | (lo < edge_ratio * hi))
    hs = np.nonzero(ok)[0]
    R, tr, okp = triad_pose(a[d[hs]], b[d[hs]])
    hs, R, tr = hs[okp], R[okp], tr[okp]
    md2 = float(max_dist) * float(max_dist)
    on_threshold = 0
    for n_, h in enumerate(hs):
        r = R[n_]
        ex = (((r[0, 0] * a[:, 0] + r[0, 1] * a[:, 1]) + r[0, 2] * a[:, 2]) + tr[n_, 0]) - b[:, 0]
        ey = (((r[1, 0] * a[:, 0] + r[1, 1] * a[:, 1]) + r[1, 2] * a[:, 2]) + tr[n_, 1]) - b[:, 1]
        ez = (((r[2, 0] * a[:, 0] + r[2, 1] * a[:, 1]) + r[2, 2] * a[:, 2]) + tr[n_, 2]) - b[:, 2]
        d2 = (ex * ex + ey * ey) + ez * ez
        counts[h] = int((d2 <= md2).sum())
        undecided += int(((np.abs(d2 - md2) <= 1e-12 * md2) & (d2 != md2)).sum())
        on_threshold += int((d2 == md2).sum())
    out.update(n_passed=len(hs), undecided=undecided, on_threshold=on_threshold)
    if len(hs):
        best = int(hs[np.argmax(counts[hs])])                     # the first maximum: the smaller h on a tie
        n_ = int(np.nonzero(hs == best)[0][0])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R[n_], tr[n_]
        out.update(T=T, status=1, best_h=best, inliers=int(counts[best]))
    return out


# ---- the recipe ----------------------------------------------------------------------------------------------------------------
def mutual_pairs(ab, ba):
    ia = np.arange(len(ab))
    has = ab >= 0
    mut = has.copy()
    mut[has] = ba[ab[has]] == ia[has]
    return has, mut


def recipe(src, src_normals, tgt, tgt_normals, k, radius, hypotheses, max_dist, seed=0, mutual=True, edge_ratio=0.9):
    """FPFH of both clouds from the given (already oriented) normals, matches both ways, the mutual filter with its 3 % fall-back,
    RANSAC.  The ransac dict with fs, ft, corr, n_mutual, mutual beside it."""
    fs, ft = fpfh(src, src_normals, k, radius), fpfh(tgt, tgt_normals, k, radius)
    ab, _ = match_features(fs["fpfh"], ft["fpfh"])
    ba, _ = match_features(ft["fpfh"], fs["fpfh"])
    has, mut = mutual_pairs(ab, ba)
    use = bool(mutual) and mut.sum() >= 0.03 * len(ab)
    keep = mut if use else has
    corr = np.stack([np.arange(len(ab))[keep], ab[keep]], axis=1).astype(np.int32)
    out = ransac(src, tgt, corr, hypotheses, max_dist, edge_ratio, seed)
    out.update(fs=fs, ft=ft, corr=corr, n_mutual=int(mut.sum()), mutual=use)
    return out


def orient_to_centroid(xyz, normals):
    """normals negated where they point away from the cloud's fp64 centroid"""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    n = np.asarray(normals, np.float32).astype(np.float64)
    c = p.mean(axis=0)
    s = np.where(((c - p) * n).sum(axis=1) < 0, -1.0, 1.0)
    return (n * s[:, None]).astype(np.float32)
