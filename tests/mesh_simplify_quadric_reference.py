"""Restatement of the quadric placement rules ("Quadric placement"): what tl3d_mesh_simplify_quadric must
give, bit for bit.  Cells, numbering, colours and triangles come from mesh_simplify_reference.simplify; the quadric terms are
exact integers (int64 products cut into 32-bit pieces for the sums, put together as Python ints); the solve runs in Python floats
(fp64) in the stated order.  No reference code exists; the rules are the project's own."""
import math

import numpy as np

import mesh_simplify_reference as msr

STEPS = 1024            # quadric steps per cell
SPAN = 3                # a corner contributes when its triangle stays within this many cells of it, per axis
REG = 2.0 ** -10        # what the pipeline passes
WORDS = ("A00", "A01", "A02", "A11", "A12", "A22", "b0", "b1", "b2")
_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def steps(q):
    """h = (q + 8192) >> 14, arithmetic: floor division by 2^14 after adding a half"""
    return (np.asarray(q, np.int64) + 8192) >> 14


def _wide_sum(idx, term, k):
    """per index the exact sum of the int64 terms, as Python ints: low 32 bits and the rest are summed apart"""
    lo, hi = np.zeros(k, np.int64), np.zeros(k, np.int64)
    np.add.at(lo, idx, term & 0xFFFFFFFF)
    np.add.at(hi, idx, term >> 32)
    return [(h << 32) + l for h, l in zip(hi.tolist(), lo.tolist())]


def quadric_sums(i, q, tris, vmap, k):
    """(sums [k][9] of Python ints in the order of WORDS, corners skipped): every corner of every triangle, seen from its own cell"""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    if not len(tris):
        return [[0] * 9 for _ in range(k)], 0
    h = steps(q)
    it, ht = i[tris], h[tris]                                        # [T, 3, 3]: corner, axis
    skipped, cl, n, d = 0, [], [], []
    for c in range(3):
        di = it - it[:, c:c + 1, :]
        ok = (np.abs(di) <= SPAN).all(axis=(1, 2))
        skipped += int((~ok).sum())
        p = (di * STEPS + ht)[ok]
        cl.append(vmap[tris[ok, c]])
        n.append(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]))     # int64, below 2^27
        d.append(-(n[-1] * p[:, 0]).sum(axis=1))                     # below 2^41
    cl, n, d = np.concatenate(cl), np.concatenate(n), np.concatenate(d)
    words = [_wide_sum(cl, n[:, a] * n[:, b], k) for a, b in _PAIRS]
    d_hi, d_lo = d >> 20, d & 0xFFFFF                                # d = d_hi 2^20 + d_lo: both products stay below 2^48
    for a in range(3):
        words.append([(s_hi << 20) + s_lo for s_hi, s_lo in zip(_wide_sum(cl, d_hi * n[:, a], k), _wide_sum(cl, d_lo * n[:, a], k))])
    return [list(w) for w in zip(*words)], skipped


def dbl(n):
    """|n| = hi 2^64 + lo: (double)hi * 2^64 + (double)lo, negated when n < 0"""
    m = -n if n < 0 else n
    d = float(m >> 64) * 18446744073709551616.0 + float(m & 0xFFFFFFFFFFFFFFFF)
    return -d if n < 0 else d


def solve(s, S, n, reg):
    """(x unclamped [3] in steps) of one cluster from its nine sums, the sums S of q and the member count; None: the mean rule"""
    A00, A01, A02, A11, A12, A22, b0, b1, b2 = s
    if A00 == 0 and A11 == 0 and A22 == 0:
        return None
    T = (dbl(A00) + dbl(A11)) + dbl(A22)
    m = [float(int(S[a])) / (float(int(n)) * 16384.0) for a in range(3)]
    K00, K01, K02 = dbl(A00) / T + reg, dbl(A01) / T, dbl(A02) / T
    K11, K12, K22 = dbl(A11) / T + reg, dbl(A12) / T, dbl(A22) / T + reg
    r0, r1, r2 = reg * m[0] - dbl(b0) / T, reg * m[1] - dbl(b1) / T, reg * m[2] - dbl(b2) / T
    c00, c01, c02 = K11 * K22 - K12 * K12, K02 * K12 - K01 * K22, K01 * K12 - K02 * K11
    c11, c12, c22 = K00 * K22 - K02 * K02, K01 * K02 - K00 * K12, K00 * K11 - K01 * K01
    det = (K00 * c00 + K01 * c01) + K02 * c02

    def div(a, b):                                                   # IEEE division also where Python raises
        try:
            return a / b
        except ZeroDivisionError:
            return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)
    x0, x1, x2 = div((c00 * r0 + c01 * r1) + c02 * r2, det), div((c01 * r0 + c11 * r1) + c12 * r2, det), div((c02 * r0 + c12 * r1) + c22 * r2, det)
    # one step of refinement with the same adjugate
    p0 = r0 - ((K00 * x0 + K01 * x1) + K02 * x2)
    p1 = r1 - ((K01 * x0 + K11 * x1) + K12 * x2)
    p2 = r2 - ((K02 * x0 + K12 * x1) + K22 * x2)
    return [x0 + div((c00 * p0 + c01 * p1) + c02 * p2, det), x1 + div((c01 * p0 + c11 * p1) + c12 * p2, det),
            x2 + div((c02 * p0 + c12 * p1) + c22 * p2, det)]


def clamp(x):
    """(x clamped to [0, 1024] per axis, any axis clamped); what is not a number becomes 0"""
    out, hit = [], False
    for v in x:
        if not v >= 0.0:
            v, hit = 0.0, True
        elif v > float(STEPS):
            v, hit = float(STEPS), True
        out.append(v)
    return out, hit


def simplify(xyz, rgb, tris, cell, origin=None, reg=REG, mean=None):
    """mesh_simplify_reference.simplify with quadric placement: (xyz, rgb, tris, info); info also has quadric_placed, clamped,
    corners_skipped and, for the tests of the rules themselves, sums ([K][9] Python ints), x (f64 [K,3] unclamped steps, NaN rows
    at the mean rule), cell_index (i64 [K,3]), S (i64 [K,3]) and n (i64 [K]).  mean: mesh_simplify_reference.simplify of the same
    arguments, where the caller has it already"""
    reg = float(reg)
    if not (math.isfinite(reg) and 0.0 < reg <= 1.0):
        raise ValueError("reg")
    pos, col, out_tris, info = mean if mean is not None else msr.simplify(xyz, rgb, tris, cell, origin)
    o = [0.0, 0.0, 0.0] if origin is None else [float(v) for v in origin]
    cell = float(cell)
    i, q = msr.cells(xyz, cell, origin)
    vmap = info["vert_map"].astype(np.int64)
    k = info["clusters"]
    n = np.bincount(vmap, minlength=k).astype(np.int64)
    S = np.zeros((k, 3), np.int64)
    np.add.at(S, vmap, q)
    ic = np.zeros((k, 3), np.int64)
    ic[vmap] = i
    sums, skipped = quadric_sums(i, q, tris, vmap, k)
    pos = pos.copy()
    xs = np.full((k, 3), np.nan)
    placed = clamped = 0
    for c in range(k):
        x = solve(sums[c], S[c], n[c], reg)
        if x is None:
            continue
        xs[c] = x
        x, hit = clamp(x)
        placed += 1
        clamped += 1 if hit else 0
        pos[c] = [np.float32(o[a] + (float(int(ic[c, a])) + x[a] / 1024.0) * cell) for a in range(3)]
    info = dict(info, quadric_placed=placed, clamped=clamped, corners_skipped=skipped, sums=sums, x=xs, cell_index=ic, S=S, n=n)
    return pos, col, out_tris, info
