"""The TSDF update rule in exact rational arithmetic -- independent of both f32 formulations (oracle/tl3d_oracle.c and
oracle/second_numpy.py), for the DYADIC frames of tsdf_edges_common only (R a signed axis permutation, every length a multiple of
2^-24).

The rule, with no rounding anywhere:
    voxel centre x = origin + (i + 1/2) voxel;  camera point (xc, yc, zc) = R x + t;  only zc > 0;
    u = fx xc / zc + cx;  in the window iff -1/2 <= u < W - 1/2 (same for v);  pixel = floor(u + 1/2);
    d = depth[pixel] * scale, valid iff min < d < max;  sdf = d - zc;  update iff sdf >= -trunc;
    q = round_half_even(32767 min(1, sdf / trunc));  record += (q, 1).
Lengths are INTEGERS in units of 2^-24 (fractions.Fraction turns every float into its exact value and checks that it is such a
multiple), pixels and q come from integer floor divisions.

The f32 sequence of the contract decides as this model does wherever its roundings cannot reach a decision.  integrate() says where
that is PROVEN, per voxel (its second result):
  * zc is a power of two and u, v are f32 numbers: 1 / zc, the product and the fma are exact, ties and borders included; or
    u + 1/2 and v + 1/2 are at least 2^-10 px from an integer with |u - cx|, |v - cy| <= 2^10 (f32 error below 2^-11 px), or the
    pixel coordinate lies more than a pixel outside the window;
  * d = raw * scale and sdf = d - zc are f32 numbers (the subtraction is exact);
  * 32767 tsdf is an f32 number, or at least 2^-9 from a half-integer: tsdf = 8 sdf is exact and |32767 tsdf| < 2^15, so the
    f32 product is within half an ulp = 2^-10 of the exact one and rint() sees the same side.  (2^-6 would do for most of the
    family, but the f32 neighbour of 0.875 under the zc = 0.8125 slice gives 16383.5 - 0.0156245: a voxel worth comparing.)
A voxel outside these cases is EXCLUDED from the comparison (a condition, not a tolerance); tests/test_tsdf_edges_reference_cpu.py
pins the number of exclusions at zero for every frame before it compares anything.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

UNIT_BITS = 24
UNIT = 1 << UNIT_BITS


def _units(x, what):
    """the float x as an integer number of 2^-24"""
    f = Fraction(float(x)) * UNIT
    assert f.denominator == 1, f"{what} = {x!r} is not a multiple of 2^-24"
    return int(f.numerator)


def _is_f32(n):
    """the int64 values n (times any power of two) are float32 numbers: at most 24 significant bits"""
    n = np.abs(np.asarray(n, np.int64))
    low = n & -n                                        # lowest set bit (0 for 0)
    return (n == 0) | (n < low * (1 << 24))


def _pow2(n):
    n = np.asarray(n, np.int64)
    return (n > 0) & ((n & (n - 1)) == 0)


def _camera_points(case):
    R = np.asarray(case.R, float)
    assert np.array_equal(np.abs(R).sum(0), np.ones(3)) and np.array_equal(np.abs(R).sum(1), np.ones(3)) and set(np.unique(R)) <= {-1.0, 0.0, 1.0}, \
        "the rational model takes signed axis permutations only"
    from tsdf_edges_common import VOXEL
    half_voxel = _units(VOXEL / 2, "voxel / 2")
    w = [_units(case.origin[a], "origin") + (2 * np.arange(case.dims[a], dtype=np.int64) + 1) * half_voxel for a in range(3)]
    K, J, I = np.meshgrid(np.arange(case.dims[2]), np.arange(case.dims[1]), np.arange(case.dims[0]), indexing="ij")
    W3 = (w[0][I], w[1][J], w[2][K])
    Ri = R.astype(np.int64)
    cam = [Ri[a, 0] * W3[0] + Ri[a, 1] * W3[1] + Ri[a, 2] * W3[2] + _units(case.t[a], "t") for a in range(3)]
    return I, J, K, cam


def _axis(f, c, n, X, Z):
    """pixel coordinate p = f X / Z + c along one axis for Z > 0: (in window, pixel, provably decided as in f32)"""
    f2, c2 = Fraction(f) * 2, Fraction(c) * 2 + 1
    assert f2.denominator == 1 and c2.denominator == 1
    f2, c2 = int(f2), int(c2)
    Zs = np.where(Z > 0, Z, 1)
    A, B = f2 * X + c2 * Zs, 2 * Zs                      # p + 1/2 = A / B
    pix = A // B
    inwin = (A >= 0) & (A < n * B)
    rem = A - pix * B
    # p itself = (A - Zs) / B as an f32 number: numerator with at most 24 significant bits once B = 2^k is divided out
    # (and so is p + 1/2, which the pixel is the floor of)
    exact = _pow2(Zs) & _is_f32(A - Zs) & _is_f32(A)
    far_out = (A < -B) | (A >= (n + 1) * B)
    modest = np.abs(A - c2 * Zs) <= (1 << 10) * B
    clear = modest & (np.minimum(rem, B - rem) * (1 << 10) >= B)
    return inwin, pix, exact | far_out | clear


def integrate(case, grid=None):
    """(grid int32 [nvox, 2] in record order, applies bool [nvox] in record order)"""
    from oracle.second_numpy import record_index
    from tsdf_edges_common import MIN_DEPTH, MAX_DEPTH, TRUNC
    assert case.dyadic
    nx, ny, nz = case.dims
    nvox = nx * ny * nz
    if grid is None:
        grid = np.zeros((nvox, 2), np.int32)
    I, J, K, (X, Y, Z) = _camera_points(case)
    front = Z > 0
    c = case.cam
    u_in, u, u_ok = _axis(c["fx"], c["cx"], c["width"], X, Z)
    v_in, v, v_ok = _axis(c["fy"], c["cy"], c["height"], Y, Z)
    win = front & u_in & v_in
    # out of the window along ONE axis, provably, settles the voxel whatever the other axis does
    geo_ok = ~front | (u_ok & v_ok) | (u_ok & ~u_in) | (v_ok & ~v_in)
    # the image: every pixel's d = raw * scale as an exact rational; valid iff min < d < max; then in units
    H, Wd = case.depth.shape
    D = np.zeros((H, Wd), np.int64)
    valid = np.zeros((H, Wd), bool)
    d_ok = np.ones((H, Wd), bool)
    sc = Fraction(float(case.scale))
    for (r, col), raw in np.ndenumerate(case.depth):
        if not np.isfinite(raw):
            continue
        d = Fraction(float(raw)) * sc
        if Fraction(MIN_DEPTH) < d < Fraction(MAX_DEPTH):
            valid[r, col] = True
            du = d * UNIT
            if du.denominator != 1 or float(np.float32(float(d))) != d:
                d_ok[r, col] = False                     # raw * scale rounds in f32: not this model's business
            else:
                D[r, col] = int(du)
    uu, vv = np.where(win, u, 0), np.where(win, v, 0)
    ok = win & valid[vv, uu]
    T = _units(TRUNC, "trunc")
    assert T & (T - 1) == 0, "1 / trunc must be exact"
    S = D[vv, uu] - Z                                    # sdf
    upd = ok & (S >= -T)
    N = 32767 * np.minimum(S, T)                         # q = round_half_even(N / T)
    Q = N // T
    r = N - Q * T
    q = Q + ((2 * r > T) | ((2 * r == T) & (Q % 2 != 0)))
    val_ok = ~ok | (d_ok[vv, uu] & _is_f32(S) & (~upd | _is_f32(N) | (np.abs(2 * r - T) * (1 << 9) >= 2 * T)))
    rec = record_index(I, J, K, nx // 8, ny // 8)
    grid[rec[upd], 0] += q[upd].astype(np.int32)
    grid[rec[upd], 1] += 1
    applies = np.zeros(nvox, bool)
    applies[rec.ravel()] = (geo_ok & val_ok).ravel()
    return grid, applies
