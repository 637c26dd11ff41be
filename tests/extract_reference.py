"""numpy restatement of tl3d_extract, written from include/tl3d.h, DESIGN.md (record order, channel formats, arithmetic contracts)
and the header comment of kernels_extract.hip -- not from the kernel or from oracle/tl3d_oracle.c: orc_extract, and formulated
differently on purpose:

* it works on dense [nx, ny, nz] volumes (one per field), not on records;
* neighbours are shifted views of those volumes, not index arithmetic per record;
* every candidate point is found first, in any order; ONE final sort on (record index of the emitting voxel, axis) gives the
  output order;
* a crossing is two usable ends of opposite sign (no product), colours are integer floor divisions.

The rule, as documented:

  t(v) = sum / (weight * 32767.0): ONE IEEE fp64 division.  Every gate compares that quotient and carries no tolerance.
  centroid mode: a voxel with n >= max(1, min_count) points emits its centroid origin + (offset + i + (S + n/2) / (4096 n)) voxel
      per axis and the colour C // n.  With a TSDF channel and min_weight > 0 it must also have weight >= min_weight and
      |t| <= max_abs_tsdf.
  TSDF mode: mw = max(1, min_weight); a voxel is usable when weight >= mw and |t| < 0.98.  The edge from v to v + e_axis (inside the
      grid) emits when both ends are usable and their t have opposite signs (t = 0 has none).  The point is the centre of v,
      origin + (offset + i + 1/2) voxel, moved along the axis by frac voxel, frac = |t_a| / (|t_a| + |t_b|).  Colour: the mean colour
      of the nearer end (smaller |t|; the lower end v on a tie) if it holds points, else of the other end, else 128.
  Only voxels inside the core [lo, hi) emit (TSDF mode: the lower end v decides).  Points come in ascending record index of the
  emitting voxel, within a voxel in the order +x, +y, +z.

Two forms of the positions:
  "contract": the fp64 expression the library promises, evaluated by numpy in float64, operation by operation, rounded once to f32;
  "exact": the same quantity in exact integer arithmetic (origin and voxel size taken as the exact values of their doubles, t as
      the exact ratio sum / (32767 weight)), rounded ONCE to f32, half to even.
"""
from fractions import Fraction

import numpy as np

QSCALE = 32767
FRAC_ONE = 4096
BAND = 0.98
MASK32 = np.uint64(0xffffffff)
FIELDS_TSDF = ("sum", "weight")
FIELDS_CENTROID = ("n", "px", "py", "pz", "cr", "cg", "cb")


# ---- layout: DESIGN.md "Record order" ----------------------------------------------------------------------------------------
def record_index(dims):
    """int64 [nx, ny, nz]: the record index of every voxel.  Bricks of 8^3 voxels, x fastest; a brick is eight sub-bricks of 4^3
    voxels, numbered x>>2 | (y>>2)<<1 | (z>>2)<<2, of 64 consecutive records each, x fastest inside a sub-brick."""
    nx, ny, nz = (int(d) for d in dims)
    assert nx % 8 == 0 and ny % 8 == 0 and nz % 8 == 0, dims
    i = np.arange(nx, dtype=np.int64)[:, None, None]
    j = np.arange(ny, dtype=np.int64)[None, :, None]
    k = np.arange(nz, dtype=np.int64)[None, None, :]
    brick = ((k // 8) * (ny // 8) + (j // 8)) * (nx // 8) + (i // 8)
    sub = (i // 4) % 2 + 2 * ((j // 4) % 2) + 4 * ((k // 4) % 2)
    cell = i % 4 + 4 * (j % 4) + 16 * (k % 4)
    return np.ascontiguousarray(np.broadcast_to(512 * brick + 64 * sub + cell, (nx, ny, nz)))


def volumes_from_records(dims, tsdf=None, centroid=None):
    """dict of int64 [nx, ny, nz] volumes from record-ordered channel images ({sum, weight} int32 pairs; four uint64 words
    {sx | sy<<32, sz | n<<32, sr | sg<<32, sb})"""
    ridx = record_index(dims)
    vol = {}
    if tsdf is not None:
        rec = np.asarray(tsdf).reshape(-1, 2)
        assert len(rec) == ridx.size
        vol["sum"] = rec[:, 0].astype(np.int64)[ridx]
        vol["weight"] = rec[:, 1].astype(np.int64)[ridx]
    if centroid is not None:
        rec = np.asarray(centroid, dtype=np.uint64).reshape(-1, 4)
        assert len(rec) == ridx.size
        lo = lambda w: (rec[:, w] & MASK32).astype(np.int64)[ridx]
        hi = lambda w: (rec[:, w] >> np.uint64(32)).astype(np.int64)[ridx]
        vol.update(px=lo(0), py=hi(0), pz=lo(1), n=hi(1), cr=lo(2), cg=hi(2), cb=lo(3))
        assert not (rec[:, 3] >> np.uint64(32)).any(), "the fourth word holds the blue sum alone"
    return vol


def records_from_volumes(vol):
    """(tsdf int32 [N, 2] or None, centroid uint64 [N, 4] or None) in record order"""
    some = vol["sum"] if "sum" in vol else vol["n"]
    ridx = record_index(some.shape).ravel()
    tsdf = cen = None
    if "sum" in vol:
        assert np.abs(vol["sum"]).max() < 2 ** 31 and 0 <= vol["weight"].min() and vol["weight"].max() < 2 ** 31
        tsdf = np.empty((ridx.size, 2), np.int32)
        tsdf[ridx, 0] = vol["sum"].ravel()
        tsdf[ridx, 1] = vol["weight"].ravel()
    if "n" in vol:
        for f in FIELDS_CENTROID:
            assert 0 <= vol[f].min() and vol[f].max() < 2 ** 32, f
        u = lambda f: vol[f].ravel().astype(np.uint64)
        cen = np.empty((ridx.size, 4), np.uint64)
        cen[ridx, 0] = u("px") | (u("py") << np.uint64(32))
        cen[ridx, 1] = u("pz") | (u("n") << np.uint64(32))
        cen[ridx, 2] = u("cr") | (u("cg") << np.uint64(32))
        cen[ridx, 3] = u("cb")
    return tsdf, cen


# ---- exact rounding ---------------------------------------------------------------------------------------------------------
def round_ratio_f32(num, den):
    """num / den (Python integers, den > 0) as the nearest float32, halves to even; exact for every finite result"""
    if num == 0:
        return 0.0
    neg, num = num < 0, abs(num)
    e = num.bit_length() - den.bit_length() - 24          # 2^23 <= num / (den 2^e) < 2^25
    for _ in range(2):
        e = max(e, -149)                                   # the subnormal grid
        a, b = (num, den << e) if e >= 0 else (num << -e, den)
        q, r = divmod(a, b)
        if q < 1 << 24:
            break
        e += 1
    if 2 * r > b or (2 * r == b and q & 1):
        q += 1
    v = float(q) * 2.0 ** e                                # q <= 2^24: exact in a double, and a float32 value
    return -v if neg else v


def _ratio(x):
    f = Fraction(float(x))                                 # the exact value of the double
    return f.numerator, f.denominator


def _exact_coords(org, vs, whole, fnum, fden):
    """float32 [len] of org + (whole + fnum / fden) * vs, rounded once; whole, fnum, fden: lists of Python integers"""
    (on, od), (vn, vd) = _ratio(org), _ratio(vs)
    return np.array([round_ratio_f32(on * (d * vd) + (w * d + p) * vn * od, od * d * vd) for w, p, d in zip(whole, fnum, fden)],
                    np.float32).reshape(-1)


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def _quotient(vol):
    with np.errstate(invalid="ignore", divide="ignore"):
        return vol["sum"].astype(np.float64) / (vol["weight"].astype(np.float64) * float(QSCALE))


def _mean_colour(vol, at):
    n = np.maximum(vol["n"][at], 1)
    return np.stack([vol[f][at] // n for f in ("cr", "cg", "cb")], axis=-1)


def extract(vol, dims, origin, voxel, voxel_offset=(0, 0, 0), core=None, mode=0, min_count=1, min_weight=0, max_abs_tsdf=1.0,
            use_centroid=True, tsdf_channel=True, form="contract", details=False):
    """(xyz float32 [N, 3], rgb uint8 [N, 3]) as tl3d_extract defines them; with details, also a dict of per-point arrays:
    `record` (record index of the emitting voxel), `axis`, `voxel` [N, 3] and in TSDF mode `neighbour` [N, 3], `tie` (|t_a| == |t_b|)
    and `colour_from` (0 the nearer end, 1 the other end, 2 neither: grey)."""
    assert form in ("contract", "exact") and mode in (0, 1)
    dims = tuple(int(d) for d in dims)
    off = [int(o) for o in voxel_offset]
    ridx = record_index(dims)
    own = np.ones(dims, bool)
    if core is not None:
        lo, hi = core
        own[:] = False
        own[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    has_cen = use_centroid and "n" in vol
    t = _quotient(vol) if (tsdf_channel and "sum" in vol) else None

    if mode == 0:
        assert has_cen, "centroid mode needs the centroid channel"
        keep = own & (vol["n"] >= max(1, int(min_count)))
        if t is not None and min_weight > 0:
            keep &= (vol["weight"] >= int(min_weight)) & (np.abs(t) <= float(max_abs_tsdf))
        where = np.nonzero(keep)
        rec = ridx[where]
        axis = np.zeros(len(rec), np.int64)
        nb = None
    else:
        assert t is not None, "TSDF mode needs the TSDF channel"
        usable = (vol["weight"] >= max(1, int(min_weight))) & (np.abs(t) < BAND)
        neg, pos = usable & (t < 0.0), usable & (t > 0.0)
        parts = []
        for a in range(3):
            lo_ = tuple(slice(0, -1) if q == a else slice(None) for q in range(3))      # the lower ends of this axis' edges
            hi_ = tuple(slice(1, None) if q == a else slice(None) for q in range(3))    # the same edges' upper ends
            cross = own[lo_] & ((neg[lo_] & pos[hi_]) | (pos[lo_] & neg[hi_]))
            w = np.nonzero(cross)
            parts.append((w, ridx[lo_][cross], np.full(len(w[0]), a, np.int64)))
        where = tuple(np.concatenate([p[0][q] for p in parts]) for q in range(3))
        rec = np.concatenate([p[1] for p in parts])
        axis = np.concatenate([p[2] for p in parts])

    order = np.lexsort((axis, rec))                                                     # by record index, then axis
    where, rec, axis = tuple(w[order] for w in where), rec[order], axis[order]
    n_out = len(rec)
    xyz = np.empty((n_out, 3), np.float32)
    info = dict(record=rec, axis=axis, voxel=np.stack(where, axis=-1) if n_out else np.zeros((0, 3), np.int64))

    if mode == 0:
        n = vol["n"][where]
        for a, f in enumerate(("px", "py", "pz")):
            s = vol[f][where]
            if form == "contract":
                frac = (s.astype(np.float64) + 0.5 * n.astype(np.float64)) / (n.astype(np.float64) * float(FRAC_ONE))
                xyz[:, a] = (float(origin[a]) + ((float(off[a]) + where[a].astype(np.float64)) + frac) * float(voxel)).astype(np.float32)
            else:                                            # (S + n/2) / (4096 n) = (2 S + n) / (8192 n)
                xyz[:, a] = _exact_coords(origin[a], voxel, (where[a] + off[a]).tolist(), (2 * s + n).tolist(),
                                          (2 * FRAC_ONE * n).tolist())
        rgb = _mean_colour(vol, where).astype(np.uint8)
    else:
        nb = tuple(where[q] + (axis == q) for q in range(3))
        ra, rb = np.abs(t[where]), np.abs(t[nb])
        for a in range(3):
            on_axis = axis == a
            if form == "contract":
                centre = float(origin[a]) + ((float(off[a]) + where[a].astype(np.float64)) + 0.5) * float(voxel)
                with np.errstate(invalid="ignore"):
                    moved = centre + (ra / (ra + rb)) * float(voxel)
                xyz[:, a] = np.where(on_axis, moved, centre).astype(np.float32)
            else:
                # centres: one exact value per lattice index; crossings: frac = |S_a| w_b / (|S_a| w_b + |S_b| w_a)
                line = _exact_coords(origin[a], voxel, [off[a] + i for i in range(dims[a])], [1] * dims[a], [2] * dims[a])
                col = line[where[a]]
                e = np.nonzero(on_axis)[0]
                ew, en = tuple(w[e] for w in where), tuple(w[e] for w in nb)
                pa = [abs(s) * w for s, w in zip(vol["sum"][ew].tolist(), vol["weight"][en].tolist())]
                pb = [abs(s) * w for s, w in zip(vol["sum"][en].tolist(), vol["weight"][ew].tolist())]
                col[e] = _exact_coords(origin[a], voxel, (ew[a] + off[a]).tolist(), [2 * x + (x + y) for x, y in zip(pa, pb)],
                                       [2 * (x + y) for x, y in zip(pa, pb)])
                xyz[:, a] = col
        tie = ra == rb
        colour_from = np.full(n_out, 2, np.int64)
        rgb = np.full((n_out, 3), 128, np.int64)
        if has_cen:
            first_is_v = ra <= rb
            near = tuple(np.where(first_is_v, where[q], nb[q]) for q in range(3))
            far = tuple(np.where(first_is_v, nb[q], where[q]) for q in range(3))
            n_near, n_far = vol["n"][near], vol["n"][far]
            colour_from = np.where(n_near > 0, 0, np.where(n_far > 0, 1, 2))
            rgb = np.where((colour_from == 0)[:, None], _mean_colour(vol, near),
                           np.where((colour_from == 1)[:, None], _mean_colour(vol, far), 128))
        rgb = rgb.astype(np.uint8)
        info.update(neighbour=np.stack(nb, axis=-1) if n_out else np.zeros((0, 3), np.int64), tie=tie, colour_from=colour_from)
    return (xyz, rgb, info) if details else (xyz, rgb)
