"""Crafted clouds and frames, and an integer model of voxel-centroid accumulation (include/tl3d.h: tl3d_accumulate_points,
tl3d_accumulate_centroid, tl3d_count_bricks, tl3d_points_bounds), for the CPU and the GPU tests.

numpy and Python integers only.  The model is written from the documented rule (tl3d.h, DESIGN.md sections 3 and 5, the header
comment of kernels_centroid.hip), not from the kernel:

  voxel     v = floor((float64(p) - origin) / voxel) per axis, in fp64 from the f32 point; the point has a voxel when v - offset
            lies in [0, dims) on every axis (a NaN or an infinite coordinate has none)
  offset    q = min(int(((p - origin) / voxel - v) * 4096), 4095): the in-voxel position in units of voxel / 4096
  record    uint64 {sx | sy << 32, sz | n << 32, sr | sg << 32, sb}: the SUMS of q and of the colour bytes over the voxel's points
            and their count n; every field stays below 2^32 while a voxel holds at most 2^20 points (2^20 x 4095 < 2^32)
  order     brick-major: 8^3 bricks x fastest; in a brick eight 4^3 sub-bricks (x>>2 | (y>>2)<<1 | (z>>2)<<2) of 64 records, x fastest
  counts    centroid_points = points whose voxel lies in the block core (the whole grid without a core), centroid_dropped =
            all other points of the list (for a frame: all other VALID samples)

Here every field is summed on its own in int64 volumes [nx, ny, nz]; the four words are packed once at the end, and the record
order is a reshape and a transpose of those volumes.

Is the clamp `q > 4095 -> 4095` reachable?  Not with voxel_offset >= 0 (the library refuses a negative offset).  A point with a
voxel has v >= offset >= 0, so rc = (p - origin) / voxel >= 0 and v = floor(rc) <= rc.  rc and v are both multiples of ulp(rc), so
rc - v is a non-negative multiple of ulp(rc) below 1 with no more significant bits than rc: the subtraction is exact and at most
1 - 2^-53.  Times 4096 is a change of exponent: at most 4096 - 2^-41 < 4096, whose integer part is at most 4095.  (For rc < 0 the
difference can round up to 1.0 -- rc = -2^-60 gives v = -1, rc - v = 1.0, q = 4096 -- but then v - offset < 0: no voxel.)  The
`faces` list holds the closest approaches: the f32 just below every voxel and grid face, where q = 4095 unclamped.

Lane control: centroid_points_kernel puts point i on lane i & 63 of wave (i >> 6) & 3 of workgroup i >> 8, and runs of equal
voxels are summed inside rows of 16 lanes (i >> 4), so the ORDER of a list decides what the on-chip scan sees.  `Lanes` builds a
list position by position, and `row_runs` reports the runs a list really contains, for the builders' own assertions.
"""
import functools

import numpy as np

FRAC = 4096
N_LIMIT = 1 << 20
FIELDS = ("n", "px", "py", "pz", "cr", "cg", "cb")          # the names tests/extract_reference.py uses
FIELD_MAX = dict(n=1, px=FRAC - 1, py=FRAC - 1, pz=FRAC - 1, cr=255, cg=255, cb=255)   # per point
S32 = np.uint64(32)
INVALID_KINDS = ("out", "nan", "pinf", "ninf")

# dyadic geometry: every axis differs; origin y = 0 so that -0.0 and +0.0 lie on a grid face
GEO = dict(dims=(32, 24, 40), origin=(-0.5, 0.0, 0.25), voxel=1.0 / 32)
GEO_TOUCH = dict(dims=(48, 32, 40), origin=(-0.75, 0.0, 0.5), voxel=1.0 / 32)      # 6 x 4 x 5 = 120 bricks
BLOCK_OFFSET = (8, 16, 24)
assert N_LIMIT * (FRAC - 1) == 4293918720 < 1 << 32 and N_LIMIT * 255 < 1 << 32


# ---- the model ------------------------------------------------------------------------------------------------------------------
def to_record_order(vol):
    """[nx, ny, nz] -> [nx ny nz] in record order, by reshapes alone"""
    nx, ny, nz = vol.shape
    v = vol.transpose(2, 1, 0).reshape(nz // 8, 2, 4, ny // 8, 2, 4, nx // 8, 2, 4)       # bz sz cz  by sy cy  bx sx cx
    return np.ascontiguousarray(v.transpose(0, 3, 6, 1, 4, 7, 2, 5, 8)).reshape(-1)        # brick (z y x), sub-brick, cell


def point_voxels(points_f32, origin, voxel, offset=(0, 0, 0), dims=None):
    """(loc int64 [n, 3], q int64 [n, 3], ok bool [n]): the grid-local voxel, the in-voxel offset and `has a voxel` of every point"""
    p = np.asarray(points_f32)
    assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 3
    with np.errstate(invalid="ignore", over="ignore"):
        rc = (p.astype(np.float64) - np.asarray(origin, np.float64)) / np.float64(voxel)
        fl = np.floor(rc)
        fin = np.isfinite(rc).all(axis=1)
        fl0, rc0 = np.where(fin[:, None], fl, 0.0), np.where(fin[:, None], rc, 0.0)
        loc = fl0.astype(np.int64) - np.asarray(offset, np.int64)
        q = np.minimum(((rc0 - fl0) * FRAC).astype(np.int64), FRAC - 1)
    ok = fin & (loc >= 0).all(axis=1)
    if dims is not None:
        ok &= (loc < np.asarray(dims, np.int64)).all(axis=1)
    return loc, q, ok


def model_volumes(points_f32, rgb_u8, dims, origin, voxel, offset=(0, 0, 0), core=None):
    """({field: int64 [nx, ny, nz]}, n_core, n_dropped): seven sums per voxel, each on its own"""
    dims = tuple(int(d) for d in dims)
    assert all(d % 8 == 0 for d in dims)
    loc, q, ok = point_voxels(points_f32, origin, voxel, offset, dims)
    c = np.asarray(rgb_u8)
    assert c.dtype == np.uint8 and c.shape == loc.shape
    at = tuple(loc[ok].T)
    per_point = dict(n=np.ones(int(ok.sum()), np.int64), px=q[ok, 0], py=q[ok, 1], pz=q[ok, 2],
                     cr=c[ok, 0].astype(np.int64), cg=c[ok, 1].astype(np.int64), cb=c[ok, 2].astype(np.int64))
    vol = {}
    for f in FIELDS:
        vol[f] = np.zeros(dims, np.int64)
        np.add.at(vol[f], at, per_point[f])
    lo, hi = ((0, 0, 0), dims) if core is None else core
    in_core = ok & (loc >= np.asarray(lo)).all(axis=1) & (loc < np.asarray(hi)).all(axis=1)
    return vol, int(in_core.sum()), int((~ok).sum())


def records_from_volumes(vol):
    """uint64 [n_vox, 4] in record order; every field must fit its 32 bits"""
    for f in FIELDS:
        assert 0 <= int(vol[f].min()) and int(vol[f].max()) < 1 << 32, (f, int(vol[f].max()))
    u = lambda f: to_record_order(vol[f]).astype(np.uint64)
    return np.stack([u("px") | (u("py") << S32), u("pz") | (u("n") << S32), u("cr") | (u("cg") << S32), u("cb")], axis=1)


def touched_bricks(vol):
    return int((to_record_order(vol["n"]).reshape(-1, 512) != 0).any(axis=1).sum())


def add_volumes(*vols, times=None):
    """the field-wise sum of models (times: how often each is taken)"""
    times = times or [1] * len(vols)
    return {f: sum(int(t) * v[f] for t, v in zip(times, vols)) for f in FIELDS}


def model_accumulate(points_f32, rgb_u8, dims, origin, voxel, offset=(0, 0, 0), core=None):
    """(records uint64 [n_vox, 4] in record order, n_core, n_dropped, touched_bricks)"""
    vol, n_core, n_dropped = model_volumes(points_f32, rgb_u8, dims, origin, voxel, offset, core)
    return records_from_volumes(vol), n_core, n_dropped, touched_bricks(vol)


# ---- what the on-chip scan sees ---------------------------------------------------------------------------------------------------
def point_keys(xyz, geo):
    """int64 [n]: a number per point that is equal for equal voxels, -1 without a voxel"""
    loc, _, ok = point_voxels(xyz, geo["origin"], geo["voxel"], (0, 0, 0), geo["dims"])
    d = geo["dims"]
    return np.where(ok, (loc[:, 0] * d[1] + loc[:, 1]) * d[2] + loc[:, 2], -1)


def row_runs(keys):
    """[(first index, length, key)]: the maximal runs of equal keys inside rows of 16 consecutive positions (-1 included)"""
    keys = np.asarray(keys)
    n = len(keys)
    head = np.ones(n, bool)
    head[1:] = (keys[1:] != keys[:-1]) | (np.arange(1, n) % 16 == 0)
    first = np.flatnonzero(head)
    length = np.diff(np.append(first, n))
    return [(int(i), int(l), int(keys[i])) for i, l in zip(first, length)]


# ---- list building ----------------------------------------------------------------------------------------------------------------
def voxel_point(geo, ijk, q=(0, 0, 0)):
    """the f32 point at in-voxel offset q / 4096 of voxel ijk: exact on the dyadic geometries"""
    v = [geo["origin"][a] + (ijk[a] + q[a] / FRAC) * geo["voxel"] for a in range(3)]
    out = np.array(v, np.float32)
    assert (out.astype(np.float64) == np.array(v, np.float64)).all(), (ijk, q)
    return out


def invalid_point(geo, kind, k):
    """a point without a voxel; k varies the axis that makes it so (the other two coordinates lie inside the grid)"""
    p = voxel_point(geo, (3, 5, 7), (k * 97 % FRAC, 11, 4000))
    a = k % 3
    p[a] = dict(out=(geo["origin"][a] - geo["voxel"], geo["origin"][a] + (geo["dims"][a] + 2) * geo["voxel"])[(k // 3) % 2],
                nan=np.nan, pinf=np.inf, ninf=-np.inf)[kind]
    return p


class Lanes:
    """a point list built position by position.  Fillers are single points of two alternating voxels that no run uses."""

    def __init__(self, geo, seed, fill=((1, 1, 1), (30, 22, 38))):
        self.geo, self.rng, self.fill = geo, np.random.default_rng(seed), fill
        self.xyz, self.rgb = [], []

    def __len__(self):
        return len(self.xyz)

    def point(self, ijk, q=None, rgb=None):
        q = self.rng.integers(0, FRAC, 3) if q is None else q
        self.xyz.append(voxel_point(self.geo, ijk, q))
        self.rgb.append(self.rng.integers(0, 256, 3) if rgb is None else rgb)

    def raw(self, p, rgb=None):
        self.xyz.append(np.asarray(p, np.float32))
        self.rgb.append(self.rng.integers(0, 256, 3) if rgb is None else rgb)

    def invalid(self, kind, k=None):
        self.raw(invalid_point(self.geo, kind, len(self) if k is None else k))

    def run(self, ijk, length, q=None, rgb=None):
        assert tuple(ijk) not in self.fill
        for _ in range(length):
            self.point(ijk, q, rgb)

    def filler(self, n=1):
        for _ in range(n):
            self.point(self.fill[len(self) % 2])

    def pad_to(self, multiple, plus=0):
        self.filler((-len(self)) % multiple + plus)

    def arrays(self):
        return np.array(self.xyz, np.float32).reshape(-1, 3), np.array(self.rgb, np.uint8).reshape(-1, 3)


def _run_voxel(geo, i):
    """a voxel for the i-th run: spread over bricks and sub-bricks, never a filler voxel, consecutive ones distinct"""
    d = geo["dims"]
    return (2 + (5 * i) % (d[0] - 4), 2 + (7 * i) % (d[1] - 4), 2 + (11 * i) % (d[2] - 4))


def _case(name, geo, lanes_or_arrays, edges):
    xyz, rgb = lanes_or_arrays.arrays() if isinstance(lanes_or_arrays, Lanes) else lanes_or_arrays
    missing = [k for k, v in edges.items() if not v]
    assert not missing, (name, "edges the builder could not place", missing)
    xyz.setflags(write=False)
    rgb.setflags(write=False)
    return dict(name=name, geo=geo, xyz=xyz, rgb=rgb, edges=edges)


LS_PAIRS = [(L, s) for L in range(1, 17) for s in range(0, 17 - L)]


def list_faces():
    """points on voxel faces and grid faces, one f32 either side, +-0, and in-voxel offsets j / 4096 and one ulp either side"""
    geo, ln = GEO, Lanes(GEO, 11)
    f32 = np.float32
    placed = dict(lower_face_kept=0, upper_face_dropped=0, below_lower_dropped=0, below_upper_kept=0, minus_zero=0, plus_zero=0,
                  q_exact=0, q_below=0)
    mid = (13, 9, 21)
    for a in range(3):
        d = geo["dims"][a]
        for k in (0, 1, 7, 8, d - 1, d):
            c = f32(geo["origin"][a] + k * geo["voxel"])
            assert float(c) == geo["origin"][a] + k * geo["voxel"]
            for x in (np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))):
                p = voxel_point(geo, mid, (5, 6, 7))
                p[a] = x
                ln.raw(p)
        for j in (0, 1, FRAC - 1):
            c = voxel_point(geo, (3, 3, 3), (j, j, j))[a]
            for x in (np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))):
                p = voxel_point(geo, mid, (9, 8, 7))
                p[a] = x
                ln.raw(p)
        if geo["origin"][a] == 0.0:
            for z in (f32(-0.0), f32(0.0)):
                p = voxel_point(geo, mid, (1, 2, 3))
                p[a] = z
                ln.raw(p)
    xyz, rgb = ln.arrays()
    loc, q, ok = point_voxels(xyz, geo["origin"], geo["voxel"], (0, 0, 0), geo["dims"])
    for a in range(3):
        o, d, v = geo["origin"][a], geo["dims"][a], geo["voxel"]
        x = xyz[:, a].astype(np.float64)
        placed["lower_face_kept"] += int((ok & (x == o) & (loc[:, a] == 0) & (q[:, a] == 0)).sum())
        placed["upper_face_dropped"] += int((~ok & (x == o + d * v)).sum())
        placed["below_lower_dropped"] += int((~ok & (x < o) & (x > o - v / 1024)).sum())
        placed["below_upper_kept"] += int((ok & (x < o + d * v) & (loc[:, a] == d - 1) & (q[:, a] == FRAC - 1)).sum())
        placed["q_exact"] += int((ok & (loc[:, a] == 3) & np.isin(q[:, a], (0, 1, FRAC - 1)) & (x == o + (3 + q[:, a] / FRAC) * v)).sum())
        placed["q_below"] += int((ok & (loc[:, a] == 3) & (x < o + (3 + (FRAC - 1) / FRAC) * v) & (q[:, a] == FRAC - 2)).sum())
        if o == 0.0:
            placed["minus_zero"] += int((ok & (xyz[:, a] == 0) & np.signbit(xyz[:, a]) & (loc[:, a] == 0)).sum())
            placed["plus_zero"] += int((ok & (xyz[:, a] == 0) & ~np.signbit(xyz[:, a]) & (loc[:, a] == 0)).sum())
    edges = {k: n >= (1 if "zero" in k else 3) for k, n in placed.items()}
    return _case("faces", geo, (xyz, rgb), edges)


def _runs_body(ln, geo, invalid=False):
    """one row of 16 lanes per (L, s): voxel V on lanes [s, s + L), fillers elsewhere.  invalid: three rows per pair, with a point
    that has no voxel just before the run, just after it and inside it (splitting it), the kind cycling"""
    n_kind = 0
    placements = {(k, w): 0 for k in INVALID_KINDS for w in ("before", "after", "inside")}
    for i, (L, s) in enumerate(LS_PAIRS):
        for where in (("before", "after", "inside") if invalid else (None,)):
            if (where == "before" and s == 0) or (where == "after" and s + L == 16) or (where == "inside" and L < 3):
                continue
            ln.pad_to(16)
            V = _run_voxel(geo, i)
            kind = INVALID_KINDS[n_kind % 4]
            for lane in range(16):
                bad = where and lane == dict(before=s - 1, after=s + L, inside=s + L // 2)[where]
                if bad:
                    ln.invalid(kind, n_kind // 4)
                    placements[(kind, where)] += 1
                    n_kind += 1
                elif s <= lane < s + L:
                    ln.point(V)
                else:
                    ln.filler()
    return placements


def list_runs():
    geo, ln = GEO, Lanes(GEO, 22)
    _runs_body(ln, geo)
    marks = {}
    for name, lane in (("row_end", 12), ("wave_end", 60), ("workgroup_end", 252)):
        ln.pad_to(256, lane)
        marks[name] = len(ln)
        ln.run(_run_voxel(geo, 200 + lane), 8)
    ln.pad_to(64)
    marks["alternation"] = len(ln)
    for i in range(64):
        ln.point(((6, 6, 6), (6, 6, 7))[i % 2])
    marks["wave_of_one_voxel"] = len(ln)
    ln.run((20, 12, 30), 64)
    ln.filler(5)
    xyz, rgb = ln.arrays()
    keys = point_keys(xyz, geo)
    runs = {(i, l): k for i, l, k in row_runs(keys)}
    edges = {}
    for r, (L, s) in enumerate(LS_PAIRS):
        edges[f"L{L}_s{s}"] = (16 * r + s, L) in runs
    for name in ("row_end", "wave_end", "workgroup_end"):
        i = marks[name]                                              # lanes 12 .. 15 and 0 .. 3 of the next row: two runs, one voxel
        edges[name] = runs.get((i, 4), -2) == runs.get((i + 4, 4), -3) and (i + 4) % {"row_end": 16, "wave_end": 64, "workgroup_end": 256}[name] == 0
    a = marks["alternation"]
    edges["alternation"] = all((a + i, 1) in runs for i in range(64)) and len(set(keys[a:a + 64].tolist())) == 2
    w = marks["wave_of_one_voxel"]
    edges["wave_of_one_voxel"] = w % 64 == 0 and all((w + 16 * i, 16) in runs for i in range(4)) and len(set(keys[w:w + 64].tolist())) == 1
    return _case("runs", geo, (xyz, rgb), edges)


def list_packed_maxima():
    """rows of 16 lanes of one voxel: every field at its maximum, then one field at its maximum and the other six at 0"""
    geo, ln = GEO, Lanes(GEO, 33)
    rows = [("all",) + tuple(FIELDS[1:])] + [("only_" + f, f) for f in FIELDS]
    for r, (name, *at_max) in enumerate(rows):
        q = [FRAC - 1 if f in at_max else 0 for f in ("px", "py", "pz")]
        c = [255 if f in at_max else 0 for f in ("cr", "cg", "cb")]
        ln.run(_run_voxel(geo, 3 * r + 1), 16, q, c)
    for r, (name, *at_max) in enumerate(rows):                          # again in ONE voxel, back to back: the rows are runs of one key
        q = [FRAC - 1 if f in at_max else 0 for f in ("px", "py", "pz")]
        c = [255 if f in at_max else 0 for f in ("cr", "cg", "cb")]
        ln.run((17, 3, 29), 16, q, c)
    xyz, rgb = ln.arrays()
    edges = {name: True for name, *_ in rows}
    for r, (name, *at_max) in enumerate(rows):
        vol, _, _ = model_volumes(xyz[16 * r:16 * r + 16], rgb[16 * r:16 * r + 16], geo["dims"], geo["origin"], geo["voxel"])
        for f in FIELDS:
            want = 16 * FIELD_MAX[f] if (f == "n" or f in at_max) else 0
            edges[name] &= int(vol[f].sum()) == want and int(vol[f].max()) == want
    edges["sixteen_lane_runs"] = all(l == 16 for _, l, _ in row_runs(point_keys(xyz, geo)))
    return _case("packed_maxima", geo, (xyz, rgb), edges)


def list_invalid(tail):
    """the runs with points that have no voxel before, after and inside them; a whole wave of such points; a last wave of `tail` points"""
    geo, ln = GEO, Lanes(GEO, 44)
    placements = _runs_body(ln, geo, invalid=True)
    ln.pad_to(64)
    w = len(ln)
    for i in range(64):
        ln.invalid(INVALID_KINDS[i % 4], i // 4)
    ln.run((9, 9, 9), 64)
    for i in range(tail):                                                # the partial wave: a run cut by the end of the list
        if i % 8 == 7:
            ln.invalid(INVALID_KINDS[(i // 8) % 4], i)
        else:
            ln.point((10, 10, 10))
    xyz, rgb = ln.arrays()
    keys = point_keys(xyz, geo)
    edges = {f"{k}_{where}": n > 0 for (k, where), n in placements.items()}
    edges["whole_wave_invalid"] = w % 64 == 0 and (keys[w:w + 64] == -1).all()
    edges[f"tail_{tail}"] = len(xyz) % 64 == tail
    # `inside` really splits: an invalid position with the same voxel on both sides, in one row
    inside = [i for i in range(1, len(keys) - 1) if keys[i] == -1 and keys[i - 1] == keys[i + 1] != -1 and (i - 1) // 16 == (i + 1) // 16]
    kinds = {k: False for k in INVALID_KINDS}
    for i in inside:
        x = xyz[i]
        kinds["nan" if np.isnan(x).any() else "pinf" if (x == np.inf).any() else "ninf" if (x == -np.inf).any() else "out"] = True
    edges.update({f"{k}_splits_a_run": v for k, v in kinds.items()})
    return _case(f"invalid_tail{tail}", geo, (xyz, rgb), edges)


def _brick_point(ln, geo, brick, rng):
    nbx, nby = geo["dims"][0] // 8, geo["dims"][1] // 8
    b = (brick % nbx, brick // nbx % nby, brick // (nbx * nby))
    ijk = tuple(8 * b[a] + int(rng.integers(0, 8)) for a in range(3))
    return ijk


def list_first_touch():
    """a wave of 64 distinct bricks, then a wave whose 16 runs of 4 lanes end in 16 further bricks"""
    geo = GEO_TOUCH
    ln, rng = Lanes(geo, 55, fill=((0, 0, 0), (47, 31, 39))), np.random.default_rng(56)
    order = rng.permutation(64)
    for b in order:
        ln.point(_brick_point(ln, geo, int(b), rng))
    for b in range(64, 80):
        ln.run(_brick_point(ln, geo, b, rng), 4)
    xyz, rgb = ln.arrays()
    vol, _, _ = model_volumes(xyz, rgb, geo["dims"], geo["origin"], geo["voxel"])
    runs = row_runs(point_keys(xyz, geo))
    edges = dict(wave_of_64_bricks=touched_bricks(model_volumes(xyz[:64], rgb[:64], geo["dims"], geo["origin"], geo["voxel"])[0]) == 64,
                 sixteen_tails_in_new_bricks=[l for i, l, _ in runs if i >= 64] == [4] * 16 and touched_bricks(vol) == 80)
    return _case("first_touch", geo, (xyz, rgb), edges)


def list_one_brick():
    """20 000 points of one brick: about 80 workgroups meet at one first touch"""
    geo = GEO_TOUCH
    rng = np.random.default_rng(66)
    ijk = np.array([16, 8, 24]) + rng.integers(0, 8, size=(20000, 3))
    q = rng.integers(0, FRAC, size=(20000, 3))
    xyz = (np.array(geo["origin"]) + (ijk + q / FRAC) * geo["voxel"]).astype(np.float32)
    rgb = rng.integers(0, 256, size=(20000, 3)).astype(np.uint8)
    vol, _, dropped = model_volumes(xyz, rgb, geo["dims"], geo["origin"], geo["voxel"])
    edges = dict(one_brick=touched_bricks(vol) == 1 and dropped == 0, many_workgroups=len(xyz) // 256 >= 78)
    return _case("one_brick", geo, (xyz, rgb), edges)


def list_every_brick():
    geo = GEO_TOUCH
    ln, rng = Lanes(geo, 77), np.random.default_rng(78)
    nbr = geo["dims"][0] * geo["dims"][1] * geo["dims"][2] // 512
    for b in rng.permutation(nbr):
        ln.point(_brick_point(ln, geo, int(b), rng))
    xyz, rgb = ln.arrays()
    vol, _, _ = model_volumes(xyz, rgb, geo["dims"], geo["origin"], geo["voxel"])
    per_brick = to_record_order(vol["n"]).reshape(-1, 512).sum(axis=1)
    return _case("every_brick", geo, (xyz, rgb), dict(every_brick_once=len(xyz) == nbr == 120 and (per_brick == 1).all()))


def list_random():
    """a seeded cloud over the grid and a little beyond it (a fifth of it dropped): the blocks' halo and core see every region"""
    geo, rng = GEO, np.random.default_rng(88)
    d = np.array(geo["dims"])
    ijk = rng.integers(-2, d + 2, size=(6000, 3))
    q = rng.integers(0, FRAC, size=(6000, 3))
    xyz = (np.array(geo["origin"]) + (ijk + q / FRAC) * geo["voxel"]).astype(np.float32)
    xyz = np.repeat(xyz, rng.integers(1, 4, size=6000), axis=0)         # short runs
    rgb = rng.integers(0, 256, size=(len(xyz), 3)).astype(np.uint8)
    _, n_core, dropped = model_volumes(xyz, rgb, geo["dims"], geo["origin"], geo["voxel"], core=((8, 8, 8), tuple(d - 8)))
    return _case("random", geo, (xyz, rgb), dict(dropped=dropped > 500, core=0 < n_core < len(xyz) - dropped, halo=len(xyz) - dropped - n_core > 500))


# the largest grid the library takes: 2^32 voxels, so its last record has the index 0xffffffff -- the low half of the `no voxel`
# key a lane without a voxel carries.  (Sparse only: three bricks of it ever hold records.)
GEO_HUGE = dict(dims=(2048, 2048, 1024), origin=(-32.0, -32.0, -16.0), voxel=1.0 / 32)


def list_last_record():
    """runs of the LAST voxel of a 2^32-voxel grid with a point that has no voxel on the next lane, of every kind"""
    geo, ln = GEO_HUGE, Lanes(GEO_HUGE, 99)
    last = tuple(d - 1 for d in geo["dims"])
    nbricks = geo["dims"][0] * geo["dims"][1] * geo["dims"][2] // 512
    followed = 0
    for row, kind in enumerate(INVALID_KINDS):
        ln.pad_to(16)
        ln.filler(row)                                                   # the run starts at another lane in every row
        ln.run(last, 3)
        ln.invalid(kind, row)
        ln.run(last, 1 + row)
        ln.invalid(kind, row + 3)
        followed += 2
        assert 0 < len(ln) % 16 <= 14
        ln.filler(14 - len(ln) % 16)
        ln.run(last, 2)                                                  # ... and one ends with its row
    xyz, rgb = ln.arrays()
    loc, _, ok = point_voxels(xyz, geo["origin"], geo["voxel"], (0, 0, 0), geo["dims"])
    is_last = ok & (loc == np.array(last)).all(axis=1)
    edges = dict(last_record_is_all_ones=512 * nbricks - 1 == 0xffffffff and last == (2047, 2047, 1023),
                 followed_by_every_kind=int((is_last[:-1] & ~ok[1:] & (np.arange(len(ok) - 1) % 16 != 15)).sum()) == followed == 8,
                 ends_a_row=int((is_last & (np.arange(len(ok)) % 16 == 15)).sum()) == 4,
                 three_bricks=len({tuple(v) for v in (loc[ok] // 8).tolist()}) == 3)
    return _case("last_record", geo, (xyz, rgb), edges)


LIMIT_VOXELS = ((5, 20, 33), (6, 20, 33))        # neighbours in x: adjacent records of one sub-brick


def limit_points(which, n=N_LIMIT):
    """n points at q = (4095, 4095, 4095) of LIMIT_VOXELS[which], colour 255"""
    xyz = np.tile(voxel_point(GEO, LIMIT_VOXELS[which], (FRAC - 1,) * 3), (n, 1))
    return xyz, np.full((n, 3), 255, np.uint8)


LIST_BUILDERS = dict(faces=list_faces, runs=list_runs, packed_maxima=list_packed_maxima, invalid_tail1=lambda: list_invalid(1),
                     invalid_tail63=lambda: list_invalid(63), first_touch=list_first_touch, one_brick=list_one_brick,
                     every_brick=list_every_brick, random=list_random)
LIST_NAMES = tuple(LIST_BUILDERS)
DYADIC_GEO_LISTS = ("faces", "runs", "packed_maxima", "invalid_tail1", "invalid_tail63", "random")      # the lists on GEO: blocks use them


@functools.lru_cache(maxsize=None)
def crafted_list(name):
    return LIST_BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def list_model(name):
    """(records, n_core, n_dropped, touched) of a list on its own geometry at offset 0, computed once (read-only)"""
    c = crafted_list(name)
    out = model_accumulate(c["xyz"], c["rgb"], **c["geo"])
    out[0].setflags(write=False)
    return out


def brick_model(case, brick_ijk):
    """(records uint64 [512, 4] of one brick of a list's grid, points of the list in that brick): the brick as a grid of its own"""
    off = tuple(8 * b for b in brick_ijk)
    rec, n_in, _, _ = model_accumulate(case["xyz"], case["rgb"], (8, 8, 8), case["geo"]["origin"], case["geo"]["voxel"], offset=off)
    return rec, n_in


def block_geometry(geo, offset=BLOCK_OFFSET):
    """the same voxels as a BLOCK: a lattice whose origin lies `offset` voxels lower, and the grid at that offset in it"""
    origin = tuple(geo["origin"][a] - offset[a] * geo["voxel"] for a in range(3))
    lattice = tuple(geo["dims"][a] + offset[a] for a in range(3))
    return dict(dims=geo["dims"], origin=origin, voxel=geo["voxel"]), lattice


def core_of(geo):
    return (8, 8, 8), tuple(d - 8 for d in geo["dims"])


# ---- frames ---------------------------------------------------------------------------------------------------------------------
CAMS = {"64x48": dict(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5),             # extract_common.CAM
        "61x47": dict(width=61, height=47, fx=60.0, fy=60.0, cx=30.0, cy=23.0),
        "33x17": dict(width=33, height=17, fx=60.0, fy=60.0, cx=16.0, cy=8.0)}
MIN_DEPTH, MAX_DEPTH = 0.01, 50.0
Z_FINE, Z_COARSE = 0.075, 1.0                    # at 0.075 m a pixel is 1.25 mm: every sample of the plane in its own 1 mm voxel
# 1 mm voxels: the plane's 80 x 60 mm but for its two left-most pixel columns (dropped); 2 m voxels: the whole plane in voxel (0, 0, 0)
GRID_FINE = dict(dims=(96, 64, 8), origin=(-0.0372, -0.0302, 0.0715), voxel=0.001)
GRID_COARSE = dict(dims=(8, 8, 8), origin=(-1.0, -1.0, 0.0), voxel=2.0)
STRIDES = (1, 2, 3, 5)
BATCHES = (1, 15, 16, 17, 32, 33)
STRIDE_SEQUENCE = (1, 1, 2, 2, 1, 3, 3)


def crafted_frames(cam):
    """[(name, depth f32 [H, W], bgr u8 [H, W, 3] or None)]: fronto-parallel planes"""
    h, w = cam["height"], cam["width"]
    rng = np.random.default_rng(1000 + w)
    v, u = np.mgrid[0:h, 0:w]
    checker = np.where((u + v) % 2 == 0, 0.0, Z_FINE).astype(np.float32)
    return [("coarse_white", np.full((h, w), Z_COARSE, np.float32), np.full((h, w, 3), 255, np.uint8)),
            ("fine_no_colour", np.full((h, w), Z_FINE, np.float32), None),
            ("fine_checker", checker, rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8))]


def tile_distinct_voxels(xyz_row_major, valid_hw, grid, tile=(32, 16)):
    """{(tx, ty): (samples with a voxel, distinct voxels)} of the 32 x 16 tiles of a (sub-sampled) frame; xyz in row-major order of
    its valid samples, valid_hw: which samples those are"""
    hs, ws = valid_hw.shape
    keys = np.full(hs * ws, -1, np.int64)
    keys[valid_hw.ravel()] = point_keys(xyz_row_major, grid)
    keys = keys.reshape(hs, ws)
    out = {}
    for ty in range(0, hs, tile[1]):
        for tx in range(0, ws, tile[0]):
            k = keys[ty:ty + tile[1], tx:tx + tile[0]].ravel()
            k = k[k >= 0]
            out[(tx // tile[0], ty // tile[1])] = (len(k), len(np.unique(k)))
    return out


# ---- bounds lists -----------------------------------------------------------------------------------------------------------------
BOUNDS_SIZES = (1, 255, 256, 257, 256 * 1024 + 1)     # the last: one point past 1024 blocks of 256, so the grid-stride loop runs


def bounds_reference(xyz):
    """(min[3], max[3]) as float64: NaN coordinates are ignored (fminf / fmaxf return the other operand); an axis with nothing but
    NaN keeps the empty extent (+inf, -inf)"""
    x = np.asarray(xyz, np.float32)
    return (np.fmin.reduce(x, axis=0, initial=np.float32(np.inf)).astype(np.float64),
            np.fmax.reduce(x, axis=0, initial=np.float32(-np.inf)).astype(np.float64))


def bounds_lists():
    """[(name, xyz)]: every size with the extreme of every axis at index 0, n - 1 and in the middle; then zeros of both signs,
    denormals, infinities and NaN"""
    out = []
    for n in BOUNDS_SIZES:
        base = np.random.default_rng(n).uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
        for pos in sorted({0, n // 2, n - 1}):
            for sign in (-1.0, 1.0):
                x = base.copy()
                x[pos] = np.float32(sign) * np.array([2.0, 3.0, 5.0], np.float32)
                out.append((f"n{n}_at{pos}_{'max' if sign > 0 else 'min'}", x))
    tiny = np.float32(1e-45)                                              # the smallest denormal
    assert tiny > 0 and tiny == np.nextafter(np.float32(0), np.float32(1))
    z = np.zeros((300, 3), np.float32)
    z[7], z[299] = -0.0, (tiny, -tiny, 0.0)
    out.append(("zeros_and_denormals", z))
    d = np.full((257, 3), np.float32(1e-39))                              # all denormal: the extremes differ in the last bits only
    d[256] = (np.float32(1e-39) + tiny, np.float32(1e-39) - tiny, -np.float32(1e-39))
    out.append(("denormals", d))
    i = np.random.default_rng(5).uniform(-1, 1, size=(600, 3)).astype(np.float32)
    i[0, 0], i[599, 1], i[300, 2], i[301, 2] = np.inf, -np.inf, np.inf, -np.inf
    out.append(("infinities", i))
    one = np.random.default_rng(6).uniform(-1, 1, size=(600, 3)).astype(np.float32)
    one[0, 0], one[255, 1], one[599, 2] = np.nan, np.nan, np.nan
    out.append(("one_nan_per_axis", one))
    col = one.copy()
    col[:, 1] = np.nan                                                     # an axis of nothing but NaN
    out.append(("an_axis_of_nan", col))
    out.append(("all_nan", np.full((300, 3), np.nan, np.float32)))
    return out
