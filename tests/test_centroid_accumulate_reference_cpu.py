"""CPU: keeps the model and the crafted inputs of tests/centroid_accumulate_common.py honest (tests/test_gpu_centroid_accumulate.py
compares the kernels with them).  The model against the C oracle, against ref_numpy's Open3D restatement to the rule's own
quantum, and against an exact-fraction evaluation of the rule; and the conditions the crafted inputs must meet."""
from fractions import Fraction

import numpy as np
import pytest

import centroid_accumulate_common as cc
import extract_reference as er
from oracle import c_oracle, ref_numpy


def _oracle(grid, cam=cc.CAMS["64x48"]):
    return c_oracle.Oracle(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], min_depth=cc.MIN_DEPTH,
                           max_depth=cc.MAX_DEPTH, dims=grid["dims"], origin=grid["origin"], voxel_size=grid["voxel"],
                           sdf_trunc=4 * grid["voxel"])


# ---- the record order -------------------------------------------------------------------------------------------------------------
def test_record_order_is_the_documented_one():
    dims = cc.GEO["dims"]
    ridx = er.record_index(dims)
    back = cc.to_record_order(ridx)                                    # every voxel's record index, put into record order
    assert np.array_equal(back, np.arange(ridx.size))
    orc = _oracle(cc.GEO)
    for ijk in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (4, 0, 0), (0, 4, 0), (0, 0, 4), (8, 0, 0), (0, 8, 0), (0, 0, 8), (31, 23, 39), (13, 9, 21)]:
        assert orc.vox_index(*ijk) == ridx[ijk]


# ---- the crafted lists hold their edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.LIST_NAMES)
def test_every_list_holds_every_declared_edge(name):
    c = cc.crafted_list(name)                                          # (the builder asserts it too: a missing edge fails, nothing skips)
    assert c["edges"] and all(c["edges"].values()), [k for k, v in c["edges"].items() if not v]
    assert c["xyz"].dtype == np.float32 and c["rgb"].dtype == np.uint8 and len(c["xyz"]) == len(c["rgb"])


def test_every_run_length_and_alignment_is_present():
    c = cc.crafted_list("runs")
    assert len(cc.LS_PAIRS) == 136
    runs = {(i % 16, l) for i, l, k in cc.row_runs(cc.point_keys(c["xyz"], c["geo"])) if k >= 0}
    assert {(s, L) for L, s in cc.LS_PAIRS} <= runs
    for L, s in cc.LS_PAIRS:
        assert c["edges"][f"L{L}_s{s}"]
    for name in ("row_end", "wave_end", "workgroup_end", "alternation", "wave_of_one_voxel"):
        assert c["edges"][name]


def test_every_field_reaches_its_sixteen_lane_maximum():
    c = cc.crafted_list("packed_maxima")
    keys = cc.point_keys(c["xyz"], c["geo"])
    _, q, ok = cc.point_voxels(c["xyz"], c["geo"]["origin"], c["geo"]["voxel"], (0, 0, 0), c["geo"]["dims"])
    assert ok.all()
    per_point = dict(n=np.ones(len(q), np.int64), px=q[:, 0], py=q[:, 1], pz=q[:, 2], cr=c["rgb"][:, 0].astype(np.int64),
                     cg=c["rgb"][:, 1].astype(np.int64), cb=c["rgb"][:, 2].astype(np.int64))
    sums = [{f: int(per_point[f][i:i + l].sum()) for f in cc.FIELDS} for i, l, _ in cc.row_runs(keys) if l == 16]
    for f in cc.FIELDS:
        top = 16 * cc.FIELD_MAX[f]
        assert any(s[f] == top for s in sums), f
        if f != "n":                                                   # ... and alone: the other six (the count apart) at 0
            assert any(s[f] == top and all(s[g] == 0 for g in cc.FIELDS if g not in (f, "n")) for s in sums), f
    assert any(all(s[f] == 16 * cc.FIELD_MAX[f] for f in cc.FIELDS) for s in sums)
    # the packed scan's field widths: n < 2^7, colour sums < 2^14 (r above n: 7 + 12 bits), offset sums < 2^32
    assert 16 < 1 << 7 and 16 * 255 < 1 << 12 and 16 * 4095 < 1 << 16


@pytest.mark.parametrize("tail", (1, 63))
def test_every_invalid_kind_occurs_before_after_and_inside_a_run(tail):
    c = cc.crafted_list(f"invalid_tail{tail}")
    for k in cc.INVALID_KINDS:
        for where in ("before", "after", "inside"):
            assert c["edges"][f"{k}_{where}"]
        assert c["edges"][f"{k}_splits_a_run"]
    assert c["edges"]["whole_wave_invalid"] and len(c["xyz"]) % 64 == tail
    x = c["xyz"]
    assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
    assert cc.list_model(c["name"])[2] == int((cc.point_keys(x, c["geo"]) < 0).sum()) > 64


# ---- the model against the C oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.LIST_NAMES)
def test_model_equals_the_oracle_on_the_lists(name):
    c = cc.crafted_list(name)
    rec, n_core, n_dropped, touched = cc.list_model(name)
    orc = _oracle(c["geo"])
    orc.centroid_points(c["xyz"], c["rgb"])
    assert np.array_equal(rec, orc.centroid)
    assert (n_core, n_dropped) == (orc.n_acc.value, orc.n_drop.value) and n_core + n_dropped == len(c["xyz"])
    assert touched == int(orc.centroid.reshape(-1, 512 * 4).any(axis=1).sum()) > 0
    # the same cloud reversed: the same records
    assert np.array_equal(cc.model_accumulate(c["xyz"][::-1].copy(), c["rgb"][::-1].copy(), **c["geo"])[0], rec)


def test_last_record_list_holds_its_edges_and_its_brick_equals_the_oracle():
    c = cc.list_last_record()
    assert all(c["edges"].values()), c["edges"]
    geo, last_brick = c["geo"], tuple(d // 8 - 1 for d in c["geo"]["dims"])
    rec, n_in = cc.brick_model(c, last_brick)
    shifted = dict(dims=(8, 8, 8), voxel=geo["voxel"], origin=tuple(o + 8 * b * geo["voxel"] for o, b in zip(geo["origin"], last_brick)))
    orc = _oracle(shifted)                                             # (dyadic: the brick's own corner as the origin names the same voxels)
    orc.centroid_points(c["xyz"], c["rgb"])
    assert np.array_equal(rec, orc.centroid) and n_in == orc.n_acc.value == int(rec[511, 1] >> cc.S32) == 4 * 3 + (1 + 2 + 3 + 4) + 4 * 2
    assert int(rec.any(axis=1).sum()) == 1


def test_model_equals_the_oracle_at_the_limit():
    assert cc.N_LIMIT * (cc.FRAC - 1) < 1 << 32
    xyz, rgb = cc.limit_points(0)
    rec, n_core, n_dropped, touched = cc.model_accumulate(xyz, rgb, **cc.GEO)
    orc = _oracle(cc.GEO)
    orc.centroid_points(xyz, rgb)
    assert np.array_equal(rec, orc.centroid) and (n_core, n_dropped, touched) == (cc.N_LIMIT, 0, 1)
    hit = rec[er.record_index(cc.GEO["dims"])[cc.LIMIT_VOXELS[0]]]
    top, n = cc.N_LIMIT * (cc.FRAC - 1), cc.N_LIMIT
    assert [int(w) for w in hit] == [top | top << 32, top | n << 32, 255 * n | (255 * n) << 32, 255 * n]
    assert int(rec.any(axis=1).sum()) == 1                               # nothing carried into a neighbour
    v, one = cc.model_volumes(xyz, rgb, **cc.GEO)[0], cc.model_volumes(xyz[:1], rgb[:1], **cc.GEO)[0]
    cc.records_from_volumes(cc.add_volumes(v, one, times=(1, 256)))      # 2^32 - 2^20 x 4095 = 2^20 = 256 x 4095 + 256: room for 256 more
    with pytest.raises(AssertionError):                                  # ... and with the 257th a half would carry: the model refuses
        cc.records_from_volumes(cc.add_volumes(v, one, times=(1, 257)))


@pytest.mark.parametrize("cam", list(cc.CAMS))
def test_model_on_the_oracle_points_equals_the_oracle_on_the_frames(cam):
    for grid in (cc.GRID_FINE, cc.GRID_COARSE):
        for stride in cc.STRIDES:
            for name, depth, bgr in cc.crafted_frames(cc.CAMS[cam]):
                orc = _oracle(grid, cc.CAMS[cam])
                xyz, rgb = orc.backproject(depth, bgr, subsample=stride, min_depth=cc.MIN_DEPTH, max_depth=cc.MAX_DEPTH)
                rec, n_core, n_dropped, _ = cc.model_accumulate(xyz, rgb, **grid)
                orc.centroid_accumulate(depth, bgr, subsample=stride, min_depth=cc.MIN_DEPTH, max_depth=cc.MAX_DEPTH)
                assert np.array_equal(rec, orc.centroid), (name, stride)
                assert (n_core, n_dropped) == (orc.n_acc.value, orc.n_drop.value), (name, stride)
                hs, ws = -(-depth.shape[0] // stride), -(-depth.shape[1] // stride)
                if name == "fine_checker":
                    assert len(xyz) in (hs * ws // 2, (hs * ws + 1) // 2) if stride % 2 else len(xyz) in (0, hs * ws)
                else:
                    assert len(xyz) == hs * ws
                if bgr is None:
                    assert not rgb.any()


def test_plane_frames_fill_and_collapse_the_table():
    cam = cc.CAMS["64x48"]
    frames = {name: (d, c) for name, d, c in cc.crafted_frames(cam)}
    orc = _oracle(cc.GRID_FINE)
    d, c = frames["fine_no_colour"]
    xyz, _ = orc.backproject(d, c, min_depth=cc.MIN_DEPTH, max_depth=cc.MAX_DEPTH)
    tiles = cc.tile_distinct_voxels(xyz, np.ones(d.shape, bool), cc.GRID_FINE)
    assert len(tiles) == 6 and sum(t == (512, 512) for t in tiles.values()) == 3       # the right-hand tiles: all 512 slots, all distinct
    assert all(n == k for n, k in tiles.values()) and tiles[(0, 0)] == (480, 480)       # two columns of the left-hand tiles are dropped
    d, c = frames["fine_checker"]
    xyz, _ = orc.backproject(d, c, min_depth=cc.MIN_DEPTH, max_depth=cc.MAX_DEPTH)
    tiles = cc.tile_distinct_voxels(xyz, d > 0, cc.GRID_FINE)
    assert tiles[(1, 1)] == (256, 256)
    d, c = frames["coarse_white"]
    xyz, rgb = _oracle(cc.GRID_COARSE).backproject(d, c, min_depth=cc.MIN_DEPTH, max_depth=cc.MAX_DEPTH)
    tiles = cc.tile_distinct_voxels(xyz, np.ones(d.shape, bool), cc.GRID_COARSE)
    assert set(tiles.values()) == {(512, 1)} and (rgb == 255).all()                     # every sample of every tile in one voxel
    rec = cc.model_accumulate(xyz, rgb, **cc.GRID_COARSE)[0]
    assert int(rec.any(axis=1).sum()) == 1 and int(rec[0, 1] >> cc.S32) == 64 * 48


# ---- the model against Open3D's rule and against exact arithmetic ----------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.DYADIC_GEO_LISTS)
def test_model_means_equal_open3d_to_the_quantum(name):
    c = cc.crafted_list(name)
    keep = cc.point_keys(c["xyz"], c["geo"]) >= 0
    xyz, rgb, voxel = c["xyz"][keep], c["rgb"][keep], c["geo"]["voxel"]
    pm, cm, idx, cnt, origin = ref_numpy.voxel_centroid_open3d(xyz, rgb, voxel)
    dims = tuple(int(-(-(d + 1) // 8) * 8) for d in idx.max(axis=0))
    vol, n_core, n_dropped = cc.model_volumes(xyz, rgb, dims, origin, voxel)
    assert n_dropped == 0 and n_core == len(xyz)
    at = np.argwhere(vol["n"] > 0)
    assert np.array_equal(at, idx) and np.array_equal(vol["n"][tuple(at.T)], cnt)
    n = cnt.astype(np.float64)
    for a, f in enumerate(("px", "py", "pz")):
        mean = origin[a] + (at[:, a] + vol[f][tuple(at.T)] / (n * cc.FRAC)) * voxel
        # q = floor(frac * 4096): every point lies in [q, q + 1) / 4096 of its voxel, and so does the mean against the mean of q
        err = pm[:, a] - mean
        assert err.min() >= -1e-12 and err.max() < voxel / cc.FRAC + 1e-12, (f, err.min(), err.max())
    for a, f in enumerate(("cr", "cg", "cb")):
        assert np.abs(cm[:, a] - vol[f][tuple(at.T)] / (255.0 * n)).max() < 1e-12


def _exact_voxel(p, origin, voxel, dims):
    """(voxel, q) of one f32 point by the rule in exact rational arithmetic, None without a voxel"""
    out = []
    for a in range(3):
        if not np.isfinite(p[a]):
            return None
        rc = (Fraction(float(p[a])) - Fraction(origin[a])) / Fraction(voxel)
        v = rc.numerator // rc.denominator
        if not 0 <= v < dims[a]:
            return None
        out.append((v, min(int((rc - v) * cc.FRAC), cc.FRAC - 1)))
    return out


@pytest.mark.parametrize("name", cc.DYADIC_GEO_LISTS)
def test_model_voxels_equal_exact_fractions(name):
    c = cc.crafted_list(name)
    geo = c["geo"]
    loc, q, ok = cc.point_voxels(c["xyz"], geo["origin"], geo["voxel"], (0, 0, 0), geo["dims"])
    for i, p in enumerate(c["xyz"]):
        e = _exact_voxel(p, geo["origin"], geo["voxel"], geo["dims"])
        assert (e is not None) == bool(ok[i]), (i, p)
        if e is not None:
            assert [v for v, _ in e] == loc[i].tolist() and [x for _, x in e] == q[i].tolist(), (i, p)


# ---- blocks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.DYADIC_GEO_LISTS)
def test_block_model_is_a_slice_of_the_lattice_model(name):
    c = cc.crafted_list(name)
    block, lattice = cc.block_geometry(c["geo"])
    off, dims = cc.BLOCK_OFFSET, c["geo"]["dims"]
    whole, _, _ = cc.model_volumes(c["xyz"], c["rgb"], lattice, block["origin"], block["voxel"])
    cut = {f: whole[f][off[0]:off[0] + dims[0], off[1]:off[1] + dims[1], off[2]:off[2] + dims[2]] for f in cc.FIELDS}
    rec, n_core, n_dropped, touched = cc.model_accumulate(c["xyz"], c["rgb"], offset=off, **block)
    assert np.array_equal(rec, cc.records_from_volumes(cut))
    if name != "faces":                                                # dyadic: the shifted origin names the same voxels ...
        assert np.array_equal(rec, cc.list_model(name)[0])
        assert (n_core, n_dropped, touched) == cc.list_model(name)[1:]
    else:           # ... but for the f32 just below 0: -2^-149 - (-0.5) rounds to 0.5 in fp64, so the block keeps what the grid at 0 drops
        assert n_dropped == cc.list_model(name)[2] - 1 and not np.array_equal(rec, cc.list_model(name)[0])
    core = cc.core_of(c["geo"])
    rec_c, n_core_c, n_dropped_c, _ = cc.model_accumulate(c["xyz"], c["rgb"], offset=off, core=core, **block)
    inner = tuple(slice(lo, hi) for lo, hi in zip(*core))
    assert np.array_equal(rec_c, rec) and n_dropped_c == n_dropped and n_core_c == int(cut["n"][inner].sum()) < n_core


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def test_bounds_lists_and_their_rule():
    lists = dict(cc.bounds_lists())
    assert {len(x) for x in lists.values()} >= set(cc.BOUNDS_SIZES)
    for name, x in lists.items():
        lo, hi = cc.bounds_reference(x)
        for a in range(3):
            col = x[:, a][~np.isnan(x[:, a])].astype(np.float64)
            col = col.tolist() if len(col) < 1000 else [col.min(), col.max()]     # (Python's own min / max on the short lists)
            assert lo[a] == (min(col) if col else np.inf) and hi[a] == (max(col) if col else -np.inf), (name, a)
        if name.startswith("n"):                                       # the planted extreme decides every axis
            pos, sign = int(name.split("_at")[1].split("_")[0]), (1.0 if name.endswith("max") else -1.0)
            want = sign * np.array([2.0, 3.0, 5.0])
            assert np.array_equal(hi if sign > 0 else lo, want) and np.array_equal(x[pos].astype(np.float64), want)
    lo, hi = cc.bounds_reference(lists["zeros_and_denormals"])
    assert lo[0] == 0 and hi[0] > 0 and lo[1] < 0 and hi[0] == 2.0 ** -149 and lo[1] == -2.0 ** -149
    lo, hi = cc.bounds_reference(lists["all_nan"])
    assert (lo == np.inf).all() and (hi == -np.inf).all()
