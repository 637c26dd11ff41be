"""CPU: what the GPU extraction tests (tests/test_gpu_extract.py) are held to.  The crafted grids of tests/extract_common.py
reach what they claim to reach (asserted from the reference alone), the numpy restatement of tests/extract_reference.py agrees with
the C oracle's orc_extract -- written apart from each other -- and the fp64 expression the library promises for a position is
the exact rational value rounded once, up to the bound below.

The `exact` bound: every coordinate within 1 float32 ulp, at most 1 coordinate in 1000 not bit-equal.  Derived, not measured: the
fp64 evaluation errs by a few 2^-53 relative, so its f32 rounding is the correctly rounded value or that value's neighbour, and
it is the neighbour only when the exact value lies within that error of a rounding boundary (about 2^-26 of all values).
Measured here, oracle against the exact form: grid A 0 of 344 k coordinates over the sweep, the fused scene 0 of 113 k, grid L
16 of 3.53 M (4.5e-6), none further than 1 ulp."""
import numpy as np
import pytest

import extract_common as ec
import extract_reference as er
from helpers import SMALL, small_scene_frames
from oracle import c_oracle


def _oracle(g, tsdf, centroid):
    orc = c_oracle.Oracle(ec.CAM["width"], ec.CAM["height"], ec.CAM["fx"], ec.CAM["fy"], ec.CAM["cx"], ec.CAM["cy"], dims=g["dims"],
                          origin=g["origin"], voxel_size=g["voxel"], sdf_trunc=4 * g["voxel"])
    orc.tsdf, orc.centroid = tsdf, centroid
    return orc


def _classes_of(vol):
    """class number of every voxel, from the volumes the reference reads"""
    table = ec.tsdf_classes()
    key = lambda w, s: w * (1 << 32) + s
    keys = np.array([key(w, s) for w, s in table], np.int64)
    order = np.argsort(keys)
    at = np.searchsorted(keys[order], key(vol["weight"], vol["sum"]))
    assert np.array_equal(keys[order][np.minimum(at, len(keys) - 1)], key(vol["weight"], vol["sum"])), "a voxel outside the table"
    return order[at], len(table)


def _edge(axis):
    return (tuple(slice(0, -1) if q == axis else slice(None) for q in range(3)),
            tuple(slice(1, None) if q == axis else slice(None) for q in range(3)))


# ---- the generators reach what they claim -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "L"])
def test_every_ordered_pair_of_tsdf_classes_lies_on_an_edge_of_each_axis(name):
    cls, k = _classes_of(ec.grid(name)["vol"])
    assert np.array_equal(np.unique(cls), np.arange(k))
    for a in range(3):
        lo, hi = _edge(a)
        assert len(np.unique(cls[lo] * k + cls[hi])) == k * k, (name, a)


@pytest.mark.parametrize("name", ["A", "B", "L"])
def test_crossings_reach_the_faces_the_ties_and_the_colour_outcomes(name):
    g = ec.grid(name)
    vol, dims = g["vol"], g["dims"]
    for mw in ec.MIN_WEIGHTS:
        _, _, d = ec.reference(g, 1, min_weight=mw, core=None, details=True)
        for a in range(3):
            on = d["axis"] == a
            at = d["voxel"][on, a] % 8
            assert (at == 3).any(), (name, a, "a crossing over a sub-brick face")
            assert (at == 7).any() or dims[a] == 8, (name, a, "a crossing over a brick face (L is one brick wide in x and y)")
            assert (d["tie"] & on).any(), (name, a, "equal magnitudes on a crossing")
            if "n" in vol:
                assert set(d["colour_from"][on].tolist()) == {0, 1, 2}, (name, a, "nearer, farther, grey")
                va, vb = tuple(d["voxel"].T), tuple(d["neighbour"].T)
                differ = (vol["n"][va] > 0) & (vol["n"][vb] > 0) & (er._mean_colour(vol, va) != er._mean_colour(vol, vb)).any(axis=1)
                assert (differ & on & d["tie"]).any(), (name, a, "a tie between two colours: the lower end's wins")
                assert (differ & on & ~d["tie"]).any(), (name, a)
        # the upper faces hold voxels that would cross if the neighbour existed: usable, of either sign
        with np.errstate(invalid="ignore", divide="ignore"):
            t = vol["sum"] / (vol["weight"] * 32767.0)
        usable = (vol["weight"] >= max(1, mw)) & (np.abs(t) < 0.98)
        for a in range(3):
            face = tuple(dims[a] - 1 if q == a else slice(None) for q in range(3))
            assert (usable[face] & (t[face] < 0)).any() and (usable[face] & (t[face] > 0)).any(), (name, a)
            # a sum of exactly 0 next to a negative neighbour, both usable: the product is -0, not < 0
            lo, hi = _edge(a)
            assert (usable[lo] & usable[hi] & (vol["sum"][lo] == 0) & (t[hi] < 0)).any(), (name, a)
            assert (usable[lo] & usable[hi] & (t[lo] < 0) & (vol["sum"][hi] == 0)).any(), (name, a)


@pytest.mark.parametrize("name", ["A", "B", "S"])
def test_every_gate_has_voxels_on_both_sides_and_on_its_threshold(name):
    vol = ec.grid(name)["vol"]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.abs(vol["sum"] / (vol["weight"] * 32767.0))
    occupied = vol["n"] >= 1
    for n in (0, 1, 2, 3, ec.N_LIMIT):                       # min_count 0..3 and the documented limit
        assert (vol["n"] == n).any(), n
    for w in (0, ec.MW - 1, ec.MW, 3, ec.W_LIMIT):           # min_weight
        assert (occupied & (vol["weight"] == w)).any(), w
    heavy = occupied & (vol["weight"] >= ec.MW)
    for gate in ec.GATES:                                    # |mean| <= max_abs_tsdf (nothing lies above 1.0: |sum| <= 32767 w)
        assert (heavy & (t == gate)).any() and (heavy & (t < gate)).any(), gate
    assert (heavy & (t > ec.HALF_GATE)).any()
    assert ((vol["weight"] >= ec.MW) & (t == 0.98)).any()    # the band: on it, and the nearest sums on either side
    for w in (ec.MW - 1, ec.MW, 3, ec.W_LIMIT):
        lo98 = 98 * 32767 * w // 100
        at = vol["weight"] == w
        assert (at & (np.abs(vol["sum"]) == lo98) & (t < 0.98)).any() and (at & (np.abs(vol["sum"]) == lo98 + 1) & (t > 0.98)).any(), w
    # sums at the ends of the 32-bit fields
    assert (vol["sum"] == 32767 * ec.W_LIMIT).any() and (vol["sum"] == -32767 * ec.W_LIMIT).any()
    full = vol["n"] == ec.N_LIMIT
    for f in ("px", "py", "pz"):
        assert (full & (vol[f] == ec.N_LIMIT * 4095)).any() and (occupied & (vol[f] == 0)).any(), f
    for f in ("cr", "cg", "cb"):
        assert (full & (vol[f] == ec.N_LIMIT * 255)).any() and (full & (vol[f] % ec.N_LIMIT == ec.N_LIMIT - 1)).any(), f


def test_sparse_grid_has_every_brick_state_next_to_every_other():
    g = ec.grid("S")
    st = g["states"]
    tsdf_any = g["tsdf"].reshape(-1, 512 * 2).any(axis=1)
    cen_any = g["centroid"].reshape(-1, 512 * 4).any(axis=1)
    bricks = st.transpose(2, 1, 0).ravel()                   # bricks are numbered x fastest
    assert np.array_equal(tsdf_any, (bricks == 0) | (bricks == 1)) and np.array_equal(cen_any, (bricks == 0) | (bricks == 2))
    for a in range(3):
        lo, hi = _edge(a)
        assert len(np.unique(st[lo] * 4 + st[hi])) == 16, a
    # crossings run from a brick with TSDF records into both kinds of such bricks, and their colour look-ups into all four kinds
    _, _, d = ec.reference(g, 1, details=True)
    vox = np.repeat(np.repeat(np.repeat(st, 8, 0), 8, 1), 8, 2)
    over = (d["voxel"] // 8 != d["neighbour"] // 8).any(axis=1)
    pairs = set(zip(vox[tuple(d["voxel"][over].T)].tolist(), vox[tuple(d["neighbour"][over].T)].tolist()))
    assert pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert set(d["colour_from"][over].tolist()) == {0, 1, 2}
    # centroid mode: a voxel with points whose TSDF brick does not exist (gated out once min_weight > 0)
    assert ((g["vol"]["n"] > 0) & (vox == 2)).any()


def test_grid_shapes_reach_the_chunk_edges():
    a, l = ec.grid("A"), ec.grid("L")
    assert len(a["tsdf"]) == 7 * 2048 + 1024 and len(l["tsdf"]) == 1024 * 2048 + 512 and l["tsdf"].nbytes == 16781312
    _, _, d = ec.reference(l, 1, details=True)
    chunk = d["record"] // 2048
    assert chunk.max() == 1024 and (chunk == 1023).any() and (chunk == 1024).any()       # both sides of the 1024th, and the last
    assert len(np.unique(chunk)) == 1025                                                  # every chunk emits
    _, _, d = ec.reference(a, 0, details=True)
    assert (d["record"] // 2048 == 7).any()


# ---- reference == oracle --------------------------------------------------------------------------------------------------------
def _against_oracle(g, orc, params, vol=None, **flags):
    mode, mc, mw, gate = params
    want = orc.extract(mode, mc, mw, gate, use_tsdf=flags.get("use_tsdf", True), use_centroid=flags.get("use_centroid", True))
    kw = dict(use_centroid=flags.get("use_centroid", True), tsdf_channel=flags.get("use_tsdf", True), vol=vol)
    ec.assert_bit_equal(ec.reference(g, mode, mc, mw, gate, **kw), want, f"contract {params} {flags}")
    return ec.assert_within_exact_bound(want, ec.reference(g, mode, mc, mw, gate, form="exact", **kw), f"exact {params} {flags}")


@pytest.mark.parametrize("params", ec.SWEEP, ids=ec.sweep_id)
def test_grid_A_equals_the_oracle(params):
    g = ec.grid("A")
    orc = _oracle(g, g["tsdf"], g["centroid"])
    want = orc.extract(*params)
    assert len(want[0]) > 1000
    ec.assert_bit_equal(ec.swept("A", params, "contract"), want, "contract")
    ec.assert_within_exact_bound(want, ec.swept("A", params, "exact"), "exact")


def test_grid_A_without_a_channel_equals_the_oracle():
    g = ec.grid("A")
    orc = _oracle(g, g["tsdf"], g["centroid"])
    for mw in ec.MIN_WEIGHTS:
        _against_oracle(g, orc, (1, 1, mw, 1.0), use_centroid=False)                      # grey crossings
        for mc in ec.MIN_COUNTS:
            _against_oracle(g, orc, (0, mc, mw, ec.HALF_GATE), use_tsdf=False)            # no channel, no gate
    grey = orc.extract(1, use_centroid=False)[1]
    assert (grey == 128).all() and len(grey) == len(orc.extract(1)[1]) and not (orc.extract(1)[1] == 128).all()
    assert len(orc.extract(0, 1, ec.MW, ec.HALF_GATE, use_tsdf=False)[0]) > len(orc.extract(0, 1, ec.MW, ec.HALF_GATE)[0])


@pytest.mark.parametrize("mw", ec.MIN_WEIGHTS)
def test_grid_L_equals_the_oracle(mw):
    """L has a TSDF channel only: TSDF mode, grey"""
    g = ec.grid("L")
    off, total = _against_oracle(g, _oracle(g, g["tsdf"], None), (1, 1, mw, 1.0), use_centroid=False)
    assert total > 1000000


def test_fused_scene_equals_the_oracle():
    poses, frames = small_scene_frames(n=3, deg=5.0)
    dims, voxel = (64, 64, 64), 0.03
    orc = c_oracle.Oracle(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], dims=dims,
                          origin=(-0.96, -1.16, -0.96), voxel_size=voxel, sdf_trunc=4 * voxel)
    for (depth, bgr), (R, t) in zip(frames, poses):
        orc.tsdf_integrate(depth, R, t)
        orc.centroid_accumulate(depth, bgr, R, t)
    g = dict(dims=dims, origin=(-0.96, -1.16, -0.96), voxel=voxel, voxel_offset=(0, 0, 0), core=None)
    vol = er.volumes_from_records(dims, orc.tsdf, orc.centroid)
    t2, c2 = er.records_from_volumes(vol)
    assert np.array_equal(t2, orc.tsdf) and np.array_equal(c2, orc.centroid)              # the two conversions undo each other
    assert len(orc.extract(0)[0]) > 1000 and len(orc.extract(1)[0]) > 500
    for params in ec.SWEEP:
        _against_oracle(g, orc, params, vol=vol)
    _against_oracle(g, orc, (1, 1, 0, 1.0), vol=vol, use_centroid=False)
    _against_oracle(g, orc, (0, 1, ec.MW, ec.HALF_GATE), vol=vol, use_tsdf=False)


# ---- what the oracle does not have: voxel_offset and core ----------------------------------------------------------------------
def _sorted_rows(xyz, rgb):
    m = np.concatenate([ec.bits(xyz).astype(np.int64), rgb.astype(np.int64)], axis=1)
    return m[np.lexsort(m.T[::-1])]


@pytest.mark.parametrize("params", [(0, 1, 0, 1.0), (0, 2, ec.MW, ec.HALF_GATE), (1, 1, 0, 1.0), (1, 1, ec.MW, 1.0)], ids=ec.sweep_id)
def test_eight_blocks_with_cores_and_offsets_give_the_whole_grid(params):
    """16-voxel cores with a halo of one brick on the + sides that have a neighbour: the blocks' points, sorted, are the whole
    grid's, bit for bit"""
    g = ec.grid("W")
    whole = ec.reference(g, *params)
    assert len(whole[0]) > 5000
    parts = []
    for b in np.ndindex(2, 2, 2):
        lo = [16 * q for q in b]
        hi = [min(32, l + 24) for l in lo]
        cut = tuple(slice(l, h) for l, h in zip(lo, hi))
        vol = {f: v[cut] for f, v in g["vol"].items()}
        part = er.extract(vol, [h - l for l, h in zip(lo, hi)], g["origin"], g["voxel"], voxel_offset=lo, core=((0, 0, 0), (16, 16, 16)),
                          mode=params[0], min_count=params[1], min_weight=params[2], max_abs_tsdf=params[3])
        assert len(part[0]) > 0
        parts.append(part)
    got = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert np.array_equal(_sorted_rows(*got), _sorted_rows(*whole))
    # the same blocks without their cores emit the halo's points a second time
    assert len(got[0]) == len(whole[0])


def test_core_decides_by_the_emitting_voxel_on_grid_B():
    g = ec.grid("B")
    (lo, hi) = g["core"]
    _, _, d = ec.reference(g, 1, details=True)
    inside = ((d["voxel"] >= lo) & (d["voxel"] < hi)).all(axis=1)
    assert inside.all()
    out = ~((d["neighbour"] >= lo) & (d["neighbour"] < hi)).all(axis=1)
    assert out.any()                                                                    # a crossing that leaves the core is emitted
    _, _, d0 = ec.reference(g, 1, core=None, details=True)
    v_in = ((d0["voxel"] >= lo) & (d0["voxel"] < hi)).all(axis=1)
    n_in = ((d0["neighbour"] >= lo) & (d0["neighbour"] < hi)).all(axis=1)
    assert (~v_in & n_in).any() and int(v_in.sum()) == len(d["record"])                # one that enters it is not
    # the offset makes the f32 rounding coarse: neighbouring voxel centres along z share a float32 value or differ by one ulp
    xyz, _ = ec.reference(g, 0)
    assert np.abs(xyz[:, 2]).min() > 4.0e4 and len(np.unique(xyz[:, 2])) < 200


def test_round_ratio_f32_rounds_once_to_even():
    f = np.float32
    assert er.round_ratio_f32(1, 3) == float(f(1.0) / f(3.0)) and er.round_ratio_f32(-1, 3) == -er.round_ratio_f32(1, 3)
    assert er.round_ratio_f32((1 << 24) + 1, 1) == float(1 << 24) and er.round_ratio_f32((1 << 24) + 3, 1) == float((1 << 24) + 4)
    assert er.round_ratio_f32((1 << 25) - 1, 1) == float(1 << 25) and er.round_ratio_f32(0, 7) == 0.0
    # where rounding the double first would go wrong: just above a tie
    assert er.round_ratio_f32(((1 << 24) + 1) * (1 << 40) + 1, 1 << 40) == float((1 << 24) + 2)
    assert er.round_ratio_f32(1, 1 << 149) == float(np.float32(1.401298464324817e-45)) and er.round_ratio_f32(1, 1 << 151) == 0.0
    rng = np.random.default_rng(5)
    x = rng.standard_normal(2000) * 10.0 ** rng.integers(-6, 6, 2000)
    for v in x.tolist():
        num, den = v.as_integer_ratio()
        assert er.round_ratio_f32(num, den) == float(np.float32(v))
