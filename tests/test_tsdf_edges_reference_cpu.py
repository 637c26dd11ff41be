"""The crafted TSDF frames (tsdf_edges_common) on the CPU: the edge counters are pinned, the exact-rational model
(tsdf_edges_reference) excludes nothing on the family and equals both oracles bit for bit, and the two oracles equal each other
where the model does not apply.  tests/test_gpu_tsdf_edges.py runs the same frames through the HIP kernels."""
import numpy as np
import pytest

import tsdf_edges_common as ec
import tsdf_edges_reference as er
from oracle import second_numpy as sn

# counters of every family frame (R = I, the nine translations), in the order of ec.COUNTER_NAMES, as they were when the family
# was written.  An edit to the inputs that moves a voxel off an edge changes a number here.
PINNED = {
    "t0": (256, 60, 0, 0, 0, 0, 129, 24, 150, 190, 40, 329, 90, 17, 1893, 357, 3686, 1394, 287, 0, 0, 0),
    "left": (256, 60, 16, 0, 0, 0, 47, 63, 54, 54, 0, 114, 48, 51, 377, 1728, 2438, 1212, 32, 0, 0, 0),
    "right": (240, 44, 0, 16, 0, 0, 1, 0, 35, 91, 56, 71, 0, 17, 1697, 397, 2491, 1270, 13, 0, 0, 0),
    "top": (128, 30, 0, 0, 16, 0, 24, 0, 84, 84, 0, 210, 24, 17, 424, 189, 1595, 523, 17, 0, 0, 0),
    "bottom": (112, 14, 0, 0, 0, 16, 55, 0, 63, 63, 0, 152, 0, 2, 822, 0, 1434, 96, 562, 0, 0, 0),
    "zhalf": (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 18, 1640, 0, 1307, 1228, 21, 256, 0, 0),
    "zone": (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 83, 0, 48, 47, 1, 256, 4096, 0),
    "eps_x": (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 81, 0, 56, 55, 1, 0, 4096, 256),
    "eps_xy": (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 74, 0, 56, 56, 0, 0, 4096, 256),
}
# the frame on which each edge must be hit
HIT_ON = dict(ties="t0", ties_on_tile_border="t0", u_eq_left="left", u_eq_right="right", v_eq_top="top", v_eq_bottom="bottom",
              sdf_eq_minus_trunc="t0", sdf_just_below_minus_trunc="t0", sdf_eq_trunc="t0", sdf_in_free_band="t0",
              sdf_inside_free_band="t0", half_way_tie="t0", hi_eq_minus_trunc="t0", over_single_invalid_pixel="t0", tile_free="t0",
              tile_skip="t0", tile_open="t0", open_ends_one="t0", open_ends_without_update="t0", zc_eq_0="zone", zc_lt_0="zone",
              zc_below_guard="eps_xy")
# voxels the rational model excludes: none on the family and the permutation poses.  The 4 x 3 camera (fx = 4) has exact pixel
# ties on slices whose depth is no power of two (1 / zc rounds there): excluded, by the model's own rule.
EXCLUDED = {"tiny": 240}

FAMILY = ec.family()
PERMS = ec.permutation_cases()
VARIANTS = ec.variants()


def _ids(cases):
    return [c.name for c in cases]


def _c_grid(case):
    orc = ec.c_oracle_for(case)
    orc.tsdf_integrate(case.depth, case.R, case.t, case.scale)
    return orc.tsdf


def _np_grid(case):
    grid = np.zeros((int(np.prod(case.dims)), 2), np.int32)
    sn.tsdf_integrate(ec.geometry(case), grid, case.depth, case.R, case.t, case.scale)
    return grid


def test_case_names_are_unique_and_the_family_is_what_is_pinned():
    names = _ids(ec.all_cases())
    assert len(set(names)) == len(names)
    assert _ids(FAMILY) == list(PINNED)
    assert set(HIT_ON) == set(ec.COUNTER_NAMES)
    assert len(PERMS) == 24 and len({tuple(c.R.ravel()) for c in PERMS}) == 24


@pytest.mark.parametrize("case", FAMILY, ids=_ids(FAMILY))
def test_edge_counters_are_what_they_were(case):
    got = ec.counters(case)
    assert tuple(got[k] for k in ec.COUNTER_NAMES) == PINNED[case.name], got


@pytest.mark.parametrize("name", ec.COUNTER_NAMES)
def test_every_edge_is_hit(name):
    frame = HIT_ON[name]
    assert PINNED[frame][ec.COUNTER_NAMES.index(name)] > 0, (name, frame)


def test_the_strict_interior_of_the_free_band_lies_under_the_unit_slice():
    """trunc < sdf < 1.001 trunc: the `band` theme, 1 + 0.125 * 1.0005, under voxels of the zc = 1 slice (1.125 * 1.0005 minus 1 is
    1.0045 trunc: beyond the band)."""
    case = FAMILY[0]
    m = ec.intermediates(case)
    d = m["d_img"][m["v"], m["u"]]
    hit = m["win"] & (d == np.float32(ec.BAND))
    assert hit.any() and (m["zc"][hit] == 1.0).any()
    sdf = d[hit & (m["zc"] == 1.0)] - np.float32(1.0)
    assert ((sdf > np.float32(ec.TRUNC)) & (sdf < np.float32(ec.TRUNC) * np.float32(1.001))).all()


def test_odd_pixels_and_themes_reach_the_partial_tiles_of_the_ragged_camera():
    d = ec.patchwork(42, 27)
    assert np.array_equal(d[:24, :40][np.isfinite(d[:24, :40])], ec.patchwork(40, 24)[np.isfinite(ec.patchwork(40, 24))])   # extended, not changed
    last_col, last_row = d[:, 40:], d[24:, :]
    assert len(np.unique(last_col[np.isfinite(last_col)])) >= 4 and len(np.unique(last_row[np.isfinite(last_row)])) >= 4
    odd_col = sum(ec.tile_odd(5, ty) is not None for ty in range(4))
    odd_row = sum(ec.tile_odd(tx, 3) is not None for tx in range(6))
    assert odd_col >= 2 and odd_row >= 2


@pytest.mark.parametrize("case", FAMILY + PERMS, ids=_ids(FAMILY + PERMS))
def test_rational_model_excludes_nothing_and_equals_both_oracles(case):
    grid, applies = er.integrate(case)
    assert int((~applies).sum()) == 0                   # first: the model hides nothing ...
    assert np.array_equal(grid, _c_grid(case))          # ... then it is compared
    assert np.array_equal(grid, _np_grid(case))


DYADIC_VARIANTS = [c for c in VARIANTS if c.dyadic]


@pytest.mark.parametrize("case", DYADIC_VARIANTS, ids=_ids(DYADIC_VARIANTS))
def test_rational_model_equals_both_oracles_on_the_dyadic_variants(case):
    grid, applies = er.integrate(case)
    assert int((~applies).sum()) == EXCLUDED.get(case.name, 0)
    c, n = _c_grid(case), _np_grid(case)
    assert np.array_equal(grid[applies], c[applies]) and np.array_equal(grid[applies], n[applies])
    assert np.array_equal(c, n)


@pytest.mark.parametrize("case", VARIANTS, ids=_ids(VARIANTS))
def test_the_two_oracles_agree_on_every_variant(case):
    """general rotations, scale = 3 and the 16-bit frames included: no rational model there"""
    c = _c_grid(case)
    assert np.array_equal(c, _np_grid(case))
    if case.name in ("no_valid",):
        assert not c.any()
    elif case.name == "all_free":
        w = c[:, 1] > 0
        assert w.sum() > 5000 and (c[w, 0] == 32767).all()
    else:
        assert c[:, 1].sum() > 0


def test_degenerate_frames_are_what_they_claim():
    with np.errstate(invalid="ignore"):
        nv = ec.no_valid_pixel().depth
        assert not ((nv > ec.MIN_DEPTH) & (nv < ec.MAX_DEPTH)).any()
        lp = ec.last_pixel_only().depth
        ok = (lp > ec.MIN_DEPTH) & (lp < ec.MAX_DEPTH)
    assert ok.sum() == 1 and ok[-1, -1]
    assert _c_grid(ec.last_pixel_only())[:, 1].sum() > 0                  # and voxels look through it
    g = _c_grid(ec.saturating_behind())
    assert ((g[:, 1] == 1) & (g[:, 0] == -32767)).sum() >= 256            # the whole zc = 1 slice: sdf == -trunc


def test_u16_frames_hold_the_special_values():
    case = [c for c in VARIANTS if c.name == "u16_t0"][0]
    assert {0, 65535, 500, 501} <= set(case.mm.ravel().tolist())
    assert np.array_equal(case.depth, case.mm.astype(np.float32) / np.float32(1000.0))


def test_the_frames_that_must_catch_a_wrong_comparison_hold_their_edges():
    """`sdf > -trunc` for `>=` loses the voxels at sdf == -trunc of frame t0; `uf > -0.5` for `>=` loses the column at uf == -0.5 of
    frame left, some of which the oracle updates"""
    t0, left = FAMILY[0], FAMILY[1]
    m = ec.intermediates(t0)
    with np.errstate(invalid="ignore"):
        d = m["d_img"][m["v"], m["u"]]
        ok = m["win"] & m["valid_img"][m["v"], m["u"]]
        assert (ok & (d - m["zc"] == -np.float32(ec.TRUNC))).sum() == PINNED["t0"][6] > 0      # `>` for `>=` drops these
    ml = ec.intermediates(left)
    assert ((ml["uf"] == np.float32(-0.5)) & ml["win"]).sum() == 16                        # `uf > -0.5` drops these
    g = _c_grid(left)
    rec = sn.record_index(ml["I"], ml["J"], ml["K"], 2, 2)
    assert (g[rec[(ml["uf"] == np.float32(-0.5)) & ml["win"]], 1] == 1).any()              # and some of them are updated

