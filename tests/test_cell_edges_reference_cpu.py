"""The crafted cell-reader cases (cell_edges_common) on the CPU: the f32 restatements the GPU tests compare the kernels with
(raycast_reference, track_reference) are held to account by the fp64 model (cell_edges_reference), which is written from the rules
in a formulation of its own.

  * every case reaches the edges it names, every family all of its edges, in both directions where an edge has two (counters);
  * on the exact cases the model, rounded to f32, equals the restatement bit for bit: depth, normals, colour and sample counts of
    every ray; n_src, n_corr and every summand of every sample, and the tracker's sums are exact (added forwards, backwards and by
    math.fsum they are one number);
  * on the generic cases (tilted poses) rays and samples whose fp64 march comes within DELTA of a decision are set aside -- at most
    2 % of a case and none of its named rays, by the model's margins alone -- and the rest agree in every decision, in depth within
    DEPTH_ULPS and in the normal within the angle that implies.

MEASURED (printed by test_generic_deviation_is_what_the_bounds_were_taken_from, which fails if a figure outgrows its bound):
  largest |x_f32 - x_f64| over the generic cases: 1.29e-5 voxel at a hit (generic_tilt_2), 9.3e-6 voxel at a tracker sample (track_tilted);
      DELTA = 2^-14 voxel = 6.1e-5, the next power of two above 4 x that (a field value F counts as |F - limit| / 4 voxels: |grad F| < 4);
  largest |z*_f32 - z*_f64| on kept rays: 6.74 ulp(f32) of z* (generic_tilt_2); DEPTH_ULPS = 27 = 4 x that, rounded up.
Four, because a deviation is a sum of a handful of f32 roundings and another pose may align them.
"""
import math

import numpy as np
import pytest

import cell_edges_common as cc
import cell_edges_reference as cer
import raycast_reference as rr
import track_reference as tr

F32 = np.float32
DELTA = 2.0 ** -14
DEPTH_ULPS = 27.0
CASES = cc.cases()
RAY = [c for c in CASES if c.kind == "ray"]
TRACK = [c for c in CASES if c.kind == "track"]
ids = lambda cs: [c.name for c in cs]

# the edges each family is there for; the family's total must be non-zero for every one
MUST_HIT = dict(
    range=("end_hit", "ended_by_z_far", "ended_by_box_exit", "first_sample_negative", "z_near_gt_z_far", "end_range_empty", "half_voxel_steps"),
    box=("axis_parallel_inside", "axis_parallel_outside", "axis_parallel_negative_zero", "first_sample_on_face", "sample_on_open_end",
         "negative_after_undefined", "F_eq_0_prev_undefined", "end_hit", "end_range_empty", "ended_by_box_exit"),
    steps=("end_cap", "end_hit", "half_voxel_steps", "ended_by_box_exit"),
    zeros=("F_eq_0_prev_defined", "F_eq_0_prev_undefined", "first_sample_negative", "negative_after_undefined", "hit_normal_zero_gradient",
           "hit_normal_cell_undefined", "end_hit", "end_behind"),
    weights=("w_eq_mw", "w_eq_mw_minus_1", "w0_sum_nonzero", "sum_not_f32", "end_hit", "ended_by_box_exit", "negative_after_undefined"),
    colour=("colour_count_0", "colour_mean", "colour_division_rounds", "colour_last_voxel"),
    shapes=("end_hit", "end_range_empty", "ended_by_box_exit"),
    generic=("end_hit", "ended_by_box_exit"),
    track=("F_eq_gate", "gated", "gate_capped", "cell_undefined", "w_eq_mw_minus_1", "d_zero", "d_nan", "d_inf", "d_negative", "d_eq_min", "d_eq_max",
           "d_next_above_min", "d_next_below_min", "d_next_above_max", "d_next_below_max", "scale_crosses_min", "scale_crosses_max"),
)

_restated = {}


def restated(case):
    """the f32 restatement's answer, computed once per case"""
    if case.name not in _restated:
        if case.kind == "ray":
            zn, zf = case.z_range
            with np.errstate(all="ignore"):
                _restated[case.name] = rr.raycast(case.rec, case.dims, case.origin, cc.VOXEL, cc.TRUNC, case.cam, case.pose, min_weight=case.min_weight,
                                                  z_near=zn, z_far=zf, centroid=case.cen)
        else:
            _restated[case.name] = tr.sums(case.rec, case.dims, case.origin, cc.VOXEL, cc.TRUNC, case.cam, cc.frame_f32(case), case.pose, stride=case.stride,
                                           max_dist=case.max_dist, min_weight=case.min_weight, min_depth=case.min_depth, max_depth=case.max_depth,
                                           scale=case.scale, detail=True)
    return _restated[case.name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the edges are reached --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in CASES if c.model], ids=ids([c for c in CASES if c.model]))
def test_a_case_reaches_the_edges_it_names(case):
    k = cc.counters(case)
    print(case.name, k)
    missing = [e for e in case.edges if not k.get(e)]
    assert not missing, (case.name, missing)
    if case.kind == "ray":
        ends = sum(v for e, v in k.items() if e.startswith("end_"))
        assert ends == k["n_rays"] == case.cam["width"] * case.cam["height"]        # every ray leaves by exactly one named exit


@pytest.mark.parametrize("fam", cc.FAMILIES)
def test_a_family_reaches_all_of_its_edges(fam):
    total = {}
    for case in cc.family(fam):
        if case.model:
            for k, v in cc.counters(case).items():
                total[k] = total.get(k, 0) + v
    print(fam, total)
    missing = [e for e in MUST_HIT[fam] if not total.get(e)]
    assert not missing, (fam, missing)


def test_the_named_rays_sit_on_their_edges():
    """what the counters cannot say: WHICH ray, after how many samples, at which depth"""
    hit, miss, skim = (cc.by_name(n) for n in ("steps_cap_reached_by_the_hit", "steps_cap_before_the_hit", "steps_skim"))
    for case, depth in ((hit, 1.0 + 4095.0 / 32.0), (miss, 0.0), (skim, 0.0)):
        d, _, _, s = restated(case)
        print(case.name, "centre ray: depth", d[2, 4], "samples", s[2, 4])
        assert s[2, 4] == rr.MAX_STEPS == cer.MAX_STEPS == 4096 and d[2, 4] == F32(depth)
        assert (s < 4096).sum() == s.size - 1                                        # the budget is spent by that ray alone
    # the long march that takes inexact steps (device against restatement only): a hit half-way between layers 3000 and 3001, 1 m + 3000.5
    # voxels from the camera, within the 0.01 voxel the secant leaves; 1200 layers further on the budget ends the ray
    d, n, _, s = restated(cc.by_name("steps_plane_at_3000"))
    assert s[2, 4] == 2998 and abs(float(d[2, 4]) - (1.0 + 3000.5 / 32.0)) < 0.01 / 32.0 and (n[2, 4] == np.array([0, 0, -1], F32)).all()
    d, _, _, s = restated(cc.by_name("steps_plane_at_4200"))
    assert s[2, 4] == 4096 and not d.any()
    # the zero of scene_a: layer 11, 1 + 11/32 from the camera, on every ray
    d, n, _, s = restated(cc.by_name("range_default"))
    assert (d == F32(1.0 + 11.0 / 32.0)).all() and (n == np.array([0, 0, -1], F32)).all() and (s == 12).all()
    # one float of z_far decides
    assert not restated(cc.by_name("range_far_one_float_before"))[0].any() and restated(cc.by_name("range_far_at_sample"))[0].all()
    # a hit AT the sample, with no normal; and a hit whose cell is not usable: depth without a normal on exactly the rays counted
    d, n, _, _ = restated(cc.by_name("zeros_slab"))
    assert (d == F32(cc.ZN78 + 10.0 / 32.0 + 1.0 / 64.0)).all() and not n.any()
    case = cc.by_name("zeros_unobserved_column")
    d, n, _, _ = restated(case)
    flat = (d > 0) & ~n.any(axis=-1)
    assert flat.sum() == cc.counters(case)["hit_normal_cell_undefined"] == 5 and flat[2, 7] and flat[:, 7].all()
    # between the last two layers of each axis
    for name in ("box_last_layers_x", "box_last_layers_y", "box_last_layers_z", "colour_last_half_voxel"):
        assert (restated(cc.by_name(name))[0] == F32(1.0 + 14.5 / 32.0)).all(), name
    d, _, bgr, _ = restated(cc.by_name("colour_last_half_voxel"))
    assert (bgr == 128).all(axis=-1).sum() == 15 and len(np.unique(bgr.reshape(-1, 3), axis=0)) > 10


def test_the_member_counts_sit_on_their_edges():
    assert cc.track_members(64, 32) == (32, 1) and cc.track_members(88, 24) == (33, 2) and cc.track_members(65, 33) == (45, 2)
    assert cc.track_members(1024, 520) == (8320, 256) and cc.track_members(512, 260) == (2112, 66)       # the cap, and below it
    assert cc.track_members(9, 5) == (2, 1) and 2 < 4                                                       # fewer tiles than one member has waves
    have = {(c.cam["width"], c.cam["height"], c.stride) for c in TRACK}
    assert {(64, 32, 1), (88, 24, 1), (65, 33, 1), (1024, 520, 1), (9, 5, 1)} <= have
    for c in TRACK:                                                                                          # partial tiles at every stride
        ws, hs = -(-c.cam["width"] // c.stride), -(-c.cam["height"] // c.stride)
        if c.cam["width"] in (9, 65):
            assert ws % 8 or hs % 8, c.name


# ---- the exact cases ----------------------------------------------------------------------------------------------------------------------
EXACT_RAY = [c for c in RAY if c.exact]


@pytest.mark.parametrize("case", EXACT_RAY, ids=ids(EXACT_RAY))
def test_exact_ray_cases_equal_the_model_bit_for_bit(case):
    d, n, bgr, s = restated(case)
    md, mn, mbgr, ms, _, _ = cc.model(case.name)
    assert same_bits(d, md.astype(F32)), (case.name, "depth", np.argwhere(d != md.astype(F32))[:4])
    # (values, not bits, for the normals: whether a zero component is +0 or -0 is left by the order of a rotation's additions, which the
    # model does not share; the GPU test compares the kernel's bytes with the restatement's)
    assert np.array_equal(n, mn.astype(F32)), (case.name, "normals")
    assert np.array_equal(bgr, mbgr), (case.name, "colour")
    assert np.array_equal(s, ms), (case.name, "samples")


def _three_ways(x, y):
    p = x * y                                                                          # f32 x f32: exact in fp64
    fwd, bwd = float(np.cumsum(p)[-1]) if len(p) else 0.0, float(np.cumsum(p[::-1])[-1]) if len(p) else 0.0
    return fwd, bwd, math.fsum(p.tolist())


EXACT_TRACK = [c for c in TRACK if c.exact]


@pytest.mark.parametrize("case", EXACT_TRACK, ids=ids(EXACT_TRACK))
def test_exact_tracker_cases_equal_the_model_and_their_sums_are_exact(case):
    w = restated(case)
    J, r = w["J"].astype(np.float64), w["r"].astype(np.float64)
    if case.model:
        m = cc.model(case.name)
        assert (w["n_src"], w["n_corr"]) == (m["n_src"], m["n_corr"]), case.name
        assert m["uv"] == list(zip(w["u"].tolist(), w["v"].tolist()))                 # the same samples, none left out
        assert same_bits(w["J"], m["J"].astype(F32)) and same_bits(w["r"], m["r"].astype(F32)), case.name
    assert w["n_corr"] > (3 if case.cam["width"] == 9 else 50) and w["n_src"] >= w["n_corr"]
    cols = [(J[:, i], J[:, j]) for i in range(6) for j in range(i, 6)] + [(J[:, i], r) for i in range(6)] + [(r, r)]
    want = np.concatenate([w["A"], w["b"], [w["e"]]])
    for q, (x, y) in enumerate(cols):
        fwd, bwd, exact = _three_ways(x, y)
        assert fwd == bwd == exact == want[q], (case.name, q, fwd, bwd, exact, want[q])
    assert np.abs(want).max() > 0 and w["e"] > 0


# ---- the generic cases --------------------------------------------------------------------------------------------------------------------
GENERIC_RAY = cc.family("generic")
GENERIC_TRACK = [c for c in TRACK if not c.exact]


def _speed(case, shape):
    """voxels per unit of z of every ray"""
    H, W = shape
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xf, yf = (uu - case.cam["cx"]) / case.cam["fx"], (vv - case.cam["cy"]) / case.cam["fy"]
    return np.sqrt(xf * xf + yf * yf + 1.0) / cc.VOXEL


def _track_positions(w):
    return w["ijk"].astype(np.float64) + w["f"].astype(np.float64)


def test_generic_deviation_is_what_the_bounds_were_taken_from():
    worst_x, worst_ulp = 0.0, 0.0
    for case in GENERIC_RAY:
        d, _, _, s = restated(case)
        md, _, _, ms, margin, _ = cc.model(case.name)
        both = (d > 0) & (md > 0) & (s == ms)
        dev = np.abs(d.astype(np.float64) - md)
        x = (dev * _speed(case, d.shape))[both].max()
        ulp = (dev[both & (margin >= DELTA)] / np.spacing(d[both & (margin >= DELTA)]).astype(np.float64)).max()
        print(f"{case.name}: largest |x_f32 - x_f64| at a hit {x:.3e} voxel; largest |z*_f32 - z*_f64| on kept rays {ulp:.2f} ulp")
        worst_x, worst_ulp = max(worst_x, x), max(worst_ulp, ulp)
    for case in GENERIC_TRACK:
        w, m = restated(case), cc.model(case.name)
        common = sorted(set(m["uv"]) & set(zip(w["u"].tolist(), w["v"].tolist())))
        iw = {uv: i for i, uv in enumerate(zip(w["u"].tolist(), w["v"].tolist()))}
        im = {uv: i for i, uv in enumerate(m["uv"])}
        x = np.abs(_track_positions(w)[[iw[q] for q in common]] - m["x"][[im[q] for q in common]]).max()
        print(f"{case.name}: largest |x_f32 - x_f64| at a sample {x:.3e} voxel")
        worst_x = max(worst_x, x)
    print(f"largest deviation {worst_x:.3e} voxel -> DELTA {DELTA:.3e}; largest depth deviation {worst_ulp:.2f} ulp -> DEPTH_ULPS {DEPTH_ULPS}")
    assert 4.0 * worst_x < DELTA <= 8.0 * worst_x                                    # the next power of two above four times it
    assert 4.0 * worst_ulp <= DEPTH_ULPS < 4.0 * worst_ulp + 1.0


@pytest.mark.parametrize("case", GENERIC_RAY, ids=ids(GENERIC_RAY))
def test_generic_rays_agree_with_the_model_away_from_decisions(case):
    d, n, bgr, s = restated(case)
    md, mn, mbgr, ms, margin, _ = cc.model(case.name)
    aside = margin < DELTA                                                            # by the fp64 march alone
    print(case.name, "set aside", int(aside.sum()), "of", aside.size, "hits", int((md > 0).sum()))
    assert aside.sum() <= 0.02 * aside.size
    assert not any(aside[v, u] for u, v in case.named)
    keep = ~aside
    assert np.array_equal((d > 0)[keep], (md > 0)[keep]) and np.array_equal(s[keep], ms[keep]) and np.array_equal(bgr[keep], mbgr[keep])
    assert (md > 0).sum() > 100 and (md == 0).sum() > 30
    hit = keep & (md > 0)
    dev = np.abs(d.astype(np.float64) - md)[hit]
    bound = DEPTH_ULPS * np.spacing(d[hit]).astype(np.float64)
    assert (dev <= bound).all(), (dev / bound).max()
    # the normal is g / |g| of a gradient that changes by less than 4 per voxel and axis: moving the point by the depth bound (in
    # voxels) turns it by less than 8 dx / |g|; |g| >= 1/2 wherever a {-1, 0, 1} field crosses zero between defined samples.  The
    # f32 normalisation and rotation add a few 2^-24.
    dx = bound * _speed(case, d.shape)[hit]
    cosang = np.clip((n[hit].astype(np.float64) * mn[hit]).sum(axis=-1), -1.0, 1.0)
    lit = np.abs(mn[hit]).sum(axis=-1) > 0
    assert np.array_equal(lit, np.abs(n[hit]).sum(axis=-1) > 0)
    assert (np.arccos(cosang[lit]) <= 16.0 * dx[lit] + 1e-3 * 2.0 ** -10).all(), np.arccos(cosang[lit]).max()


@pytest.mark.parametrize("case", GENERIC_TRACK, ids=ids(GENERIC_TRACK))
def test_generic_samples_agree_with_the_model_away_from_decisions(case):
    w, m = restated(case), cc.model(case.name)
    H, W = case.cam["height"], case.cam["width"]
    grid = [(u, v) for v in range(0, H, case.stride) for u in range(0, W, case.stride)]
    assert len(grid) == len(m["margin"])
    aside = {uv for uv, mg in zip(grid, m["margin"]) if mg < DELTA}
    print(case.name, "set aside", len(aside), "of", len(grid), "n_corr", w["n_corr"], m["n_corr"], "n_src", w["n_src"], m["n_src"])
    assert len(aside) <= 0.02 * len(grid)
    got, want = set(zip(w["u"].tolist(), w["v"].tolist())) - aside, set(m["uv"]) - aside
    assert got == want and len(want) > 400
    if not aside:
        assert (w["n_src"], w["n_corr"]) == (m["n_src"], m["n_corr"])
    iw = {uv: i for i, uv in enumerate(zip(w["u"].tolist(), w["v"].tolist()))}
    im = {uv: i for i, uv in enumerate(m["uv"])}
    order = sorted(want)
    Jw, Jm = w["J"][[iw[q] for q in order]].astype(np.float64), m["J"][[im[q] for q in order]]
    rw, rm = w["r"][[iw[q] for q in order]].astype(np.float64), m["r"][[im[q] for q in order]]
    # r = trunc F and J = [p x n, n] with |n| <= 4 sqrt(3) trunc / voxel: a point DELTA / 4 off (the measured deviation) changes F by less
    # than DELTA and n by less than 4 DELTA * trunc / voxel per component; |p| < 1 here
    assert np.abs(rw - rm).max() <= cc.TRUNC * DELTA
    assert np.abs(Jw - Jm).max() <= 2.0 * 4.0 * DELTA * cc.TRUNC / cc.VOXEL
