"""The crafted ICP pairs (icp_edges_common) on the CPU: the C oracle and the numpy formulation give the same maps bit for bit, the
same counts and the same sums; the restated rule (counters) agrees with both; every exit of the rule is hit somewhere in its family;
the dyadic cases' sums are exact.  tests/test_gpu_icp_edges.py runs the same pairs through the HIP kernels."""
import math

import numpy as np
import pytest

import icp_edges_common as ic
from loop_closure_common import sym6
from oracle import second_numpy as sn

EPS = 2.0 ** -52
CASES = ic.cases()

# the exits and edges each family is there for: the family's total must be non-zero
MUST_HIT = dict(
    validity=("src_zero", "src_nan", "src_inf", "src_negative", "src_eq_min", "src_eq_max", "src_next_above_min", "src_next_below_max",
              "src_scale_makes_valid", "src_scale_makes_invalid", "gated", "accepted"),
    pz=("pz_eq_0", "pz_lt_0", "pz_subnormal", "pz_subnormal_accepted", "out_of_window", "tie_v", "accepted"),
    ties=("tie_u", "tie_v", "tie_uv", "tie_u_candidates_differ", "tie_v_candidates_differ", "uf_eq_left", "uf_eq_right", "vf_eq_top",
          "vf_eq_bottom", "out_of_window", "accepted"),
    target=("target_border", "target_hole", "target_neighbour", "target_jump", "target_at_jump", "target_one_float_past_jump", "accepted"),
    gate=("gate_eq", "gate_one_float_inside", "gate_one_float_outside", "gated", "accepted"),
    walk=("tie_u", "tie_u_candidates_differ", "target_border", "target_hole", "target_neighbour", "target_jump", "uf_eq_right", "accepted"),
    smoothing=("target_border", "target_hole", "target_neighbour", "target_jump", "accepted"),
)


@pytest.fixture(scope="module")
def references():
    """per case name: maps, sums and counters of both references, computed once"""
    out = {}
    for case in CASES:
        g = ic.geometry(case)
        mc, mn = ic.maps_c(case), ic.maps_numpy(case)
        orc = ic.c_oracle_for(case)
        sums, cnt, nsrc = orc.icp_sums(mc[0], mc[2], case.T, stride=case.stride, max_dist=case.max_dist, scale_src=case.scale)
        A, b, e, cnt_n, nsrc_n = sn.icp_sums(g, mn[0], mn[2], case.T, stride=case.stride, max_dist=case.max_dist, scale_src=case.scale)
        out[case.name] = dict(maps_c=mc, maps_n=mn, c=(sym6(sums), sums[21:27], sums[27], cnt, nsrc), n=(A, b, e, cnt_n, nsrc_n),
                              counters=ic.counters(case, *mn))
    return out


def _within_reordering_bound(A, b, e, A0, b0, e0, cnt):
    """the bound of test_gpu_icp_eval._check_against_oracle: an fp64 sum of n_corr terms, reordered"""
    d_a = np.abs(A - A0) / np.maximum(np.sqrt(np.outer(np.diag(A0), np.diag(A0))), 1e-300)
    d_b = np.abs(b - b0) / np.maximum(np.sqrt(np.diag(A0) * e0), 1e-300)
    d_e = abs(e - e0) / max(e0, 1e-300)
    return d_a.max() <= cnt * EPS and d_b.max() <= cnt * EPS and d_e <= cnt * EPS


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_two_references_and_the_restated_rule_agree(case, references):
    ref = references[case.name]
    for which, a, b in zip(("source depth", "target depth", "normal map"), ref["maps_c"], ref["maps_n"]):
        assert ic.same_bits(a, b), f"{case.name}: {which} differs between the C oracle and the numpy formulation"
    A, b, e, cnt, nsrc = ref["c"]
    A_n, b_n, e_n, cnt_n, nsrc_n = ref["n"]
    k = ref["counters"]
    print(case.name, "n_corr", cnt, cnt_n, k["n_corr"], "n_src", nsrc, nsrc_n, k["n_src"])
    assert cnt == cnt_n == k["n_corr"] and nsrc == nsrc_n == k["n_src"]
    assert _within_reordering_bound(A_n, b_n, e_n, A, b, e, cnt)
    exits = k["n_samples"] - k["n_src"] + k["pz_eq_0"] + k["pz_lt_0"] + k["out_of_window"] + k["gated"] + k["accepted"]
    exits += k["target_border"] + k["target_hole"] + k["target_neighbour"] + k["target_jump"] + k["target_degenerate"]
    assert exits == k["n_samples"] == case.n_samples                       # every sample leaves by exactly one named exit


@pytest.mark.parametrize("case", [c for c in CASES if c.exact], ids=[c.name for c in CASES if c.exact])
def test_dyadic_sums_are_exact(case, references):
    ref = references[case.name]
    J, r = ic.terms(case, ref["maps_n"][0], ref["maps_n"][2])
    A, b, e = ref["c"][:3]
    A_n, b_n, e_n = ref["n"][:3]
    assert J.shape[1] == ref["c"][3]

    def three_ways(x, y):
        p = (x * y).tolist()                                               # f32 x f32: exact in fp64
        fwd, bwd = 0.0, 0.0
        for q in p:
            fwd += q
        for q in reversed(p):
            bwd += q
        assert fwd == bwd == math.fsum(p), case.name
        return fwd
    for i in range(6):
        for j in range(i, 6):
            s = three_ways(J[i], J[j])
            assert s == A[i, j] == A_n[i, j] == A_n[j, i], (case.name, i, j)
        s = three_ways(J[i], r)
        assert s == b[i] == b_n[i], (case.name, i)
    assert three_ways(r, r) == e == e_n


@pytest.mark.parametrize("fam", ic.FAMILIES)
def test_every_edge_of_the_family_is_hit(fam, references):
    total = {k: 0 for k in ic.COUNTER_NAMES}
    for case in ic.family(fam):
        for k, v in references[case.name]["counters"].items():
            total[k] += v
    print(fam, {k: v for k, v in total.items() if v})
    missing = [k for k in MUST_HIT[fam] if total[k] == 0]
    assert not missing, (fam, missing)


def test_ties_are_total_and_some_would_change_the_count(references):
    """with the all-valid half of the source, every sample of a tie pose is a tie; where the two candidates differ in validity, the
    other rounding changes n_corr"""
    for name in ("tie_u", "tie_v", "tie_uv", "tie_u_neg", "tie_uv_neg", "tie_uv_far"):
        k = references[name]["counters"]
        case = next(c for c in CASES if c.name == name)
        m = ic.sample_rule(case, *[references[name]["maps_n"][i] for i in (0, 2)])
        plain = m["reach"] & (m["d"] == 1)                                 # the depth-1 plane itself, not its odd pixels
        assert max(k["tie_u"], k["tie_v"]) == plain.sum() > 600, (name, k)
        assert k["tie_u_candidates_differ"] + k["tie_v_candidates_differ"] > 0, name
    assert references["tie_uv"]["counters"]["tie_uv"] == references["tie_uv"]["counters"]["tie_u"]


def test_the_subnormal_pz_sample_is_accepted(references):
    """pixel (0, 12): px = py = 0, pz = 2^-127 * 20/32 -- 1 / pz is finite only as the IEEE quotient"""
    k = references["pz_subnormal"]["counters"]
    assert k["pz_subnormal_accepted"] == 1 == k["n_corr"] and k["pz_subnormal"] == 20 * ic.BASE_H
    assert references["pz_subnormal"]["c"][3] == 1


@pytest.mark.parametrize("md", [0.05, 0.0625, 0.1])
def test_gate_frames_straddle_the_gate(md, references):
    case = next(c for c in CASES if c.name == f"gate_{md}")
    frame, n_eq = ic.gate_frame(md)
    m = ic.sample_rule(case, *[references[case.name]["maps_n"][i] for i in (0, 2)])
    uu, vv = np.meshgrid(np.arange(ic.BASE_W), np.arange(ic.BASE_H))
    assert m["reach"].all() and np.array_equal(m["ut"], uu) and np.array_equal(m["vt"], vv)      # every sample projects to its own pixel
    inside = (uu + vv) % 2 == 0
    interior = m["tvalid"]
    assert interior.sum() == (ic.BASE_W - 2) * (ic.BASE_H - 2)
    assert np.array_equal(m["code"][interior] == ic.ACCEPTED, inside[interior])
    assert np.array_equal(m["code"][interior] == ic.GATED, ~inside[interior])
    k = references[case.name]["counters"]
    print(md, "dist2 == md2 on", n_eq, "pixels;", k)
    assert k["gate_one_float_inside"] == k["accepted"] > 0 and k["gate_one_float_outside"] == k["gated"] > 0
    assert n_eq > 0 if md != 0.0625 else True
    # the f32 gate squared in f32 is not the double's square rounded, for two of the three
    assert (np.float32(np.float32(md) * np.float32(md)) != np.float32(md * md)) == (md != 0.0625)


def test_the_walk_reaches_the_pipeline_break_points():
    """threads of the evaluation / batched kernels (members of 256 threads, four samples per trip) hold 0, 1, 3, 4, 5, 8 and 9 samples
    somewhere in the family: no trip, one ragged trip, one full trip, a second trip with one sample, two full trips, a third"""
    seen = {}
    for case in ic.family("walk"):
        n = case.n_samples
        assert ic.members(n) == ic.members(n, ic.BATCH_MEMBERS_CAP)
        seen[case.name] = set(ic.samples_per_thread(n, ic.members(n)).tolist())
    assert seen["walk_40x24_s1"] == {3, 4} and seen["walk_41x25_s1"] == {4, 5} and seen["walk_131x67_s2"] == {8, 9}
    assert seen["walk_37x1_s1"] == {0, 1} and seen["walk_1x1_s1"] == {0, 1} and seen["walk_40x24_s5"] == {0, 1}
    assert set().union(*seen.values()) >= {0, 1, 3, 4, 5, 8, 9}
    assert ic.members(131 * 67) == 2 and ic.members(700 * 13) == 2 and 2 * 256 < 700      # two members; step = 512 < Ws
    assert ic.members(300 * 3) == 1 and 300 > 256                                        # dvs == 0 with one member
    assert {w % 4 for w, _ in ic.WALK} == {0, 1, 2, 3}
    assert any(s > h for (w, h), (strides, _) in ic.WALK.items() for s in strides)       # a stride larger than H
