"""CPU: the numpy restatement of the global registration (tests/cloud_global_reference.py) is held to independent formulations and
to the property the feature exists for, before the GPU is held to it (tests/test_gpu_cloud_global.py).

The condition.  On the four-solids scene (2 600 independently sampled points per cloud, planted motion 130 degrees and 1.4 m,
k = 48 within 0.15 m, 20 000 hypotheses, 3 cm threshold) the recipe must leave every source point within 0.10 m of where the planted
pose puts it: half the local ICP's default gate of 0.20 m, so the ICP is entitled to take over.  It is a condition, not a
measurement.  Recorded with this file's seeds (scene 1 / 2, noise 3, RANSAC 0), largest displacement / inliers of m / true pairs:
    no noise, mutual pairs   0.0128 m   64 of  754   15.3 %        no noise, all pairs   0.0262 m  153 of 2600   11.6 %
    2 mm noise, mutual       0.0342 m   44 of  554   14.6 %        2 mm noise, all       0.0108 m  174 of 2600   11.4 %
"""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import cloud_global_common as cc
import cloud_global_reference as gr

GATE = 0.20                                     # FusionContext.CLOUD_LEVELS' first max_dist


@pytest.mark.parametrize("noise", [0.0, 0.002])
@pytest.mark.parametrize("mutual", [True, False])
def test_the_recipe_lands_inside_half_the_icp_gate(noise, mutual):
    s, r = cc.scene(noise), cc.scene_recipe(noise, mutual)
    moved = s["src"].astype(np.float64) @ s["T"][:3, :3].T + s["T"][:3, 3]
    true = np.linalg.norm(moved[r["corr"][:, 0]] - s["tgt"][r["corr"][:, 1]].astype(np.float64), axis=1) < 0.05
    disp = cc.displacement(r["T"], s["T"], s["src"])
    print(f"noise {noise} mutual {mutual}: displacement {disp:.4f} m, inliers {r['inliers']} of {r['m']}, scored {r['n_passed']} of "
          f"{cc.HYPOTHESES}, mutual pairs {r['n_mutual']}, true correspondences {100 * true.mean():.1f} %, best_h {r['best_h']}")
    assert r["status"] == 1 and r["mutual"] == mutual
    assert disp <= GATE / 2


def test_no_case_the_gpu_is_compared_on_is_undecided():
    for name in cc.FPFH_CASES:
        assert cc.fpfh_ref(name)["undecided"] == 0, name
    for name in cc.RANSAC_CASES:
        assert cc.ransac_ref(name)["undecided"] == 0, name
    for mutual in (True, False):
        r = cc.scene_recipe(0.0, mutual)
        assert r["undecided"] == 0 and r["fs"]["undecided"] == 0 and r["ft"]["undecided"] == 0


def test_the_cases_hold_what_they_are_for():
    assert cc.ransac_ref("all_fail")["status"] == 2 and cc.ransac_ref("all_fail")["n_passed"] == 0
    thr = cc.ransac_ref("threshold")
    assert thr["on_threshold"] > 0 and thr["inliers"] == 4
    # (a few ulps of 4: most of the passing triads have edges of length sqrt 2)
    assert np.abs(thr["T"] - np.array([[1, 0, 0, 4], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])).max() <= 2e-15
    m3 = cc.ransac_ref("m3")
    assert m3["inliers"] == 3 and 0 < m3["n_passed"] < 64
    par = cc.fpfh_ref("parallel")
    assert par["spfh"][1, 33] < (par["members"][1] >= 0).sum()          # the pairs along x were skipped
    iso = cc.fpfh_ref("isolated")
    assert not iso["fpfh"][77].any() and not iso["spfh"][77].any()
    z = cc.fpfh_ref("zero_normals")
    assert not z["spfh"][::5].any() and not z["fpfh"][::5].any() and z["spfh"][1::5, 33].all()
    lat = cc.fpfh_case("lattice_ties")
    _, d2 = gr.knn_lists(lat["xyz"], lat["k"] + 1, lat["radius"])
    assert (d2[:, lat["k"] - 1] == d2[:, lat["k"]]).any()               # a tie across the k-th place
    a, b = cc.match_case("ties")
    _, dist = cc.match_ref("ties")
    assert ((((a[:, None, :] - b[None, :, :]) ** 2).sum(-1) == dist[:, None]).sum(1) >= 3).all()      # every minimum is met three times


def test_generator_against_hand_computed_draws():
    # computed with arbitrary-precision integers: mix(seed + 0x9E3779B97F4A7C15 * (3 h + j + 1) mod 2^64) mod m
    assert gr.mix(np.array([0x9E3779B97F4A7C15], np.uint64))[0] == 0x9CA066F1A4AB2EEA
    assert gr.draws(0, 2, 754).tolist() == [[450, 451, 387], [430, 147, 314]]
    assert gr.draws(5, 8, 1000)[7].tolist() == [174, 214, 850]
    assert gr.draws(2 ** 64 - 1, 12346, 3)[12345].tolist() == [1, 0, 1]             # the seed wraps


def test_triad_pose_is_orthonormal_and_maps_the_source_frame():
    rng = np.random.default_rng(0)
    s = rng.uniform(-1, 1, (500, 3, 3))
    Rt = np.stack([cc.rotation(rng.normal(size=3), rng.uniform(0, 180)) for _ in range(500)])
    t = np.einsum("nij,nkj->nki", Rt, s) + rng.uniform(-2, 2, (500, 1, 3))
    R, tr, ok = gr.triad_pose(s, t)
    assert ok.all()
    assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() <= 1e-14
    assert np.abs(np.linalg.det(R) - 1).max() <= 1e-14
    assert np.abs(np.einsum("nij,nkj->nki", R, s) + tr[:, None, :] - t).max() <= 1e-12    # a rigid triple: all three points land
    # a non-congruent triple: the frames still map (x to x, the planes' normals), and the means
    t2 = t + rng.normal(0, 0.05, t.shape)
    R2, tr2, _ = gr.triad_pose(s, t2)
    xs, ys, zs, _ = gr.triad(s[:, 0], s[:, 1], s[:, 2])
    xt, yt, zt, _ = gr.triad(t2[:, 0], t2[:, 1], t2[:, 2])
    for u, v in ((xs, xt), (ys, yt), (zs, zt)):
        assert np.abs(np.einsum("nij,nj->ni", R2, u) - v).max() <= 1e-14
    assert np.abs(np.einsum("nij,nj->ni", R2, s.mean(1)) + tr2 - t2.mean(1)).max() <= 1e-14
    # collinear points have no frame
    line = np.array([[[0, 0, 0], [1, 1, 1], [2, 2, 2.0]]])
    assert not gr.triad_pose(line, line)[2][0]


def test_subsample_keeps_the_first_point_of_every_cell():
    for name in cc.SUB_CASES:
        p, voxel = cc.sub_case(name)
        idx = gr.voxel_subsample(p, voxel)
        cell = np.floor(p.astype(np.float64) / voxel).astype(np.int64)
        assert np.all(np.diff(idx) > 0)
        assert len(np.unique(cell[idx], axis=0)) == len(idx) == len(np.unique(cell, axis=0))
        first = {}
        for i, c in enumerate(map(tuple, cell)):
            first.setdefault(c, i)
        assert sorted(first.values()) == idx.tolist()
    far = np.array([[(1 << 20) / 16.0, 0, 0]], np.float32)
    with pytest.raises(ValueError):
        gr.voxel_subsample(far, 1 / 16)
    assert len(gr.voxel_subsample(cc.sub_case("one_voxel")[0], 0.5)) == 1
    assert gr.voxel_subsample(cc.sub_case("cell_limit")[0], 1 / 16).tolist() == [0, 1, 2, 3]      # the fifth shares the first's voxel


def test_neighbourhoods_and_matches_against_a_kd_tree():
    c = cc.fpfh_case("scene_k32")
    p = c["xyz"].astype(np.float64)
    idx, d2 = gr.knn_lists(p, 32, c["radius"])
    d, j = cKDTree(p).query(p, k=32, distance_upper_bound=c["radius"])
    assert np.array_equal(np.isfinite(d), idx >= 0)
    assert np.allclose(np.where(idx >= 0, np.sqrt(d2), 0), np.where(np.isfinite(d), d, 0), rtol=1e-12, atol=0)
    a, b = cc.match_case("dim33")
    index, dist = cc.match_ref("dim33")
    dk, jk = cKDTree(b.astype(np.float64)).query(a.astype(np.float64))
    assert np.array_equal(index, jk) and np.allclose(np.sqrt(dist), dk, rtol=1e-12)


def _pair_feature(pi, ni, pj, nj):
    """one pair, scalar by scalar, with numpy's own cross / dot: a second formulation of the contract's pair feature"""
    d = pj - pi
    L = np.sqrt(d @ d)
    a1, a2 = ni @ d / L, nj @ d / L
    ns, nt, f3 = (nj, ni, -a2) if abs(a1) < abs(a2) else (ni, nj, a1)
    if abs(a1) < abs(a2):
        d = -d
    v = np.cross(d, ns)
    if not v.any():
        return None
    v = v / np.linalg.norm(v)
    w = np.cross(ns, v)
    return np.arctan2(w @ nt, ns @ nt), v @ nt, f3


def test_spfh_counts_against_a_pair_by_pair_formulation():
    for name in ("duplicates", "zero_normals", "parallel", "k_gt_n"):
        c, ref = cc.fpfh_case(name), cc.fpfh_ref(name)
        p, nr = c["xyz"].astype(np.float64), c["normals"].astype(np.float64)
        for i in range(0, len(p), 7):
            cnt, m = np.zeros(33, int), 0
            for j in ref["members"][i]:
                if j < 0 or not nr[i].any():
                    continue
                f = _pair_feature(p[i], nr[i], p[j], nr[j])
                if f is None:
                    continue
                for off, u in ((0, 11 * (f[0] + np.pi) / (2 * np.pi)), (11, 11 * (f[1] + 1) / 2), (22, 11 * (f[2] + 1) / 2)):
                    cnt[off + int(min(max(np.floor(u), 0), 10))] += 1
                m += 1
            assert ref["spfh"][i].tolist() == cnt.tolist() + [m], (name, i)
    # the descriptor's groups: each sums to 100 (neighbours) + 100 (own) where the point has counted neighbours
    ref = cc.fpfh_ref("scene_k32")
    full = ref["spfh"][:, 33] > 0
    sums = ref["fpfh"].astype(np.float64).reshape(-1, 3, 11).sum(-1)
    assert full.sum() > 1000 and np.allclose(sums[full], 200.0, rtol=1e-5)
