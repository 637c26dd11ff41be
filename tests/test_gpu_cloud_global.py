"""GPU: the global registration front end (kernels_cloudglobal.hip: tl3d_cloud_voxel_subsample, tl3d_cloud_fpfh, tl3d_feature_match,
tl3d_cloud_ransac; metrics.global_align_clouds) against the numpy restatement of its contracts
(tests/cloud_global_reference.py, held to independent formulations in tests/test_cloud_global_reference_cpu.py) on the cases of
tests/cloud_global_common.py.

Integers are exact: the kept indices, the SPFH counts, the matched indices, every hypothesis' count, best_h, inliers, n_passed.  The
CPU file asserts that no compared case has an undecided decision (a feature within 1e-9 of a bin edge, a score within 1e-12 of the
threshold), so nothing is tolerated here.  The squared feature distances are bit-equal (one stated order of exact-input operations).
The FPFH bar.  Every TERM of S[b] is bit-identical by contract (integers, two divisions), so S[b] differs from the reference's by the
order of its additions at most: e_b = n_terms * 2^-52 * sum |term|.  Through the group scaling f = 100 / sum (sum carries the e's of
its 11 bins and 11 roundings) and the own term: |dF_b| <= f e_b + f S[b] (sum_group e + 11 * 2^-52 sum) / sum + 4 * 2^-52 |F_b| for
the multiplication, the division, the product and the addition, plus 2^-23 |F_b| for one f32 rounding on either side.  The reference
computes the bar per entry from its own sums (cloud_global_reference.fpfh).
The pose T of the RANSAC is a handful of fp64 operations on exact inputs: within 1e-12 of the reference's.
"""
import ctypes as C

import numpy as np
import pytest

import cloud_global_common as cc
import cloud_global_reference as gr
import tl3d
from tl3d import _cabi as abi
from tl3d import metrics

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as c:
        yield c


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                # (a copy: the cases are read-only)


# ---- subsample -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.SUB_CASES)
def test_subsample_keeps_the_reference_indices(ctx, name):
    p, voxel = cc.sub_case(name)
    got = ctx.voxel_subsample(p, voxel)
    assert got.dtype == np.int32 and np.array_equal(got, gr.voxel_subsample(p, voxel))
    assert np.array_equal(ctx.voxel_subsample(_dev(p), voxel).cpu().numpy(), got)


def test_subsample_refusals(ctx):
    far = np.array([[0, 0, 0], [(1 << 20) / 16.0, 0, 0]], np.float32)           # cell 2^20
    with pytest.raises(abi.Tl3dError, match="2\\^20"):
        ctx.voxel_subsample(far, 1 / 16)
    with pytest.raises(abi.Tl3dError, match="2\\^20"):
        ctx.voxel_subsample(-far, 1 / 16 * (1 - 2.0 ** -30))                     # cell -(2^20) - 1
    p = cc.sub_case("n255")[0]
    for voxel in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(abi.Tl3dError, match="voxel"):
            ctx.voxel_subsample(p, voxel)
    bad = p.copy()
    bad[17, 1] = np.nan
    with pytest.raises(abi.Tl3dError, match="non-finite"):
        ctx.voxel_subsample(bad, 0.1)
    assert len(ctx.voxel_subsample(np.zeros((0, 3), np.float32), 0.1)) == 0
    n = C.c_int64(7)
    lib = ctx._lib
    assert lib.tl3d_cloud_voxel_subsample(ctx._h, abi.ptr(p), len(p), 0.1, None, C.byref(n)) == abi.E_INVALID
    assert lib.tl3d_cloud_voxel_subsample(ctx._h, abi.ptr(p), -1, 0.1, abi.ptr(p), C.byref(n)) == abi.E_INVALID
    assert lib.tl3d_cloud_voxel_subsample(ctx._h, abi.ptr(p), 1 << 31, 0.1, abi.ptr(np.zeros(4, np.int32)), C.byref(n)) == abi.E_INVALID
    assert lib.tl3d_cloud_voxel_subsample(ctx._h, abi.ptr(p), len(p), 0.1, abi.ptr(p), C.byref(n)) == abi.E_INVALID        # aliased
    idx = np.full(len(bad), -5, np.int32)                        # a refusal from the bounds pass writes nothing
    assert lib.tl3d_cloud_voxel_subsample(ctx._h, abi.ptr(bad), len(bad), 0.1, abi.ptr(idx), C.byref(n)) == abi.E_INVALID
    assert lib.tl3d_cloud_voxel_subsample(ctx._h, abi.ptr(far), len(far), 1 / 16, abi.ptr(idx), C.byref(n)) == abi.E_INVALID
    assert n.value == 7 and np.all(idx == -5)


# ---- FPFH ----------------------------------------------------------------------------------------------------------------------
def _fpfh(ctx, c, **over):
    kw = dict(nb_neighbors=c["k"], max_radius=c["radius"], cell_size=0.07, spfh=True)
    kw.update(over)
    return ctx.compute_fpfh(c["xyz"], c["normals"], **kw)


@pytest.mark.parametrize("name", cc.FPFH_CASES)
def test_fpfh_matches_the_reference(ctx, name):
    c, ref = cc.fpfh_case(name), cc.fpfh_ref(name)
    f, s = _fpfh(ctx, c)
    assert s.dtype == np.int32 and np.array_equal(s, ref["spfh"]), f"{name}: SPFH counts differ in {(s != ref['spfh']).any(1).sum()} rows"
    err = np.abs(f.astype(np.float64) - ref["fpfh"].astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(ref["bar"] > 0, err / ref["bar"], 0.0)))
    print(f"{name}: {len(f)} points, counted pairs {int(s[:, 33].sum())}, largest error / bar {worst:.3g}, "
          f"rows bit-equal {int((f == ref['fpfh']).all(1).sum())}")
    assert np.all(err <= ref["bar"]), f"{name}: off by {err.max():.3g}"
    assert np.all(f[ref["spfh"][:, 33] == 0] == 0)


def test_fpfh_same_bytes_for_cell_sizes_arrays_and_runs(ctx):
    for name in ("scene_k48", "lattice_ties", "duplicates"):
        c = cc.fpfh_case(name)
        f0, s0 = _fpfh(ctx, c)
        for cell in (0.021, 0.15, 1.7):
            f, s = _fpfh(ctx, c, cell_size=cell)
            assert f.tobytes() == f0.tobytes() and s.tobytes() == s0.tobytes(), (name, cell)
        f, s = _fpfh(ctx, c)
        assert f.tobytes() == f0.tobytes() and s.tobytes() == s0.tobytes()
        fd, sd = ctx.compute_fpfh(_dev(c["xyz"]), _dev(c["normals"]), nb_neighbors=c["k"], max_radius=c["radius"], cell_size=0.07, spfh=True)
        assert fd.cpu().numpy().tobytes() == f0.tobytes() and sd.cpu().numpy().tobytes() == s0.tobytes()
        assert ctx.compute_fpfh(c["xyz"], c["normals"], nb_neighbors=c["k"], max_radius=c["radius"]).tobytes() == f0.tobytes()   # no spfh_out


def test_fpfh_refusals(ctx):
    c = cc.fpfh_case("k_gt_n")
    for k in (3, 65):
        with pytest.raises(abi.Tl3dError, match="nb_neighbors"):
            ctx.compute_fpfh(c["xyz"], c["normals"], nb_neighbors=k)
    with pytest.raises(abi.Tl3dError, match="cell_size"):
        ctx.compute_fpfh(c["xyz"], c["normals"], cell_size=0.0)
    bad = c["xyz"].copy()
    bad[2, 0] = np.inf
    with pytest.raises(abi.Tl3dError, match="non-finite"):
        ctx.compute_fpfh(bad, c["normals"])
    none = np.zeros((0, 3), np.float32)
    assert ctx.compute_fpfh(none, none).shape == (0, 33)
    out = np.zeros((6, 33), np.float32)
    lib = ctx._lib
    assert lib.tl3d_cloud_fpfh(ctx._h, abi.ptr(c["xyz"]), None, 6, 8, 0.0, 0.1, abi.ptr(out), None) == abi.E_INVALID
    assert lib.tl3d_cloud_fpfh(ctx._h, abi.ptr(c["xyz"]), abi.ptr(c["normals"]), 6, 8, 0.0, 0.1, abi.ptr(c["xyz"]), None) == abi.E_INVALID


# ---- match ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.MATCH_CASES)
def test_match_is_exact(ctx, name):
    a, b = cc.match_case(name)
    ref_i, ref_d = cc.match_ref(name)
    idx, d2 = ctx.match_features(a, b, dist2=True)
    assert idx.dtype == np.int32 and np.array_equal(idx, ref_i), f"{name}: {(idx != ref_i).sum()} indices differ"
    assert d2.tobytes() == ref_d.tobytes(), f"{name}: squared distances are not bit-equal"
    di, dd = ctx.match_features(_dev(a), _dev(b), dist2=True)
    assert np.array_equal(di.cpu().numpy(), idx) and dd.cpu().numpy().tobytes() == d2.tobytes()
    assert np.array_equal(ctx.match_features(a, b), idx)


def test_match_edges_and_refusals(ctx):
    a, b = cc.match_case("ties")
    idx, _ = cc.match_ref("ties")
    assert idx.max() < 40                                       # b's rows repeat at +40 and +80: the first copy wins
    idx, d2 = ctx.match_features(a, np.zeros((0, 33), np.float32), dist2=True)
    assert np.all(idx == -1) and np.all(np.isposinf(d2))
    assert len(ctx.match_features(np.zeros((0, 33), np.float32), b)) == 0
    # rows none of whose distances is finite: (d2, index) has its minimum at index 0 all the same
    idx, d2 = ctx.match_features(np.array([[np.inf, 0], [0, 0], [np.nan, 1]], np.float32), np.array([[5, 5], [6, 6], [7, 7], [1, 1]], np.float32),
                                 dist2=True)
    assert idx.tolist() == [0, 3, 0] and np.isposinf(d2[0]) and d2[1] == 2.0 and np.isposinf(d2[2])
    lib, one = ctx._lib, np.zeros(64, np.float32)
    # the size refusal comes before any allocation or access: the pointers are never followed
    assert lib.tl3d_feature_match(ctx._h, abi.ptr(one), (1 << 17) + 1, abi.ptr(one), 1 << 17, 33, None, None) == abi.E_INVALID
    assert b"subsample" in lib.tl3d_last_error()
    assert lib.tl3d_feature_match(ctx._h, abi.ptr(one), 1 << 17, abi.ptr(one), 1 << 17, 33, None, None) == abi.OK        # 2^34 itself, no output asked
    for dim in (0, 65):
        assert lib.tl3d_feature_match(ctx._h, abi.ptr(one), 1, abi.ptr(one), 1, dim, None, None) == abi.E_INVALID
    assert lib.tl3d_feature_match(ctx._h, abi.ptr(one), -1, abi.ptr(one), 1, 4, None, None) == abi.E_INVALID
    assert lib.tl3d_feature_match(ctx._h, abi.ptr(one), 1 << 31, abi.ptr(one), 1, 4, None, None) == abi.E_INVALID
    assert lib.tl3d_feature_match(ctx._h, abi.ptr(one), 2, abi.ptr(one), 2, 4, abi.ptr(one), None) == abi.E_INVALID        # aliased


# ---- RANSAC --------------------------------------------------------------------------------------------------------------------
def _ransac(ctx, c, dev=False):
    f = _dev if dev else (lambda a: a)
    return ctx.ransac_register(f(c["src"]), f(c["tgt"]), f(c["corr"]), hypotheses=c["hypotheses"], max_dist=c["max_dist"],
                               edge_ratio=c["edge_ratio"], seed=c["seed"], counts=True)


@pytest.mark.parametrize("name", cc.RANSAC_CASES)
def test_ransac_matches_the_reference(ctx, name):
    c, ref = cc.ransac_case(name), cc.ransac_ref(name)
    got = _ransac(ctx, c)
    assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], ref["counts"]), \
        f"{name}: {(got['counts'] != ref['counts']).sum()} of {len(ref['counts'])} counts differ"
    for k in ("status", "best_h", "inliers", "n_passed", "m"):
        assert got[k] == ref[k], f"{name}: {k} {got[k]} != {ref[k]}"
    err = float(np.abs(got["T"] - ref["T"]).max())
    print(f"{name}: m {got['m']}, scored {got['n_passed']} of {c['hypotheses']}, best_h {got['best_h']}, inliers {got['inliers']}, |dT| {err:.3g}")
    assert err <= 1e-12
    again = _ransac(ctx, c)
    assert again["T"].tobytes() == got["T"].tobytes() and again["counts"].tobytes() == got["counts"].tobytes()
    dev = _ransac(ctx, c, dev=True)
    assert dev["T"].tobytes() == got["T"].tobytes() and np.array_equal(dev["counts"].cpu().numpy(), got["counts"])
    nc = ctx.ransac_register(c["src"], c["tgt"], c["corr"], hypotheses=c["hypotheses"], max_dist=c["max_dist"], edge_ratio=c["edge_ratio"],
                             seed=c["seed"])
    assert nc["T"].tobytes() == got["T"].tobytes() and nc["best_h"] == got["best_h"]


def test_ransac_edges_and_refusals(ctx):
    fail = _ransac(ctx, cc.ransac_case("all_fail"))
    assert fail["status"] == 2 and np.array_equal(fail["T"], np.eye(4)) and fail["best_h"] == -1 and np.all(fail["counts"] == -1)
    thr = _ransac(ctx, cc.ransac_case("threshold"))
    assert thr["inliers"] == 4                                  # the pair exactly on the threshold counts, the one beyond does not
    c = cc.ransac_case("m3")
    empty = ctx.ransac_register(c["src"], c["tgt"], np.zeros((0, 2), np.int32), hypotheses=16, max_dist=0.1, counts=True)
    assert empty["status"] == 2 and np.array_equal(empty["T"], np.eye(4)) and np.all(empty["counts"] == -1) and empty["m"] == 0
    two = ctx.ransac_register(c["src"], c["tgt"], c["corr"][:2], hypotheses=16, max_dist=0.1)
    assert two["status"] == 2 and two["n_passed"] == 0
    for kw, what in ((dict(hypotheses=0), "n_hypotheses"), (dict(hypotheses=(1 << 24) + 1), "n_hypotheses"), (dict(max_dist=0.0), "max_dist"),
                     (dict(max_dist=np.nan), "max_dist"), (dict(edge_ratio=1.5), "edge_ratio")):
        with pytest.raises(abi.Tl3dError, match=what):
            ctx.ransac_register(c["src"], c["tgt"], c["corr"], **dict(dict(hypotheses=16, max_dist=0.1), **kw))
    with pytest.raises(abi.Tl3dError, match="outside their cloud"):
        ctx.ransac_register(c["src"], c["tgt"], np.array([[0, 0], [1, 4], [2, 2]], np.int32), hypotheses=16, max_dist=0.1)
    with pytest.raises(abi.Tl3dError, match="outside their cloud"):
        ctx.ransac_register(c["src"], c["tgt"], np.array([[0, 0], [-1, 1], [2, 2]], np.int32), hypotheses=16, max_dist=0.1)
    bad = c["tgt"].copy()
    bad[3, 2] = np.nan
    with pytest.raises(abi.Tl3dError, match="non-finite"):
        ctx.ransac_register(c["src"], bad, c["corr"], hypotheses=16, max_dist=0.1)


# ---- the recipe ----------------------------------------------------------------------------------------------------------------
def _recipe_reference(ctx, s, voxel, k, radius, normal_k, gate, hypotheses):
    """the reference's FPFH -> match -> RANSAC on what the GPU's subsample and normals (tested in their own files) give"""
    pts, nrm = [], []
    for cloud in (s["src"], s["tgt"]):
        p = cloud[gr.voxel_subsample(cloud, voxel)]
        c = p.astype(np.float64).mean(axis=0)
        pts.append(p)
        nrm.append(ctx.estimate_normals(p, nb_neighbors=normal_k, max_radius=radius, viewpoints=c[None], cell_size=radius / 2))
    return gr.recipe(pts[0], nrm[0], pts[1], nrm[1], k, radius, hypotheses, gate, seed=0), pts


def test_recipe_returns_the_reference_and_icp_finishes_from_it(ctx):
    s = cc.scene()
    kw = dict(voxel=0.03, nb_neighbors=cc.K, feature_radius=cc.RADIUS, normal_neighbors=30, max_dist=cc.MAX_DIST, hypotheses=cc.HYPOTHESES,
              seed=0)
    got = metrics.global_align_clouds(ctx, s["src"], s["tgt"], **kw)
    ref, pts = _recipe_reference(ctx, s, 0.03, cc.K, cc.RADIUS, 30, cc.MAX_DIST, cc.HYPOTHESES)
    assert ref["undecided"] == 0 and ref["fs"]["undecided"] == 0 and ref["ft"]["undecided"] == 0
    print(f"recipe: {got['n_a']} / {got['n_b']} points, mutual pairs {got['n_mutual']}, scored {got['n_passed']}, best_h {got['best_h']} "
          f"(reference {ref['best_h']}), inliers {got['inliers']} of {got['m']}, displacement {cc.displacement(got['T'], s['T'], s['src']):.4f} m")
    assert got["status"] == 1 and got["n_a"] == len(pts[0]) and got["n_b"] == len(pts[1])
    assert got["n_corr"] == len(ref["corr"]) and got["n_mutual"] == ref["n_mutual"] and got["mutual"] == ref["mutual"]
    assert got["best_h"] == ref["best_h"] and got["inliers"] == ref["inliers"] and got["n_passed"] == ref["n_passed"]
    assert np.abs(got["T"] - ref["T"]).max() <= 1e-12
    assert cc.displacement(got["T"], s["T"], s["src"]) <= 0.10

    # the local ICP takes over: as near the planted pose as when it starts AT the planted pose (twice: two runs that stop on eps from
    # different sides may differ by a step)
    tn = ctx.estimate_normals(s["tgt"], nb_neighbors=30, cell_size=0.05)
    res, moved = metrics.align_clouds(ctx, s["src"], s["tgt"], tn, T_init="global", global_kw=kw)
    at, _ = metrics.align_clouds(ctx, s["src"], s["tgt"], tn, T_init=s["T"])
    plain, _ = metrics.align_clouds(ctx, s["src"], s["tgt"], tn)
    d_res, d_at, d_plain = (cc.displacement(r["T"], s["T"], s["src"]) for r in (res, at, plain))
    print(f"ICP from the global start: status {res['status']}, displacement {d_res:.5f} m; from the planted pose {d_at:.5f} m; "
          f"from the identity: status {plain['status']}, displacement {d_plain:.3f} m")
    assert res["status"] == 1 and res["global"]["best_h"] == got["best_h"] and moved.shape == s["src"].shape
    assert d_res <= 2 * d_at
    assert d_plain > 0.10                                       # without the global start the local method does not get there
