"""GPU: the outlier filter's k-NN (kernels_sor.hip) against fp64 references at its edges (tests/sor_common.py; the references are
held to a second formulation and to the oracle in tests/test_sor_reference_cpu.py).

Means: tl3d_knn_mean_distance, the stage tl3d_statistical_outlier thresholds, to 1e-12 relative and exactly 0 where the reference
is 0.  The bound is derived, not measured: both sides work in fp64 from the same float32 points, whose differences are exact in
fp64; the sum of the three squares may be rounded differently (fused or not: at most 2 ulp), a square root is correctly rounded,
and a mean sums at most 64 of them in another order: some tens of ulp of 1.1e-16.  A missed or doubled neighbour moves a mean
by (d_{k+1} - d_k) / k, many orders above that.
Mask: identical to the reference's, because no reference mean lies within 1e-9 of its threshold (asserted first)."""
import ctypes as C

import numpy as np
import pytest

import sor_common as sc
import tl3d
from tl3d import _cabi as abi

pytestmark = pytest.mark.gpu

RTOL = 1e-12
CASE_K_RATIO = [(name, k, r) for name, k in sc.CASE_K for r in sc.RATIOS]


@pytest.fixture
def ctx():
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as c:
        yield c


def _assert_means(got, ref, what):
    zero = ref == 0
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert np.all(got[zero] == 0), f"{what}: a mean that must be exactly 0 is not"
    assert np.all(got[~zero] > 0), f"{what}: a zero mean where the reference has none"
    err = np.abs(got - ref)[~zero] / ref[~zero]
    print(f"{what}: n={len(ref)} zero means {int(zero.sum())}, max rel err {err.max() if err.size else 0.0:.3g}")
    assert np.all(err <= RTOL), f"{what}: {int((err > RTOL).sum())} means off, worst at point {int(np.flatnonzero(~zero)[err.argmax()])}"


@pytest.mark.parametrize("name,k", sc.CASE_K, ids=sc.case_id)
def test_means_match_the_reference(ctx, name, k):
    got = ctx.knn_mean_distance(sc.points(name), k, cell_size=sc.cell_size(name))
    _assert_means(got, sc.case_ref_means(name, k), f"{name} k={k}")


@pytest.mark.parametrize("k", sorted(sc.LATTICE_KNOWN))
def test_lattice_known_answers(ctx, k):
    got = ctx.knn_mean_distance(sc.points("lattice"), k, cell_size=sc.cell_size("lattice"))
    inside = sc.lattice_interior()
    np.testing.assert_allclose(got[inside], sc.LATTICE_KNOWN[k], rtol=1e-14, atol=0)
    assert np.all(got[~inside] > sc.LATTICE_KNOWN[k])


@pytest.mark.parametrize("name,k,ratio", CASE_K_RATIO, ids=sc.case_id)
def test_mask_is_the_references(ctx, name, k, ratio):
    means = sc.case_ref_means(name, k)
    thr, ref = sc.ref_mask(means, ratio)
    if name == "tiny_n2":
        assert means[0] == means[1] == thr and not ref.any()              # both ON the threshold: neither is below it
    else:
        assert sc.margin_count(means, thr) == 0
    if name in ("same", "tiny_n1"):
        assert not ref.any()
    keep = ctx.statistical_outlier(sc.points(name), k, ratio, cell_size=sc.cell_size(name))
    print(f"{name} k={k} ratio={ratio}: kept {int(keep.sum())} of {len(keep)}, reference {int(ref.sum())}, differ {int((keep != ref).sum())}")
    assert keep.dtype == bool and np.array_equal(keep, ref)


@pytest.mark.parametrize("k", [20, 33])
def test_means_do_not_depend_on_the_cell(ctx, k):
    """the k smallest distances are a property of the points, not of the grid that finds them: same multiset, same ordered sum"""
    p = sc.points("k_edges")
    got = [ctx.knn_mean_distance(p, k, cell_size=c) for c in (0.005, 0.05, 0.3, 10.0)]
    _assert_means(got[0], sc.ref_means(p, k), f"k_edges k={k} cell 0.005")
    for g in got[1:]:
        assert np.array_equal(g, got[0])


def test_repeatable_bit_for_bit(ctx):
    """the fill pass places points with atomics, so the order inside a cell may differ between runs; the result must not"""
    p, cell = sc.points("ring"), sc.cell_size("ring")
    m1, m2 = ctx.knn_mean_distance(p, 20, cell_size=cell), ctx.knn_mean_distance(p, 20, cell_size=cell)
    k1, k2 = ctx.statistical_outlier(p, 20, 2.0, cell_size=cell), ctx.statistical_outlier(p, 20, 2.0, cell_size=cell)
    assert np.array_equal(m1, m2) and np.array_equal(k1, k2)


# ---- the raw C ABI ---------------------------------------------------------------------------------------------------------------
def _raw_outlier(ctx, xyz, n, k, ratio, cell, keep, kept):
    return ctx._lib.tl3d_statistical_outlier(ctx._h, abi.ptr(xyz), n, k, ratio, cell, abi.ptr(keep), kept)


def _raw_means(ctx, xyz, n, k, cell, mean):
    return ctx._lib.tl3d_knn_mean_distance(ctx._h, abi.ptr(xyz), n, k, cell, abi.ptr(mean))


@pytest.mark.parametrize("name", ["ring", "dups"])
def test_out_kept_counts_the_mask(ctx, name):
    p, cell = sc.points(name), sc.cell_size(name)
    for ratio in sc.RATIOS:
        keep, kept = np.full(len(p), 7, np.uint8), C.c_int64(-1)
        assert _raw_outlier(ctx, p, len(p), 20, ratio, cell, keep, C.byref(kept)) == abi.OK
        ref = sc.ref_mask(sc.case_ref_means(name, 20), ratio)[1]
        assert set(np.unique(keep).tolist()) <= {0, 1} and np.array_equal(keep.astype(bool), ref)
        assert kept.value == int(keep.sum()) == int(ref.sum())


def test_empty_input_and_argument_checks(ctx):
    p = sc.points("tiny_n21")
    keep, mean, kept = np.zeros(len(p), np.uint8), np.zeros(len(p), np.float64), C.c_int64(-1)
    # n == 0 is not an error, with or without a point pointer
    for xyz in (p, None):
        kept.value = -1
        assert _raw_outlier(ctx, xyz, 0, 20, 2.0, 0.1, keep, C.byref(kept)) == abi.OK and kept.value == 0
        assert _raw_means(ctx, xyz, 0, 20, 0.1, mean) == abi.OK
    assert len(ctx.knn_mean_distance(np.zeros((0, 3), np.float32))) == 0
    # the same checks on both entries
    for k, cell in ((0, 0.1), (65, 0.1), (-1, 0.1), (20, 0.0), (20, -0.1)):
        assert _raw_outlier(ctx, p, len(p), k, 2.0, cell, keep, C.byref(kept)) == abi.E_INVALID, (k, cell)
        assert _raw_means(ctx, p, len(p), k, cell, mean) == abi.E_INVALID, (k, cell)
    assert _raw_outlier(ctx, p, len(p), 20, 2.0, 0.1, None, C.byref(kept)) == abi.E_INVALID
    assert _raw_outlier(ctx, p, len(p), 20, 2.0, 0.1, keep, None) == abi.E_INVALID
    assert _raw_means(ctx, p, len(p), 20, 0.1, None) == abi.E_INVALID
    assert _raw_outlier(ctx, None, len(p), 20, 2.0, 0.1, keep, C.byref(kept)) == abi.E_INVALID
    assert _raw_means(ctx, None, len(p), 20, 0.1, mean) == abi.E_INVALID
    assert _raw_means(ctx, p, -1, 20, 0.1, mean) == abi.E_INVALID
    assert not keep.any() and not mean.any()                               # a refused call writes nothing
    # and the bounds themselves are accepted
    assert _raw_means(ctx, p, len(p), 64, 0.1, mean) == abi.OK and _raw_means(ctx, p, len(p), 1, 0.1, mean) == abi.OK


def test_device_pointers_give_the_host_result(ctx):
    import torch
    dev = torch.device("cuda", 0)
    p, cell, k = sc.points("k_edges"), sc.cell_size("k_edges"), 33
    n = len(p)
    host_mean = ctx.knn_mean_distance(p, k, cell_size=cell)
    host_keep = ctx.statistical_outlier(p, k, 0.0, cell_size=cell)
    _assert_means(host_mean, sc.case_ref_means("k_edges", k), "k_edges k=33 host")
    p_dev = torch.from_numpy(np.array(p)).to(dev)
    for xyz_on_dev in (False, True):
        for out_on_dev in (False, True):
            xyz = p_dev if xyz_on_dev else p
            mean = torch.full((n,), -1.0, dtype=torch.float64, device=dev) if out_on_dev else np.full(n, -1.0)
            keep = torch.full((n,), 7, dtype=torch.uint8, device=dev) if out_on_dev else np.full(n, 7, np.uint8)
            kept = C.c_int64(-1)
            assert _raw_means(ctx, xyz, n, k, cell, mean) == abi.OK
            assert _raw_outlier(ctx, xyz, n, k, 0.0, cell, keep, C.byref(kept)) == abi.OK
            got_mean = mean.cpu().numpy() if out_on_dev else mean
            got_keep = keep.cpu().numpy() if out_on_dev else keep
            assert np.array_equal(got_mean, host_mean), (xyz_on_dev, out_on_dev)
            assert np.array_equal(got_keep.astype(bool), host_keep) and kept.value == int(host_keep.sum()), (xyz_on_dev, out_on_dev)
    assert np.array_equal(p_dev.cpu().numpy(), p)                          # the input is read, never written
