"""CPU: the references the outlier filter's GPU tests (tests/test_gpu_sor.py) are held to.  The k-d tree reference against a
brute-force second formulation that shares no code with it, the mask rule against the oracle's, closed-form answers on a lattice,
and the condition that lets the GPU test demand an identical mask: no reference mean sits on its threshold."""
import numpy as np
import pytest

import sor_common as sc
from oracle import ref_numpy as rn

SMALL_CASE_K = [(name, k) for name, k in sc.CASE_K if len(sc.points(name)) <= sc.BRUTE_MAX_N]
CASE_K_RATIO = [(name, k, r) for name, k in sc.CASE_K for r in sc.RATIOS]


def test_the_cases_are_the_ones_the_table_names():
    assert len(sc.points("ring")) == 40400 and len(sc.points("k_edges")) == 3300 and len(sc.points("lattice")) == 960
    assert len(sc.points("dups")) == 3033 and len(sc.points("offset")) == 5200 and len(sc.points("doubling")) == 100000
    assert [len(sc.points(f"tiny_n{n}")) for n in (1, 2, 3, 19, 20, 21)] == [1, 2, 3, 19, 20, 21]
    assert len(np.unique(sc.points("same"), axis=0)) == 1 and len(sc.points("same")) == 30
    assert np.ptp(sc.points("plane")[:, 2]) == 0 and np.ptp(sc.points("line")[:, 1:]) == 0
    assert np.all(sc.points("offset").min(axis=0) > (499, -301, 39)) and all(p.dtype == np.float32 for p in map(sc.points, sc.CASES))
    # every case the brute force skips is named here, so none drops out of the second formulation unnoticed
    assert sorted({name for name, _ in sc.CASE_K} - {name for name, _ in SMALL_CASE_K}) == ["doubling", "ring"]


@pytest.mark.parametrize("name,k", SMALL_CASE_K, ids=sc.case_id)
def test_brute_force_agrees_with_the_tree(name, k):
    tree, brute = sc.case_ref_means(name, k), sc.brute_means(sc.points(name), k)
    zero = tree == 0
    assert np.array_equal(brute == 0, zero)                               # a mean that should be zero is exactly 0 on both sides
    err = np.abs(brute - tree)[~zero] / tree[~zero]
    print(f"{name} k={k}: n={len(tree)} zero means {int(zero.sum())}, max rel diff {err.max() if err.size else 0.0:.3g}")
    assert np.all(err <= 1e-12)


def test_zero_means_are_where_they_should_be():
    assert np.all(sc.case_ref_means("same", 20) == 0) and np.all(sc.case_ref_means("tiny_n1", 20) == 0)
    m = sc.case_ref_means("dups", 20)
    group25 = np.r_[0, 3000:3024]
    group10 = np.r_[1, 3024:3033]
    assert np.flatnonzero(m == 0).tolist() == group25.tolist()            # 25 copies: the 20 nearest are all at distance 0
    assert np.all(m[group10] > 0) and len(set(m[group10].tolist())) == 1    # 10 copies: ten more neighbours lie further out


@pytest.mark.parametrize("name,k,ratio", CASE_K_RATIO, ids=sc.case_id)
def test_mask_rule_is_the_oracles(name, k, ratio):
    thr, mask = sc.ref_mask(sc.case_ref_means(name, k), ratio)
    assert np.array_equal(mask, rn.statistical_outlier_open3d(sc.points(name), k, ratio))


@pytest.mark.parametrize("k", sorted(sc.LATTICE_KNOWN))
def test_lattice_known_answers(k):
    inside = sc.lattice_interior()
    assert inside.sum() == 10 * 8 * 6
    for means in (sc.case_ref_means("lattice", k), sc.brute_means(sc.points("lattice"), k)):
        np.testing.assert_allclose(means[inside], sc.LATTICE_KNOWN[k], rtol=1e-14, atol=0)
        assert np.all(means[~inside] > sc.LATTICE_KNOWN[k])               # a boundary point reaches further for its k-th neighbour


@pytest.mark.parametrize("name,k,ratio", CASE_K_RATIO, ids=sc.case_id)
def test_no_reference_mean_sits_on_its_threshold(name, k, ratio):
    """A condition on the cases, not a measurement: it is what allows the GPU test to ask for an identical mask."""
    means = sc.case_ref_means(name, k)
    thr, mask = sc.ref_mask(means, ratio)
    print(f"{name} k={k} ratio={ratio}: thr {thr:.6g}, kept {mask.mean():.4f}, zero means {int((means == 0).sum())}")
    if name == "tiny_n2":
        # two points: both means are d / 2, mu is d / 2 exactly, sigma is 0: both sit ON the threshold and neither is below it
        assert means[0] == means[1] == thr and not mask.any()
        return
    assert sc.margin_count(means, thr) == 0
    if name in ("same", "tiny_n1"):
        assert not mask.any()                                             # every mean is 0: nothing is valid, nothing is kept


def test_doubling_case_doubles_its_cell():
    p, cell = sc.points("doubling"), sc.cell_size("doubling")
    final, dims, doublings = sc.final_cell(p, cell)
    assert final != cell and final == cell * 2 ** doublings and doublings == 3
    assert np.prod(dims, dtype=np.float64) <= sc.CELL_CAP                  # the final grid fits under the cap ...
    extent = p.max(axis=0).astype(np.float64) - p.min(axis=0).astype(np.float64)
    assert np.prod(np.floor(extent / (final / 2)) + 1) > sc.CELL_CAP       # ... and the cell before it did not
    assert dims == tuple(int(np.floor(e / final)) + 1 for e in extent)
    # no other case leaves its requested cell
    for name in sc.CASES:
        if name != "doubling":
            assert sc.final_cell(sc.points(name), sc.cell_size(name))[2] == 0, name
