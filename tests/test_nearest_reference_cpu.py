"""CPU: the brute-force references of the nearest-neighbour tests (tests/nearest_reference.py) against independent formulations,
on every case of tests/nearest_common.py, and the properties of the cases the GPU test relies on."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import nearest_common as nc
import nearest_reference as nr


@pytest.mark.parametrize("name", nc.POINT_CASES)
def test_point_reference_is_the_kd_trees(name):
    q, t, _, dyadic = nc.point_case(name)
    d, i = nc.point_ref(name)
    kd, ki = cKDTree(t.astype(np.float64)).query(q.astype(np.float64))
    assert d.shape == kd.shape and np.all(np.abs(d - kd) <= 1e-15 * np.maximum(kd, 1e-300) * 4), name
    # the tree's index is a minimiser of the reference; the reference's is the smallest-index one
    assert np.array_equal(nr.point_dist_to(q, t, ki), d)
    m = nr.point_d2_matrix(q, t)
    assert np.array_equal(i, np.array([np.flatnonzero(row == row.min())[0] for row in m]))
    if dyadic:                                              # every product exact: ties are exact ties
        assert np.all(m * 2.0 ** 40 == np.rint(m * 2.0 ** 40))


def test_lattice_ties_are_2_4_8_way():
    q, t, _, _ = nc.point_case("lattice")
    m = nr.point_d2_matrix(q, t)
    ways = (m == m.min(axis=1, keepdims=True)).sum(axis=1)
    assert set(ways.tolist()) == {2, 4, 8}
    d, i = nc.point_ref("lattice")
    assert np.all(i == np.array([np.flatnonzero(row == row.min()).min() for row in m]))


def test_case_properties():
    q, t, cell, _ = nc.point_case("l_shape")
    d, i = nc.point_ref("l_shape")
    assert i[0] == len(t) - 1 and np.floor(t[-2, 1] / cell) == np.floor(q[0, 1] / cell) != np.floor(t[-1, 1] / cell)
    q, t, cell, _ = nc.point_case("lone_point")
    d, i = nc.point_ref("lone_point")
    assert i[0] == i[1] == len(t) - 1 and (t[-1, 0] - t[:-1, 0].max()) / cell > 45
    q, t, _, _ = nc.point_case("five_copies")
    assert np.all(nc.point_ref("five_copies")[1] == 7)
    q, t, _, _ = nc.point_case("self")
    d, i = nc.point_ref("self")
    assert np.all(d == 0) and np.all(i[100:110] == 5) and np.all(np.delete(i, np.arange(100, 110)) == np.delete(np.arange(300), np.arange(100, 110)))


def test_triangle_formulations_agree_and_eps_tri():
    """EPS_TRI: the largest disagreement of the region form (fp64) and the minimum form (long double), relative to the diagonal"""
    worst = 0.0
    for name in nc.TRI_CASES:
        q, v, t, _, _ = nc.tri_case(name)
        a = nr.tri_dist_matrix(q, v, t)
        b = nr.tri_dist_second(q, v, t)
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b.astype(np.float64))), name
        e = float(np.max(np.abs(a.astype(np.longdouble) - b))) / nc.tri_diag(name)
        print(f"{name}: {a.shape[0]} queries x {a.shape[1]} triangles, disagreement {e:.3g} of the diagonal")
        worst = max(worst, e)
    print(f"eps_tri measured {worst:.3g}, asserted {nc.EPS_TRI:.3g}")
    assert worst <= nc.EPS_TRI


@pytest.mark.parametrize("name", nc.TRI_CASES)
def test_triangle_cases_have_the_gap(name):
    assert nc.tri_gap_ok(name)


def test_triangle_known_answers():
    d, i, _ = nc.tri_ref("regions")
    q = nc.tri_case("regions")[0].astype(np.float64)
    assert np.array_equal(d[:7], np.sqrt([1, 3, 3, 3, 2, 2, 3]))           # above: interior, corners, edges, the hypotenuse
    assert np.all(d[-6:] == 0) and np.array_equal(d[14], 0.0) and np.array_equal(d[0], 1.0)
    d, i, m = nc.tri_ref("degenerate")
    assert np.array_equal(d[:3], [1.0, np.sqrt(2.0), np.sqrt(2.0)]) and d[4] == 1.0 and d[7] == 1.0 and d[8] == 1.0
    assert np.array_equal(m[:, 0], m[:, 3]) and np.array_equal(m[:, 1], m[:, 4])
    d, i, m = nc.tri_ref("cube_ties")
    assert d[0] == 0.5 and (m[0] == 0.5).sum() == 2 and i[0] == np.flatnonzero(m[0] == 0.5).min()
    assert (m[2] == 0.5).sum() == 12 and i[2] == 0                           # the centre: every face, so triangle 0
