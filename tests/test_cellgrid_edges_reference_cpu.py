"""CPU: the cases of tests/cellgrid_edges_common.py are what they say they are, and the references the GPU test
(tests/test_gpu_cellgrid_edges.py) holds the cell index's callers to agree with a second formulation each.

The cases: per axis floor((max - min) / cell) + 1 cells, the intended cell count, and the intended number of points in the first
and in the last cell.  The references: the k-d tree means (sor_common.ref_means) against a partition-based brute force, the
argmin-based nearest point (nearest_reference.nearest_points_ref) against a sort-based one, the region form of the triangle
distance against the long-double minimum form; and the share of (case, k, ratio) triples the mask comparison has to drop.  The thin
grid: its cells, that the walk from the corner needs shells 1 to 7, and that no k the GPU test uses splits a tie."""
import numpy as np
import pytest

import cellgrid_edges_common as cg
import cloud_normals_common as cn
import nearest_common as nc
import nearest_reference as nr
import sor_common as sc

CHUNK = 1024                     # cells per block of the scan (cell_chunks, csrc/tl3d_internal.h)


@pytest.mark.parametrize("name", cg.CASES + (cg.THIN,))
def test_cells_and_occupancy_are_the_intended(name):
    p, cell = cg.points(name).astype(np.float64), cg.cell_size(name)
    per_axis = tuple(int(np.floor((p[:, a].max() - p[:, a].min()) / cell)) + 1 for a in range(3))
    assert per_axis == cg.dims(name)
    n, occ = cg.binned(name)
    assert n == per_axis and len(occ) == int(np.prod(per_axis)) and occ.sum() == len(p)
    assert (int(occ[0]), int(occ[-1])) == cg.occupancy(name)
    assert np.all(p * 64 == np.rint(p * 64)) and cell in (1.0, 64.0)         # nothing to round
    assert len(np.unique(p, axis=0)) == len(p)


def test_cell_counts_sit_at_the_chunk_edges():
    ncell = {name: int(np.prod(cg.dims(name))) for name in cg.CASES}
    assert [ncell[f"line_{n}"] for n in cg.LINE_NS] == list(cg.LINE_NS) == [1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
    assert all(np.all(cg.binned(f"line_{n}")[1] == 1) for n in cg.LINE_NS)  # one point per cell
    for n in cg.LAST_FULL_NS:
        occ = cg.binned(f"last_full_{n}")[1]
        assert ncell[f"last_full_{n}"] == n and np.all(occ[:-1] == 1) and occ[-1] == 40
    occ = cg.binned("plane")[1]
    assert ncell["plane"] == 1056 and CHUNK < 1056 < 2 * CHUNK and np.all(occ[:-cg.PLANE_NX] == 1) and np.all(occ[-cg.PLANE_NX:] == 2)
    assert (CHUNK - 1) // cg.PLANE_NX == 31                                 # the chunk edge lies inside the doubled last row of cells
    assert ncell["box"] == 1 and len(cg.points("box")) == 30


def _partition_means(p32, k):
    """the k smallest squared distances by np.partition (no sort, no tree), their roots, averaged"""
    p = np.asarray(p32, dtype=np.float64)
    k = min(k, len(p))
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.sqrt(np.partition(d2, k - 1, axis=1)[:, :k]).sum(axis=1) / k


@pytest.mark.parametrize("name", cg.CASES)
def test_mean_references_agree(name):
    for k in cg.KS:
        tree, part = cg.ref_means(name, k), _partition_means(cg.points(name), k)
        zero = tree == 0
        assert np.array_equal(part == 0, zero)
        err = np.abs(part - tree)[~zero] / tree[~zero]
        print(f"{name} k={k}: n={len(tree)} zero means {int(zero.sum())}, max rel diff {err.max() if err.size else 0.0:.3g}")
        assert np.all(err <= 1e-12)
        if k == 1:
            assert zero.all()                                               # the point itself


def test_mask_triples_stay_within_the_cap():
    every = len(cg.CASES) * len(cg.KS) * len(sc.RATIOS)
    kept = cg.mask_triples()                                                # asserts the cap itself
    dropped = every - len(kept)
    print(f"{dropped} of {every} triples dropped")
    assert dropped <= cg.MAX_DROPPED * every
    # the dropped ones are the two-point line, whose two means ARE the threshold (sigma = 0), and nothing else
    assert sorted(set((n, k) for n in cg.CASES for k in cg.KS for r in sc.RATIOS) - set((n, k) for n, k, _ in kept)) == [("line_2", 20), ("line_2", 33)]


@pytest.mark.parametrize("name", cg.CASES)
def test_point_reference_agrees_with_a_sort(name):
    q, t = cg.queries(name), cg.points(name)
    assert len(q) == len(t) + 4
    d, i = cg.point_ref(name)
    m = nr.point_d2_matrix(q, t)
    assert np.all(m * 2.0 ** 12 == np.rint(m * 2.0 ** 12))                  # every product exact: ties are exact ties
    order = np.argsort(m, axis=1, kind="stable")                            # stable: the smallest index among equal distances
    assert np.array_equal(i, order[:, 0]) and np.array_equal(d, np.sqrt(m[np.arange(len(q)), order[:, 0]]))
    lo, hi = t.min(axis=0), t.max(axis=0)
    assert np.sum(np.any((q[-4:] < lo) | (q[-4:] > hi), axis=1)) == 4       # the four outside points are outside


def test_plane_triangle_reference_agrees_with_the_second_formulation():
    q, v, t = cg.queries("plane"), cg.points("plane"), cg.plane_triangles()
    assert len(t) == 2 * (cg.PLANE_NX - 1) * (cg.PLANE_NY - 1) and t.max() < cg.PLANE_NX * cg.PLANE_NY
    a, b = nr.tri_dist_matrix(q, v, t), nr.tri_dist_second(q, v, t)
    e = float(np.max(np.abs(a.astype(np.longdouble) - b))) / cg.plane_tri_diag()
    print(f"plane: {a.shape[0]} queries x {a.shape[1]} triangles, disagreement {e:.3g} of the diagonal")
    assert e <= nc.EPS_TRI
    d, i, m = cg.plane_tri_ref()
    above = m - d[:, None]
    lo, hi = nc.TRI_TOL_FACTOR * nc.EPS_TRI * cg.plane_tri_diag(), nc.TRI_GAP_FACTOR * nc.EPS_TRI * cg.plane_tri_diag()
    assert not np.any((above > lo) & (above <= hi))                         # the gap nearest_common.tri_gap_ok asks of its cases
    assert np.array_equal(i, np.array([np.flatnonzero(row == row.min())[0] for row in m]))


# ---- the thin grid -----------------------------------------------------------------------------------------------------------------
def _thin_cells(p):
    return np.floor(np.asarray(p, np.float64)).astype(np.int64)             # cell 1, origin 0: the cell of a point is its floor


def test_thin_grid_is_a_corner_cluster_and_two_far_cells():
    p = cg.points(cg.THIN)
    assert len(p) <= 64 and cg.dims(cg.THIN) == (1, 2, 8) and np.all(p.min(axis=0) == 0)
    n, occ = cg.binned(cg.THIN)
    assert n == (1, 2, 8) and list(occ) == [4, 0] + [0] * 12 + [22, 22]     # cell order: x, then y, then z
    c = _thin_cells(p)
    assert np.all(c[:4] == 0) and np.all(c[4:, 2] == 7) and np.all(c[:, 0] == 0)
    # a walk from the corner: shells 1 to 6 hold nothing (in z: empty cells; in y: (0, 1, 0) is empty too), shell 7 the rest
    cheb = np.abs(c - c[0]).max(axis=1)
    assert sorted(set(cheb)) == [0, 7]
    assert all(k > 4 for k in cg.THIN_KS + (cg.THIN_K_NORMALS,))            # every k the GPU test uses has to reach shell 7


def test_thin_grid_references_are_unambiguous():
    """no k in use has its k-th and (k+1)-th neighbour at the same d^2: the k-d tree's means and the brute-force members are the
    only answer, whatever the tie rule; d^2 is exact (multiples of 2^-12)"""
    p = cg.points(cg.THIN)
    idx, d2 = cn.brute_neighbours(p, kmax=max(cg.THIN_KS) + 1)
    assert np.all(d2 * 4096 == np.rint(d2 * 4096))
    for k in cg.THIN_KS + (cg.THIN_K_NORMALS,):
        assert np.all(d2[:, k - 1] < d2[:, k]), k
    r = cn.brute(p, cg.THIN_K_NORMALS)
    assert not r.degenerate.any() and not cn.excluded(r).any()
    ref = cn.ref(p, cg.THIN_K_NORMALS)                                      # the k-d tree formulation agrees on the members' spectrum
    assert np.allclose(ref.lam, r.lam, rtol=1e-9, atol=1e-12)


def test_thin_grid_queries_and_their_reference():
    q, t = cg.thin_queries(), cg.points(cg.THIN)
    lo, hi = t.min(axis=0), t.max(axis=0)
    inside = np.all((q >= lo) & (q <= hi), axis=1)
    assert list(inside) == [True] * (len(q) - 1) + [False] and q[-1, 0] > hi[0] + 1 and np.all((q[-1, 1:] >= lo[1:]) & (q[-1, 1:] <= hi[1:]))
    d, i = cg.point_ref(cg.THIN)
    m = nr.point_d2_matrix(q, t)
    assert np.all(m * 2.0 ** 12 == np.rint(m * 2.0 ** 12))                  # every product exact: ties are exact ties
    order = np.argsort(m, axis=1, kind="stable")
    assert np.array_equal(i, order[:, 0]) and np.array_equal(d, np.sqrt(m[np.arange(len(q)), order[:, 0]]))
    far = _thin_cells(t[i])[:, 2] == 7                                      # the two middle queries: three shells back, three shells on
    assert [bool(f) for f in far] == [False, False, False, True, True, False]
