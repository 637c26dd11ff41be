"""GPU: the callers of the uniform cell index (csrc/cellgrid.h, kernels_cellgrid.hip) on clouds that sit at the edges of its count /
scan / fill (tests/cellgrid_edges_common.py; the cases and the references are held to a restatement and to second formulations in
tests/test_cellgrid_edges_reference_cpu.py).  Public API only.

Two edges carry the outlier filter: the end of the last cell comes from start[ncell], the entry behind the last chunk's scan, and
the cell counts must be zero on entry in a scratch buffer that an earlier, larger call of another kind has left dirty -- the
filter, the searches, cloud normals and plane segmentation build their index by one routine (cell_index_build) and take turns on
one context.  A third carries the shell walk they share (cell_shell_walk): the thin grid of cellgrid_edges_common.py, whose rows are
one cell long and whose neighbours are seven shells off.

The rules are those of the callers' own tests.  Means: test_gpu_sor.py's, 1e-12 relative and exactly 0 where the reference is 0
(derived in that file's docstring).  Mask: the reference's, wherever no reference mean lies within 1e-9 of the threshold (asserted
first; the triples where one does are dropped, at most one in four, and which they are is asserted on the CPU).  Nearest point:
test_gpu_nearest.py's helper; every coordinate here is dyadic, so ties are exact and go to the smaller index.  Nearest triangle:
that file's tolerance, 16 x EPS_TRI x the diagonal, a minimiser, and -- the case being dyadic -- exact zeros and the smallest index.
Normals: cloud_normals_common.check against its brute-force reference, whose neighbours are in (d^2, index) order."""
import numpy as np
import pytest

import cellgrid_edges_common as cg
import cloud_normals_common as cn
import nearest_common as nc
import sor_common as sc
import tl3d
from test_gpu_nearest import _assert_points
from test_gpu_sor import _assert_means

pytestmark = pytest.mark.gpu


def _fresh():
    return tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1)


@pytest.fixture(scope="module")
def ctx():
    with _fresh() as c:
        yield c


@pytest.mark.parametrize("name", cg.CASES)
def test_means_match_the_reference(ctx, name):
    for k in cg.KS:
        got = ctx.knn_mean_distance(cg.points(name), k, cell_size=cg.cell_size(name))
        _assert_means(got, cg.ref_means(name, k), f"{name} k={k}")


@pytest.mark.parametrize("name", cg.CASES)
def test_mask_is_the_references(ctx, name):
    triples = [t for t in cg.mask_triples() if t[0] == name]               # (mask_triples asserts the cap on what it drops)
    assert triples
    for _, k, ratio in triples:
        means = cg.ref_means(name, k)
        thr, ref = sc.ref_mask(means, ratio)
        assert sc.margin_count(means, thr) == 0
        keep = ctx.statistical_outlier(cg.points(name), k, ratio, cell_size=cg.cell_size(name))
        print(f"{name} k={k} ratio={ratio}: kept {int(keep.sum())} of {len(keep)}, reference {int(ref.sum())}, differ {int((keep != ref).sum())}")
        assert keep.dtype == bool and np.array_equal(keep, ref)


@pytest.mark.parametrize("name", cg.CASES)
def test_nearest_points_match_the_reference(ctx, name):
    q, t = cg.queries(name), cg.points(name)
    got = ctx.nearest_points(q, t, cell_size=cg.cell_size(name))
    _assert_points(q, t, got, cg.point_ref(name), True, name)


def _assert_plane_triangles(got, what):
    rd, ri, m = cg.plane_tri_ref()
    d, i = got
    tol = nc.TRI_TOL_FACTOR * nc.EPS_TRI * cg.plane_tri_diag()
    assert d.dtype == np.float64 and i.dtype == np.int32 and d.shape == rd.shape and not np.any(np.isnan(d))
    err = np.abs(d - rd)
    print(f"{what}: {len(rd)} queries x {m.shape[1]} triangles, max err {err.max():.3g} (tolerance {tol:.3g}), triangle differs at {int((i != ri).sum())}")
    assert np.all(err <= tol), f"{what}: {int((err > tol).sum())} distances off"
    assert np.all((i >= 0) & (i < m.shape[1]))
    assert np.all(np.abs(m[np.arange(len(rd)), i] - rd) <= tol), f"{what}: a triangle that is no minimiser"
    assert np.all(d[rd == 0] == 0) and np.array_equal(i, ri), f"{what}: zero distance or tie rule"


def test_nearest_triangles_on_the_plane(ctx):
    got = ctx.nearest_triangles(cg.queries("plane"), cg.points("plane"), cg.plane_triangles(), cell_size=cg.cell_size("plane"))
    _assert_plane_triangles(got, "plane")


def _calls():
    """the reuse sequence: a large search that leaves the scratch dirty, then small calls of every kind"""
    dq, dt, dcell = cg.dirty_cloud()
    lf, pl = "last_full_1025", "plane"
    up = np.tile(np.float32([0, 0, 1]), (len(cg.points(pl)), 1))

    def planes(c):
        ids, recs, counts = c.segment_planes(cg.points(pl), up, radius=1.5, max_offset=0.5, min_points=3, cell_size=cg.cell_size(pl))
        return ids, np.frombuffer(recs.tobytes(), np.uint8), np.int64([counts[k] for k in ("eligible", "regions", "candidates", "planes")])
    return [
        ("dirty nearest_points", lambda c: c.nearest_points(dq, dt, cell_size=dcell)),
        ("last_full knn", lambda c: (c.knn_mean_distance(cg.points(lf), 20, cell_size=cg.cell_size(lf)),)),
        ("line_1025 normals", lambda c: c.estimate_normals(cg.points("line_1025"), 20, cell_size=1.0, curvature=True)),
        ("plane nearest_triangles", lambda c: c.nearest_triangles(cg.queries(pl), cg.points(pl), cg.plane_triangles(), cell_size=cg.cell_size(pl))),
        ("line_1025 outlier", lambda c: (c.statistical_outlier(cg.points("line_1025"), 20, 2.0, cell_size=1.0),)),
        ("plane planes", planes),
        ("last_full knn again", lambda c: (c.knn_mean_distance(cg.points(lf), 20, cell_size=cg.cell_size(lf)),)),
        # twice the cells of the call before it: its counts lie over the (non-zero) start table that call left behind
        ("line_2049 knn", lambda c: (c.knn_mean_distance(cg.points("line_2049"), 20, cell_size=1.0),)),
    ]


def test_a_dirty_scratch_does_not_show():
    """every call of the sequence on ONE context gives, bit for bit, what the same call gives on a fresh context"""
    with _fresh() as one:
        shared = {what: call(one) for what, call in _calls()}
    for what, call in _calls():
        with _fresh() as c:
            alone = call(c)
        assert len(shared[what]) == len(alone)
        for a, b in zip(shared[what], alone):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what
    _assert_means(shared["last_full knn"][0], cg.ref_means("last_full_1025", 20), "last_full_1025 behind the dirty call")
    _assert_plane_triangles(shared["plane nearest_triangles"], "plane behind the normals")
    ids, _, counts = shared["plane planes"]
    assert np.all(ids == 0) and list(counts) == [len(ids), 1, 1, 1]                    # the lattice is one region, and it is a plane
    assert np.array_equal(shared["last_full knn again"][0], shared["last_full knn"][0])
    _assert_means(shared["line_2049 knn"][0], cg.ref_means("line_2049", 20), "line_2049 over the last call's tables")


# ---- the thin grid: 1 x 2 x 8 cells ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", cg.THIN_KS)
def test_thin_grid_means_match_the_reference(ctx, k):
    got = ctx.knn_mean_distance(cg.points(cg.THIN), k, cell_size=cg.cell_size(cg.THIN))
    _assert_means(got, cg.ref_means(cg.THIN, k), f"thin k={k}")


def test_thin_grid_normals_match_the_reference(ctx):
    p, k = cg.points(cg.THIN), cg.THIN_K_NORMALS
    r = cn.brute(p, k)
    assert not r.degenerate.any() and not cn.excluded(r).any()             # on the reference first
    n, c = ctx.estimate_normals(p, k, cell_size=cg.cell_size(cg.THIN), curvature=True)
    assert ctx.last_normals_degenerate == 0
    cn.check(n, c, r, False, f"thin k={k}")


def test_thin_grid_nearest_points_match_the_reference(ctx):
    q, t = cg.thin_queries(), cg.points(cg.THIN)
    got = ctx.nearest_points(q, t, cell_size=cg.cell_size(cg.THIN))
    _assert_points(q, t, got, cg.point_ref(cg.THIN), True, "thin")


@pytest.mark.parametrize("name", cg.NEAREST_ORDER_CASES)
def test_query_order_does_not_show(ctx, name):
    q, t, cell = cg.queries(name), cg.points(name), cg.cell_size(name)

    def run():
        out = list(ctx.nearest_points(q, t, cell_size=cell))
        if name == "plane":
            out += list(ctx.nearest_triangles(q, t, cg.plane_triangles(), cell_size=cell))
        return out
    try:
        ctx.set_nearest_query_order(False)
        in_order = run()
    finally:
        ctx.set_nearest_query_order(True)
    by_cell = run()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(in_order, by_cell))
