"""GPU: nearest neighbours from one set to another (kernels_nearest.hip: tl3d_nearest_points, tl3d_nearest_triangles,
tl3d_distance_summary), tl3d.metrics and the pipeline's compare stage, against the fp64 brute-force references of
tests/nearest_reference.py on the cases of tests/nearest_common.py (the references are held to cKDTree and to a long-double second
formulation in tests/test_nearest_reference_cpu.py).

Points.  Distances to 1e-12 relative and exactly 0 where the reference is 0.  Derived as in test_gpu_sor.py, not measured: both
sides take the differences of the same float32 coordinates in fp64 (exact), the sum of the three squares may be rounded
differently (at most 2 ulp), and the square root is correctly rounded: a few ulp of 1.1e-16.  The index: on the dyadic cases every
product is exact, ties are exact ties and the index is the smallest-index minimiser; on the others it is A minimiser (the reference
distance to target[index] is within the tolerance of the minimum).

Triangles.  Within 16 x eps_tri x the box diagonal of the reference, eps_tri = 2.24e-16 being the measured (and, as 2.5e-16,
asserted) largest disagreement of the reference's two formulations relative to the diagonal; 16 is the margin for another operation
order; nearest_common.tri_gap_ok holds every non-minimiser 1000 x eps_tri x diagonal away, three orders above.  The triangle is a
minimiser to the same tolerance, and on the dyadic cases the smallest-index one."""
import ctypes as C
import math

import numpy as np
import pytest

import nearest_common as nc
import nearest_reference as nr
import tl3d
from tl3d import _cabi as abi
from tl3d import fileio, metrics, synth
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu

RTOL = nc.POINT_RTOL


@pytest.fixture(scope="module")
def ctx():
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as c:
        yield c


def _cell(base, factor):
    return None if factor is None else base * factor


def _assert_points(q, t, got, ref, dyadic, what):
    (d, i), (rd, ri) = got, ref
    assert d.dtype == np.float64 and i.dtype == np.int32 and d.shape == rd.shape == i.shape
    zero = rd == 0
    err = np.abs(d - rd)[~zero] / rd[~zero]
    print(f"{what}: n={len(rd)} zero {int(zero.sum())}, max rel err {err.max() if err.size else 0.0:.3g}, index differs at {int((i != ri).sum())}")
    assert np.all(d[zero] == 0), f"{what}: a distance that must be exactly 0 is not"
    assert np.all(err <= RTOL), f"{what}: {int((err > RTOL).sum())} distances off"
    assert np.all((i >= 0) & (i < len(t)))
    if dyadic:
        assert np.array_equal(i, ri), f"{what}: a tie did not go to the smallest index"
    else:
        at = nr.point_dist_to(q, t, i)
        assert np.all(np.abs(at - rd) <= RTOL * rd), f"{what}: an index that is no minimiser"


# ---- points ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.POINT_CASES)
def test_points_match_the_reference_at_every_cell_size(ctx, name):
    q, t, cell, dyadic = nc.point_case(name)
    first = None
    for f in nc.CELL_FACTORS:
        got = ctx.nearest_points(q, t, cell_size=_cell(cell, f))
        if first is None:
            first = got
            _assert_points(q, t, got, nc.point_ref(name), dyadic, f"{name} cell x{f}")
        else:
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), f"{name}: cell x{f} changes the result"


def test_points_self_and_copies(ctx):
    q, t, cell, _ = nc.point_case("self")
    d, i = ctx.nearest_points(q, t, cell_size=cell)
    assert np.all(d == 0) and np.array_equal(i, nc.point_ref("self")[1]) and np.all(i[100:110] == 5)
    q, t, cell, _ = nc.point_case("five_copies")
    d, i = ctx.nearest_points(q, t, cell_size=cell)
    assert np.all(i == 7) and d[0] == 0 and d[1] == 0.0625 and d[2] == 0.0625


def test_points_empty_sets(ctx):
    q, t, _, _ = nc.point_case("plane")
    d, i = ctx.nearest_points(q, np.zeros((0, 3), np.float32))
    assert np.all(np.isposinf(d)) and np.all(i == -1) and len(d) == len(q)
    d, i = ctx.nearest_points(np.zeros((0, 3), np.float32), t)
    assert len(d) == 0 and len(i) == 0
    # either output may be null
    d = np.full(len(q), -1.0)
    i = np.full(len(q), -7, np.int32)
    assert ctx._lib.tl3d_nearest_points(ctx._h, abi.ptr(q), len(q), abi.ptr(t), len(t), 0.2, 0.0, abi.ptr(d), None) == abi.OK
    assert ctx._lib.tl3d_nearest_points(ctx._h, abi.ptr(q), len(q), abi.ptr(t), len(t), 0.2, 0.0, None, abi.ptr(i)) == abi.OK
    rd, ri = nc.point_ref("plane")
    assert np.all(np.abs(d - rd) <= RTOL * rd) and np.array_equal(d, ctx.nearest_points(q, t)[0]) and np.array_equal(i, ctx.nearest_points(q, t)[1])


def test_points_max_dist_is_inclusive(ctx):
    """dyadic: the target at the origin among far ones, queries at exactly max_dist (kept) and one float32 step beyond (+inf / -1)"""
    md = 0.75
    t = np.array([[0, 0, 0], [8, 8, 8], [0, 8, 0], [-8, 0, 0]], np.float32)
    up = np.nextafter(np.float32(md), np.float32(2))
    q = np.array([[md, 0, 0], [up, 0, 0], [0, -md, 0], [0, 0, -up], [0.25, 0.25, 0.25], [8, 8, 8.5], [4, 4, 4], [0, 0.5, 0.5]], np.float32)
    free = ctx.nearest_points(q, t)
    assert np.array_equal(free[0], nr.nearest_points_ref(q, t)[0]) and free[0][0] == md and free[0][1] == float(up) > md
    for cell in (None, 0.1, 1.0, 100.0):
        d, i = ctx.nearest_points(q, t, max_dist=md, cell_size=cell)
        inside = free[0] <= md
        assert inside.tolist() == [True, False, True, False, True, True, False, True]
        assert np.array_equal(d[inside], free[0][inside]) and np.array_equal(i[inside], free[1][inside])
        assert np.all(np.isposinf(d[~inside])) and np.all(i[~inside] == -1)
    # on a general case: the results within the limit are those of the unlimited call, bit for bit
    q, t, cell, _ = nc.point_case("shell_plane")
    rd = nc.point_ref("shell_plane")[0]
    md = float(np.median(rd))
    assert not np.any(np.abs(rd - md) < 1e-9)
    free = ctx.nearest_points(q, t, cell_size=cell)
    d, i = ctx.nearest_points(q, t, max_dist=md, cell_size=cell)
    inside = free[0] <= md
    assert 0 < inside.sum() < len(q)
    assert np.array_equal(d[inside], free[0][inside]) and np.array_equal(i[inside], free[1][inside])
    assert np.all(np.isposinf(d[~inside])) and np.all(i[~inside] == -1)


def test_points_repeatable_and_query_order(ctx):
    """the fills place points and queries with atomics; neither that nor the order the queries run in may show"""
    q, t, cell, _ = nc.point_case("shell_plane")
    a, b = ctx.nearest_points(q, t, cell_size=cell), ctx.nearest_points(q, t, cell_size=cell)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    try:
        ctx.set_nearest_query_order(False)
        c = ctx.nearest_points(q, t, cell_size=cell)
        qm, vm, tm, cm, _ = nc.tri_case("icosphere")
        tri_in = ctx.nearest_triangles(qm, vm, tm, cell_size=cm)
    finally:
        ctx.set_nearest_query_order(True)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    tri_cell = ctx.nearest_triangles(qm, vm, tm, cell_size=cm)
    assert np.array_equal(tri_in[0], tri_cell[0]) and np.array_equal(tri_in[1], tri_cell[1])


def test_points_device_tensors_give_the_host_bytes(ctx):
    import torch
    dev = torch.device("cuda", 0)
    q, t, cell, _ = nc.point_case("nq257")
    host = ctx.nearest_points(q, t, cell_size=cell)
    qd, td = torch.from_numpy(np.array(q)).to(dev), torch.from_numpy(np.array(t)).to(dev)
    d, i = ctx.nearest_points(qd, td, cell_size=cell)
    assert d.is_cuda and i.is_cuda and d.dtype == torch.float64 and i.dtype == torch.int32
    assert np.array_equal(d.cpu().numpy(), host[0]) and np.array_equal(i.cpu().numpy(), host[1])
    d, i = ctx.nearest_points(qd, t, cell_size=cell)                        # mixed: device queries, host target
    assert np.array_equal(d.cpu().numpy(), host[0]) and np.array_equal(i.cpu().numpy(), host[1])
    assert np.array_equal(qd.cpu().numpy(), q) and np.array_equal(td.cpu().numpy(), t)
    s_host = ctx.distance_summary(host[0], (0.1, 0.2))
    assert ctx.distance_summary(torch.from_numpy(host[0]).to(dev), (0.1, 0.2)) == s_host


def test_points_argument_errors_write_nothing(ctx):
    q, t, cell, _ = nc.point_case("plane")
    nq, nt = len(q), len(t)
    d, i = np.full(nq, -1.0), np.full(nq, -7, np.int32)

    def call(qq, n_q, tt, n_t, dd=d, ii=i, h=None):
        return ctx._lib.tl3d_nearest_points(ctx._h if h is None else h, abi.ptr(qq), n_q, abi.ptr(tt), n_t, cell, 0.0, abi.ptr(dd), abi.ptr(ii))
    assert ctx._lib.tl3d_nearest_points(None, abi.ptr(q), nq, abi.ptr(t), nt, cell, 0.0, abi.ptr(d), abi.ptr(i)) == abi.E_INVALID
    assert call(q, -1, t, nt) == abi.E_INVALID and call(q, nq, t, -1) == abi.E_INVALID
    assert call(q, nq, t, 2 ** 31) == abi.E_INVALID
    assert call(None, nq, t, nt) == abi.E_INVALID and call(q, nq, None, nt) == abi.E_INVALID
    # an output that overlaps an input: the distances over the target, the indices over the queries
    big = np.zeros(max(nq * 8, nt * 12) // 4 + 8, np.float32)
    assert ctx._lib.tl3d_nearest_points(ctx._h, abi.ptr(q), nq, abi.ptr(big), nt, cell, 0.0, abi.ptr(big), abi.ptr(i)) == abi.E_INVALID
    assert ctx._lib.tl3d_nearest_points(ctx._h, abi.ptr(big), nq, abi.ptr(t), nt, cell, 0.0, abi.ptr(d), abi.ptr(big)) == abi.E_INVALID
    for bad in (np.nan, np.inf, -np.inf):
        for which in ("query", "target"):
            qq, tt = np.array(q), np.array(t)
            (qq if which == "query" else tt)[3, 1] = bad
            assert call(qq, nq, tt, nt) == abi.E_INVALID, (bad, which)
            assert b"non-finite" in ctx._lib.tl3d_last_error()
    qq = np.array(q)
    qq[0, 0] = np.nan
    assert call(qq, nq, t, 0) == abi.E_INVALID                               # ... with an empty target too
    assert np.all(d == -1.0) and np.all(i == -7)                            # a refused call writes nothing
    assert call(q, 0, t, nt) == abi.OK and call(None, 0, t, nt) == abi.OK and np.all(d == -1.0)
    assert call(q, nq, t, nt) == abi.OK and np.all(d >= 0)


# ---- triangles ---------------------------------------------------------------------------------------------------------------
def _assert_tris(name, got, what):
    q, v, t, _, dyadic = nc.tri_case(name)
    rd, ri, m = nc.tri_ref(name)
    d, i = got
    tol = nc.tri_tol(name)
    assert d.dtype == np.float64 and i.dtype == np.int32 and d.shape == rd.shape
    assert not np.any(np.isnan(d))
    err = np.abs(d - rd)
    print(f"{what}: {len(rd)} queries x {len(t)} triangles, max err {err.max():.3g} (tolerance {tol:.3g}), triangle differs at {int((i != ri).sum())}")
    assert np.all(err <= tol), f"{what}: {int((err > tol).sum())} distances off"
    assert np.all((i >= 0) & (i < len(t)))
    assert np.all(np.abs(m[np.arange(len(rd)), i] - rd) <= tol), f"{what}: a triangle that is no minimiser"
    if dyadic:
        assert np.all(d[rd == 0] == 0) and np.array_equal(i, ri), f"{what}: zero distance or tie rule"


@pytest.mark.parametrize("name", nc.TRI_CASES)
def test_triangles_match_the_reference_at_every_cell_size(ctx, name):
    assert nc.tri_gap_ok(name)
    q, v, t, cell, _ = nc.tri_case(name)
    first = None
    for f in nc.CELL_FACTORS:
        got = ctx.nearest_triangles(q, v, t, cell_size=_cell(cell, f))
        if first is None:
            first = got
            _assert_tris(name, got, f"{name} cell x{f}")
        else:
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), f"{name}: cell x{f} changes the result"
    again = ctx.nearest_triangles(q, v, t, cell_size=cell)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])


def test_triangles_known_answers(ctx):
    q, v, t, cell, _ = nc.tri_case("regions")
    d, i = ctx.nearest_triangles(q, v, t, cell_size=cell)
    assert np.array_equal(d[:7], np.sqrt([1, 3, 3, 3, 2, 2, 3])) and np.all(d[-6:] == 0) and np.all(i == 0)
    q, v, t, cell, _ = nc.tri_case("degenerate")
    d, i = ctx.nearest_triangles(q, v, t, cell_size=cell)
    assert np.array_equal(d[:3], [1.0, math.sqrt(2.0), math.sqrt(2.0)]) and d[4] == 1.0 and d[7] == 1.0 and d[8] == 1.0
    q, v, t, cell, _ = nc.tri_case("cube_ties")
    d, i = ctx.nearest_triangles(q, v, t, cell_size=cell)
    assert d[0] == 0.5 and i[0] == nc.tri_ref("cube_ties")[1][0] and d[2] == 0.5 and i[2] == 0


def test_triangles_empty_errors_and_max_dist(ctx):
    q, v, t, cell, _ = nc.tri_case("cube")
    d, i = ctx.nearest_triangles(q, v, np.zeros((0, 3), np.uint32))
    assert np.all(np.isposinf(d)) and np.all(i == -1)
    d, i = np.full(len(q), -1.0), np.full(len(q), -7, np.int32)

    def call(qq, vv, tt, n_v=None):
        return ctx._lib.tl3d_nearest_triangles(ctx._h, abi.ptr(qq), len(qq), abi.ptr(vv), len(vv) if n_v is None else n_v, abi.ptr(tt), len(tt),
                                               cell, 0.0, abi.ptr(d), abi.ptr(i))
    bad = np.array(t)
    bad[5, 2] = len(v)
    assert call(q, v, bad) == abi.E_INVALID and b"out of range" in ctx._lib.tl3d_last_error()
    bad[5, 2] = 0xFFFFFFFF
    assert call(q, v, bad) == abi.E_INVALID
    assert call(q, v, t, n_v=len(v) - 1) == abi.E_INVALID
    for arr in ("q", "v"):
        qq, vv = np.array(q), np.array(v)
        (qq if arr == "q" else vv)[2, 0] = np.nan
        assert call(qq, vv, t) == abi.E_INVALID
    assert call(q, v, t, n_v=2 ** 31) == abi.E_INVALID
    assert ctx._lib.tl3d_nearest_triangles(None, abi.ptr(q), len(q), abi.ptr(v), len(v), abi.ptr(t), len(t), cell, 0.0, abi.ptr(d), abi.ptr(i)) == abi.E_INVALID
    assert np.all(d == -1.0) and np.all(i == -7)
    free = ctx.nearest_triangles(q, v, t, cell_size=cell)
    md = 0.3
    assert not np.any(np.abs(free[0] - md) < 1e-9)
    d, i = ctx.nearest_triangles(q, v, t, cell_size=cell, max_dist=md)
    inside = free[0] <= md
    assert 0 < inside.sum() < len(q)
    assert np.array_equal(d[inside], free[0][inside]) and np.array_equal(i[inside], free[1][inside])
    assert np.all(np.isposinf(d[~inside])) and np.all(i[~inside] == -1)


# ---- summary -----------------------------------------------------------------------------------------------------------------
def test_distance_summary(ctx):
    r = np.random.default_rng(2)
    d = np.abs(r.normal(size=300_001)) * 0.01
    d[::1000] = np.inf
    d[5] = 0.0125                                                            # an entry equal to a threshold is below it
    thr = (0.0125, 0.001, 0.05, 0.0)
    s = ctx.distance_summary(d, thr)
    fin = d[np.isfinite(d)]
    assert s["n"] == len(d) and s["within"] == len(fin) and s["max"] == fin.max()
    assert s["below"] == [int((d <= t).sum()) for t in thr] and (d == 0.0125).sum() >= 1
    for got, want in ((s["sum"], math.fsum(fin)), (s["sum_sq"], math.fsum(fin * fin))):
        assert abs(got - want) <= 1e-12 * want
    assert s["mean"] == s["sum"] / s["within"] and s["rms"] == math.sqrt(s["sum_sq"] / s["within"])
    assert ctx.distance_summary(d, thr) == s
    e = ctx.distance_summary(np.zeros(0), ())
    assert e["n"] == 0 and e["within"] == 0 and e["below"] == [] and math.isnan(e["mean"])
    allinf = ctx.distance_summary(np.full(7, np.inf), (1.0,))
    assert allinf["within"] == 0 and allinf["below"] == [0] and allinf["sum"] == 0
    out = abi.DistanceStats()
    nine = np.arange(9, dtype=np.float64)
    assert ctx._lib.tl3d_distance_summary(ctx._h, abi.ptr(d), len(d), abi.ptr(nine), 9, C.byref(out)) == abi.E_INVALID
    assert ctx._lib.tl3d_distance_summary(ctx._h, abi.ptr(d), -1, None, 0, C.byref(out)) == abi.E_INVALID
    assert ctx._lib.tl3d_distance_summary(ctx._h, abi.ptr(d), len(d), None, 0, None) == abi.E_INVALID
    assert ctx._lib.tl3d_distance_summary(ctx._h, abi.ptr(d), len(d), abi.ptr(nine), 8, C.byref(out)) == abi.OK and out.n == len(d)


# ---- metrics, pipeline, command line -------------------------------------------------------------------------------------------
CAM = dict(fx=130.0, fy=130.0, cx=80.0, cy=60.0)
W, H = 160, 120


@pytest.fixture(scope="module")
def sequence():
    scene = synth.plane_sphere_scene()
    poses = synth.dolly_poses(3, (-0.02, 0.0, 0.0), (0.02, 0.0, 0.0))
    r0, t0 = poses[0]
    rel = [(r @ r0.T, t.reshape(3, 1) - (r @ r0.T) @ t0.reshape(3, 1)) for r, t in poses]
    return rel, [synth.render(scene, p, W, H, **CAM) for p in poses]


def _pipe(frames, **kw):
    cfg = ReconstructionConfig(**CAM, voxel_size=0.02, subsample_factor=1, grid_dim=256, **kw)
    pipe = DepthToReconstructionPipeline(cfg)
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    return pipe, cfg


def _clear_of(t, values):
    """the first of t, t + 3e-9, ... that no value lies within 1e-9 of"""
    while np.any(np.abs(values - t) < 1e-9):
        t += 3e-9
    return t


def test_compare_clouds_is_the_kd_trees_chamfer(ctx, sequence):
    from oracle import ref_numpy as rn
    from scipy.spatial import cKDTree
    rel, frames = sequence
    pipe, cfg = _pipe(frames)
    pts, _, _ = pipe.reconstruct(poses=rel)
    clouds = [rn.backproject(d, c, cfg.fx, cfg.fy, cfg.cx, cfg.cy, pose=p, scale=1.0, subsample=cfg.subsample_factor,
                             min_depth=cfg.min_depth, max_depth=cfg.max_depth) for (d, c), p in zip(frames, rel)]
    ref_p, _ = rn.merge_open3d(clouds, cfg.voxel_size, sor=True)
    a, b = np.asarray(pts, np.float32), np.asarray(ref_p, np.float32)
    assert len(a) > 500 and len(b) > 500
    dab = cKDTree(b.astype(np.float64)).query(a.astype(np.float64))[0]
    dba = cKDTree(a.astype(np.float64)).query(b.astype(np.float64))[0]
    both = np.concatenate([dab, dba])
    thr = tuple(_clear_of(float(x), both) for x in (*np.quantile(both, [0.5, 0.9]), 1e-3))
    assert all(not np.any(np.abs(both - t) < 1e-9) for t in thr)
    got = metrics.compare_clouds(ctx, a, b, thresholds=thr)
    want = 0.5 * (dab.mean() + dba.mean())
    print(f"chamfer {got['chamfer_mean']:.6g} (tree {want:.6g}), {len(a)} / {len(b)} points")
    assert abs(got["chamfer_mean"] - want) <= 1e-12 * want
    assert got["a_to_b"]["n"] == got["a_to_b"]["within"] == len(a) and got["b_to_a"]["n"] == len(b)
    for j, t in enumerate(thr):
        p, r = (dab <= t).sum() / len(a), (dba <= t).sum() / len(b)
        assert got["at"][j]["precision"] == p and got["at"][j]["recall"] == r
        assert got["at"][j]["fscore"] == (2 * p * r / (p + r) if p + r > 0 else 0.0)
    assert "chamfer" in metrics.format_line(got)


def test_compare_cloud_to_mesh_on_a_sphere(ctx):
    v, t = nc._icosphere(2)
    r = np.random.default_rng(4)
    p = r.normal(size=(400, 3))
    p = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)
    v32, t32 = v.astype(np.float32), t.astype(np.uint32)
    got = metrics.compare_cloud_to_mesh(ctx, p, v32, t32, thresholds=(0.01, 0.05))
    dps = nr.nearest_triangles_ref(p, v32, t32)[0]
    dvp = nr.nearest_points_ref(v32, p)[0]
    ps, vp = got["points_to_surface"], got["vertices_to_points"]
    assert ps["n"] == 400 and vp["n"] == len(v)
    assert abs(ps["mean"] - dps.mean()) <= 1e-12 and abs(ps["max"] - dps.max()) <= 16 * nc.EPS_TRI * 4 and abs(vp["mean"] - dvp.mean()) <= 1e-12 * dvp.mean()
    assert 0 < dps.max() < 0.03                                              # the chords of a twice-subdivided icosahedron
    assert not np.any(np.abs(dps[:, None] - np.array([0.01, 0.05])) < 1e-9) and not np.any(np.abs(dvp[:, None] - np.array([0.01, 0.05])) < 1e-9)
    assert ps["below"] == [int((dps <= x).sum()) for x in (0.01, 0.05)] and vp["below"] == [int((dvp <= x).sum()) for x in (0.01, 0.05)]
    assert got["at"][1]["recall"] == 1.0


def test_pipeline_compare_to_its_own_output(sequence, tmp_path):
    rel, frames = sequence
    plain, _ = _pipe(frames, extract_mesh=True)
    pts, col, _ = plain.reconstruct(poses=rel)
    ref = tmp_path / "ref.ply"
    fileio.write_ply_binary(ref, pts, col)
    assert np.array_equal(fileio.read_ply_points(ref), pts.astype(np.float32))
    pipe, _ = _pipe(frames, extract_mesh=True, compare_to=str(ref), compare_thresholds=(0.001, 0.01))
    pts2, col2, _ = pipe.reconstruct(poses=rel)
    cmp = pipe.stats["compare"]
    assert cmp["chamfer_mean"] == 0 and cmp["a_to_b"]["max"] == 0 and cmp["b_to_a"]["max"] == 0
    assert all(r["precision"] == 1.0 and r["recall"] == 1.0 and r["fscore"] == 1.0 for r in cmp["at"]) and len(cmp["at"]) == 2
    assert cmp["mesh"]["points_to_surface"]["n"] == len(pts) and cmp["mesh"]["vertices_to_points"]["n"] == len(pipe.mesh[0])
    assert cmp["mesh"]["points_to_surface"]["mean"] < 0.02
    assert pipe.timings["compare_s"] >= 0 and "compare_s" not in plain.timings and "compare" not in plain.stats
    assert np.array_equal(pts2, pts) and np.array_equal(col2, col)
    assert {k: v for k, v in pipe.stats.items() if k != "compare"} == plain.stats
    for m2, m1 in zip(pipe.mesh, plain.mesh):
        assert np.array_equal(m2, m1)


def test_cli_compare_to(sequence, tmp_path, capsys):
    from PIL import Image
    rel, frames = sequence
    rgb_dir, depth_dir = tmp_path / "rgb", tmp_path / "depth"
    rgb_dir.mkdir()
    depth_dir.mkdir()
    for k, (d, c) in enumerate(frames):
        Image.fromarray(c[..., ::-1]).save(rgb_dir / f"frame_{k:04d}.png")
        np.save(depth_dir / f"frame_{k:04d}_depth.npy", d)
    import depth_to_reconstruction as cli
    common = ["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--fx", "130", "--fy", "130", "--cx", "80", "--cy", "60",
              "--voxel-size", "0.02", "--grid", "256", "--no-vis"]
    first = tmp_path / "first.ply"
    assert cli.main(common + ["--output", str(first)]) == 0 and first.exists()
    capsys.readouterr()
    assert cli.main(common + ["--output", str(tmp_path / "second.ply"), "--compare-to", str(first), "--compare-threshold", "0.004",
                              "--compare-threshold", "0.03", "--compare-max-dist", "0.5"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "Compare:" in ln]
    assert len(lines) == 1 and "chamfer 0 m" in lines[0] and "F@0.004 1.0000" in lines[0] and "F@0.03 1.0000" in lines[0]
