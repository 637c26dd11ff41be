"""GPU: Taubin smoothing and vertex normals of a mesh (tl3d_mesh_smooth_taubin, tl3d_mesh_vertex_normals)
against the Python-integer restatement of the rules (tests/mesh_smooth_reference.py), bit for bit: positions, valences, edge counts
and normals, through host and device pointers, on the smallest shapes at which counting, summing, the row scan, the long rows, the
probing and the wide sums can go wrong; the refusals; the pipeline options on one grid, after the filter and the simplification
and across blocks; the command-line flags."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_components_reference as mcr
import mesh_simplify_reference as msr
import mesh_smooth_reference as ref
import tl3d
from helpers import SMALL, small_scene_frames
from mesh_components_common import SPECK_GRID, SPECK_MIN_TRIANGLES, speck_scene
from mesh_smooth_common import (SHEETS, SMALL_SHAPES, WIDE_FAN_K, extremes, fan, noisy_sphere, reference, renumber, sheet, small_shape, soup,
                                spiky, wide_fan)
from tl3d import _cabi as abi
from tl3d import fileio
from tl3d import pipeline as pl
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bare_ctx():
    """a context without a grid: the calls need none"""
    return tl3d.FusionContext(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], n_slots=1, grid=None)


@pytest.fixture(scope="module")
def ctx():
    with _bare_ctx() as c:
        yield c


def _dev(a):
    import torch
    a = np.array(a)                                                 # (a writable copy: the shared inputs are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _host(t):
    if isinstance(t, np.ndarray):
        return t
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
        bad = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(a)} rows differ, first {bad[0]}: {a[bad[0]]} != {b[bad[0]]}")


def _n_zero(ctx, xyz, tris):
    """the call itself, for its count of zero normals"""
    xyz, tris = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(tris, np.uint32)
    out, nz = np.empty((len(xyz), 3), np.float32), C.c_int64(-1)
    abi.check(ctx._lib.tl3d_mesh_vertex_normals(ctx._h, abi.ptr(xyz) if len(xyz) else None, len(xyz), abi.ptr(tris) if len(tris) else None,
                                                len(tris), abi.ptr(out) if len(xyz) else None, C.byref(nz)))
    return out, nz.value


def _check(ctx, case, device=False, what=""):
    """smoothing of the case's mesh, and the normals of the smoothed mesh, against the shared reference"""
    xyz, tris, want, info, _, _ = case[:6]
    it, lam, mu = case[6:]
    a, t = (_dev(xyz), _dev(tris)) if device else (np.array(xyz), np.array(tris))
    got, ginfo = ctx.smooth_mesh(a, t, it, lam=lam, mu=mu)
    assert ginfo["edges"] == info["edges"] and ginfo["max_valence"] == info["max_valence"], (what, ginfo["edges"], info["edges"])
    assert np.array_equal(_host(ginfo["valence"]), info["valence"]), what + " valence"
    _same_bytes(_host(got), want, what + " positions")
    if device:
        assert got.is_cuda and ginfo["valence"].is_cuda
    return got


_NORMALS = {}


def _want_normals(key, xyz, tris):
    if key not in _NORMALS:
        _NORMALS[key] = ref.normals(xyz, tris)
    return _NORMALS[key]


def _case(name, build, it, lam=0.5, mu=-0.53):
    return reference(name, build, it, lam, mu) + (it, lam, mu)


def _check_normals(ctx, key, xyz, tris, device=False):
    want, wz = _want_normals(key, xyz, tris)
    got = ctx.mesh_normals(_dev(xyz) if device else np.array(xyz), _dev(tris) if device else np.array(tris))
    _same_bytes(_host(got), want, f"{key} normals")
    return want, wz


# ---- crafted shapes -------------------------------------------------------------------------------------------------------------
def test_no_vertex(ctx):
    e, t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)
    out, info = ctx.smooth_mesh(e, t, 3)
    assert out.shape == (0, 3) and info["edges"] == 0 and info["max_valence"] == 0 and len(info["valence"]) == 0
    assert ctx.mesh_normals(e, t).shape == (0, 3) and _n_zero(ctx, e, t)[1] == 0
    # nothing is read: null pointers will do
    ne = C.c_int64(5)
    assert ctx._lib.tl3d_mesh_smooth_taubin(ctx._h, None, 0, None, 0, 3, 0.5, -0.53, None, None, C.byref(ne)) == abi.OK and ne.value == 0
    assert ctx._lib.tl3d_mesh_vertex_normals(ctx._h, None, 0, None, 0, None, C.byref(ne)) == abi.OK and ne.value == 0


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", SMALL_SHAPES)
def test_small_shapes(ctx, name, device):
    case = _case(name, lambda: small_shape(name), 2)
    xyz, tris, want, info = case[:4]
    _check(ctx, case, device, name)
    for key, pos in ((name, xyz), (name + " smoothed", want)):
        nrm, wz = _check_normals(ctx, key, pos, tris, device)
        assert _n_zero(ctx, pos, tris)[1] == wz
    # what the shapes are there for
    nrm, wz = _want_normals(name, xyz, tris)
    if name == "no triangle":
        assert info["edges"] == 0 and not info["valence"].any() and want.tobytes() == xyz.tobytes() and wz == len(xyz) and not nrm.any()
    if name == "isolated vertex":
        assert info["valence"].tolist() == [2, 2, 2, 0, 0] and want[3:].tobytes() == xyz[3:].tobytes() and wz == 2
    if name == "two triangles on one edge":
        assert info["edges"] == 5 and info["valence"].tolist() == [2, 3, 3, 2]
    if name == "tetrahedron":
        assert info["edges"] == 6 and info["valence"].tolist() == [3, 3, 3, 3]
    if name == "bow-tie":
        assert info["edges"] == 6 and info["valence"].tolist() == [2, 2, 4, 2, 2]
    if name == "twice and reversed":
        assert wz == 0 and nrm.tobytes() == ref.normals(xyz, tris[:1])[0].tobytes() and info["edges"] == 3
    if name == "pair that cancels":
        assert wz == 3 and not nrm.any()
    if name == "(a, a, b)":
        assert info["valence"].tolist() == [1, 2, 1] and wz == 3


def test_iterations_zero_copies_and_still_counts(ctx):
    xyz, tris, _ = noisy_sphere()
    for a, t in ((xyz, tris), (_dev(xyz), _dev(tris))):
        out, info = ctx.smooth_mesh(a, t, 0)
        _same_bytes(_host(out), xyz, "copy")
        assert info["edges"] == 1920 and info["max_valence"] == 6 and np.bincount(_host(info["valence"])).tolist() == [0] * 5 + [12, 630]


@pytest.mark.parametrize("it,mu", [(1, -0.53), (10, -0.53), (1, 0.0), (10, 0.0)])
def test_sphere(ctx, it, mu):
    case = _case("sphere", lambda: noisy_sphere()[:2], it, 0.5, mu)
    _check(ctx, case, False, "sphere")
    _check(ctx, case, True, "sphere on the device")
    _check_normals(ctx, f"sphere {it} {mu}", case[2], case[1], device=(it == 10))


def test_fan_of_valence_4096(ctx):
    """the hub's row is summed by a whole wave; nothing is sized by the valence"""
    case = _case("fan", fan, 2)
    assert case[3]["max_valence"] == 4096 and case[3]["edges"] == 2 * 4096
    _check(ctx, case, False, "fan")
    _check(ctx, case, True, "fan on the device")
    _, wz = _check_normals(ctx, "fan smoothed", case[2], case[1])
    assert wz == 0


@pytest.mark.parametrize("nv,nt", SHEETS)
def test_sheets_around_the_chunk(ctx, nv, nt):
    case = _case(f"sheet {nv} {nt}", lambda: sheet(nv, nt), 2)
    assert len(case[0]) == nv and len(case[1]) == nt
    _check(ctx, case, False, f"sheet {nv}")
    _check_normals(ctx, f"sheet {nv} {nt}", case[2], case[1])
    _check(ctx, case, True, f"sheet {nv} on the device")


def test_soup_twice_and_renumbered(ctx):
    case = _case("soup", soup, 2)
    xyz, tris, want, info = case[:4]
    print(f"soup: {info['edges']} edges, largest valence {info['max_valence']}")
    first = _host(_check(ctx, case, True, "soup"))
    second = _host(_check(ctx, case, True, "soup again"))
    assert first.tobytes() == second.tobytes()
    n1 = _host(ctx.mesh_normals(_dev(want), _dev(tris)))
    n2 = _host(ctx.mesh_normals(_dev(want), _dev(tris)))
    wn, wz = _want_normals("soup smoothed", want, tris)
    _same_bytes(n1, wn, "soup normals")
    assert n1.tobytes() == n2.tobytes() and _n_zero(ctx, want, tris)[1] == wz
    # another numbering of the same mesh: the same bytes through the permutation
    xyz2, tris2, perm = renumber(xyz, tris, seed=12)
    out2, info2 = ctx.smooth_mesh(xyz2, tris2, 2)
    assert info2["edges"] == info["edges"] and np.array_equal(info2["valence"][perm], info["valence"])
    _same_bytes(out2[perm], want, "renumbered soup")
    _same_bytes(ctx.mesh_normals(out2, tris2)[perm], wn, "renumbered soup normals")


def test_extreme_coordinates(ctx):
    case = _case("extremes", extremes, 3)
    assert np.abs(case[0]).max() == 1048576.0 and np.abs(case[2]).max() == 1048576.0
    _check(ctx, case, False, "extremes")
    _check_normals(ctx, "extremes", case[0], case[1])
    _check_normals(ctx, "extremes smoothed", case[2], case[1], device=True)


def test_sums_wider_than_64_bits(ctx):
    """a hub 2^21 m from its rim: its D_x passes 2^63 and the normal sums 2^64, which only the wide registers hold"""
    case = _case("wide fan", wide_fan, 1)
    xyz, tris, want, info = case[:4]
    hub = int(np.argmax(info["valence"]))
    q = ref.quantise(xyz)
    D = sum(int(v) for v in q[info["valence"] == 3, 0]) - WIDE_FAN_K * int(q[hub, 0])
    N = ref.normal_sums(xyz, tris)
    assert info["max_valence"] == WIDE_FAN_K and D >= 1 << 63 and max(abs(int(v)) for v in N[hub]) >= 1 << 64
    _check(ctx, case, True, "wide fan")
    _check_normals(ctx, "wide fan", xyz, tris, device=True)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    lib = ctx._lib
    xyz0, tris0 = small_shape("two triangles on one edge")
    p = abi.ptr

    def smooth(xyz, tris, it=2, lam=0.5, mu=-0.53, out=None, val=None):
        out = np.full_like(xyz, 7.0) if out is None else out
        ne = C.c_int64(-1)
        rc = lib.tl3d_mesh_smooth_taubin(ctx._h, p(xyz), len(xyz), p(tris), len(tris), it, lam, mu, p(out), p(val) if val is not None else None,
                                         C.byref(ne))
        return rc, lib.tl3d_last_error().decode(), out

    def normals(xyz, tris, out=None):
        out = np.full_like(xyz, 7.0) if out is None else out
        nz = C.c_int64(-1)
        rc = lib.tl3d_mesh_vertex_normals(ctx._h, p(xyz), len(xyz), p(tris), len(tris), p(out), C.byref(nz))
        return rc, lib.tl3d_last_error().decode(), out
    bad_index = tris0.copy()
    bad_index[1, 2] = 4
    huge_index = tris0.copy()
    huge_index[0, 0] = 0xFFFFFFFF
    for call in (smooth, normals):
        for t in (bad_index, huge_index):
            rc, msg, out = call(xyz0.copy(), t)
            assert rc == abi.E_INVALID and "out of range" in msg and (out == 7.0).all(), msg
        for bad in (np.nan, np.inf, -np.inf, 1048577.0, -3.0e6):
            x = xyz0.copy()
            x[3, 1] = bad
            rc, msg, out = call(x, tris0)
            assert rc == abi.E_INVALID and "2^20" in msg and (out == 7.0).all(), (bad, msg)
        x = xyz0.copy()
        rc, msg, _ = call(x, tris0, out=x)
        assert rc == abi.E_INVALID and "aliases" in msg and x.tobytes() == xyz0.tobytes()
    # the same refusals for device memory, decided by the validation passes
    import torch
    dx, dt = _dev(xyz0), _dev(bad_index)
    with pytest.raises(abi.Tl3dError) as e:
        ctx.smooth_mesh(dx, dt, 2)
    assert e.value.code == abi.E_INVALID
    with pytest.raises(abi.Tl3dError) as e:
        ctx.mesh_normals(dx, dt)
    assert e.value.code == abi.E_INVALID
    dx[2, 0] = float("nan")
    with pytest.raises(abi.Tl3dError) as e:
        ctx.smooth_mesh(dx, _dev(tris0), 2)
    assert e.value.code == abi.E_INVALID
    for kw, word in ((dict(it=-1), "iterations"), (dict(it=1001), "iterations"), (dict(lam=0.0), "lambda"), (dict(lam=1.5), "lambda"),
                     (dict(lam=float("nan")), "lambda"), (dict(mu=0.5), "mu"), (dict(mu=-2.5), "mu"), (dict(mu=float("nan")), "mu")):
        rc, msg, out = smooth(xyz0.copy(), tris0, **kw)
        assert rc == abi.E_INVALID and word in msg and (out == 7.0).all(), (kw, msg)
    out = np.full_like(xyz0, 7.0)
    rc, msg, _ = smooth(xyz0.copy(), tris0, out=out, val=out.view(np.uint32).reshape(-1)[:4])          # the valences inside the positions
    assert rc == abi.E_INVALID and "aliases" in msg and (out == 7.0).all()
    # the limits themselves are accepted, and the context still works after every refusal
    rc, msg, out = smooth(xyz0.copy(), tris0, it=1, lam=1.0, mu=-2.0)
    assert rc == abi.OK, msg
    _same_bytes(out, ref.smooth(xyz0, tris0, 1, 1.0, -2.0)[0], "lambda 1, mu -2")
    torch.cuda.synchronize()


def test_divergence_is_reported_and_the_steps_stop_moving(ctx):
    """lambda 1, mu -2 on a 100 km tetrahedron leaves 2^20 m within a dozen iterations: the call runs its 40 iterations, the ones
    after the flag copy their input through (Q never sees the out-of-range values), and the answer is TL3D_E_INVALID"""
    xyz, tris = spiky()
    with pytest.raises(ValueError, match="diverged"):
        ref.smooth(xyz, tris, 40, 1.0, -2.0)
    last = max(i for i in range(40) if _stays(xyz, tris, i))
    assert 2 <= last < 20
    out, ne = np.full_like(xyz, 7.0), C.c_int64(-1)
    rc = ctx._lib.tl3d_mesh_smooth_taubin(ctx._h, abi.ptr(xyz), 4, abi.ptr(tris), 4, 40, 1.0, -2.0, abi.ptr(out), None, C.byref(ne))
    msg = ctx._lib.tl3d_last_error().decode()
    assert rc == abi.E_INVALID and "diverged" in msg and "lambda 1" in msg and "mu -2" in msg, msg
    assert ne.value == 6
    # what is left in the buffer is the first surface that left the range, copied through the remaining steps: finite, one step
    # beyond the last iteration that stayed inside
    assert np.isfinite(out).all() and np.abs(out).max() > 1048576.0
    edges, val = ref.unique_edges(tris, 4)
    inside = ref.smooth(xyz, tris, last, 1.0, -2.0)[0]
    one = ref.step(inside, edges, val, 1.0)
    two = ref.step(one, edges, val, -2.0)
    first_out = one if np.abs(one).max() > 1048576.0 else two
    _same_bytes(out, first_out, "the surface that left the range")
    with pytest.raises(abi.Tl3dError) as e:
        ctx.smooth_mesh(_dev(xyz), _dev(tris), 40, lam=1.0, mu=-2.0)
    assert e.value.code == abi.E_INVALID
    # one iteration fewer than it takes is fine, and the context works on
    got, _ = ctx.smooth_mesh(xyz, tris, last, lam=1.0, mu=-2.0)
    _same_bytes(got, inside, "the last iteration inside the range")


def _stays(xyz, tris, iterations):
    try:
        ref.smooth(xyz, tris, iterations, 1.0, -2.0)
        return True
    except ValueError:
        return False


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------
def _speck_pipeline(**kw):
    """The pipeline on the speck scene of the component tests (SMALL's camera): the SMALL scene of helpers.py has no floating
    fragment, so the component filter of the chain below would drop nothing on it; the blocked test further down runs on the
    SMALL scene itself."""
    poses, frames, _ = speck_scene()
    dims, voxel, centre = SPECK_GRID["dims"], SPECK_GRID["voxel"], SPECK_GRID["centre"]
    grid = tl3d.GridSpec(dims, tuple(centre[i] - 0.5 * dims[i] * voxel for i in range(3)), voxel, 4 * voxel)
    cam = {k: SMALL[k] for k in ("fx", "fy", "cx", "cy")}
    pipe = DepthToReconstructionPipeline(ReconstructionConfig(**cam, voxel_size=voxel, subsample_factor=1, **kw))
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    out = pipe.reconstruct(grid=grid, poses=poses)
    return pipe, out


def _read_ply_mesh_with_normals(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    assert [l.split()[-1] for l in head if l.startswith("property") and "list" not in l] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    nv = int(next(l for l in head if l.startswith("element vertex")).split()[-1])
    nf = int(next(l for l in head if l.startswith("element face")).split()[-1])
    v = np.frombuffer(data, np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]), nv, end)
    f = np.frombuffer(data, np.dtype([("k", "u1"), ("i", "<i4", 3)]), nf, end + 27 * nv)
    assert len(data) == end + 27 * nv + 13 * nf and (f["k"] == 3).all()
    return v["p"].copy(), v["n"].copy(), v["c"].copy(), f["i"].astype(np.uint32)


def _smooth_stats(info, it=3):
    return {"iterations": it, "lambda": 0.5, "mu": -0.53, "edges": info["edges"], "max_valence": info["max_valence"]}


def test_pipeline_options(tmp_path):
    off, cloud_off = _speck_pipeline(extract_mesh=True)
    on, cloud_on = _speck_pipeline(extract_mesh=True, mesh_smooth_iterations=3, mesh_normals=True)
    # the defaults: no trace of the stages, the PLY as it was; the cloud is not touched by them
    assert off.mesh_normals is None and "mesh_smooth" not in off.stats and not {"mesh_smooth_s", "mesh_normals_s"} & set(off.timings)
    assert set(on.stats) - set(off.stats) == {"mesh_smooth"} and set(on.timings) - set(off.timings) == {"mesh_smooth_s", "mesh_normals_s"}
    assert np.array_equal(cloud_off[0], cloud_on[0]) and np.array_equal(cloud_off[1], cloud_on[1])
    xyz, rgb, tris = off.mesh
    off.save_mesh(str(tmp_path / "plain.ply"))
    fileio.write_ply_mesh(str(tmp_path / "plain_want.ply"), xyz, rgb, tris)
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "plain_want.ply").read_bytes()
    # the options: exactly the reference applied to the plain run's mesh; triangles and colours untouched
    want, info = ref.smooth(xyz, tris, 3)
    wn, wz = ref.normals(want, tris)
    print(f"{len(xyz)} vertices, {len(tris)} triangles, {info['edges']} edges, largest valence {info['max_valence']}, {wz} zero normals")
    assert len(tris) > 1000 and want.tobytes() != xyz.tobytes()
    assert isinstance(on.mesh, tuple) and len(on.mesh) == 3
    _same_bytes(on.mesh[0], want, "smoothed positions")
    _same_bytes(on.mesh[1], rgb, "colours")
    _same_bytes(on.mesh[2], tris, "triangles")
    _same_bytes(on.mesh_normals, wn, "normals")
    assert on.stats["mesh_smooth"] == _smooth_stats(info)
    assert on.stats["mesh_vertices"] == len(xyz) and on.stats["mesh_triangles"] == len(tris)
    assert on.timings["mesh_smooth_s"] >= 0 and on.timings["mesh_normals_s"] >= 0
    on.save_mesh(str(tmp_path / "smooth.ply"))
    p, n, c, f = _read_ply_mesh_with_normals(tmp_path / "smooth.ply")
    assert p.tobytes() == want.tobytes() and n.tobytes() == wn.tobytes() and np.array_equal(c, rgb) and np.array_equal(f, tris)
    # normals alone: of the unsmoothed mesh
    only, _ = _speck_pipeline(extract_mesh=True, mesh_normals=True)
    _same_bytes(only.mesh[0], xyz, "positions")
    _same_bytes(only.mesh_normals, ref.normals(xyz, tris)[0], "normals of the plain mesh")
    assert "mesh_smooth" not in only.stats and "mesh_normals_s" in only.timings and "mesh_smooth_s" not in only.timings
    # after the component filter and the simplification: filter, simplify, smooth, normals
    cell = 2 * SPECK_GRID["voxel"]
    chain, _ = _speck_pipeline(extract_mesh=True, mesh_min_component_triangles=SPECK_MIN_TRIANGLES, mesh_simplify_cell=cell,
                               mesh_smooth_iterations=3, mesh_normals=True)
    filtered = mcr.filter_mesh(xyz, rgb, tris, SPECK_MIN_TRIANGLES)
    simple = msr.simplify(*filtered[:3], cell)
    assert 0 < len(simple[2]) < len(filtered[2]) < len(tris)
    want2, info2 = ref.smooth(simple[0], simple[2], 3)
    _same_bytes(chain.mesh[0], want2, "chain positions")
    _same_bytes(chain.mesh[1], simple[1], "chain colours")
    _same_bytes(chain.mesh[2], simple[2], "chain triangles")
    _same_bytes(chain.mesh_normals, ref.normals(want2, simple[2])[0], "chain normals")
    assert chain.stats["mesh_smooth"] == _smooth_stats(info2) and chain.stats["mesh_vertices"] == len(want2)
    # refused before anything is fused
    for kw in (dict(mesh_smooth_iterations=3), dict(mesh_normals=True)):
        with pytest.raises(ValueError, match="extract_mesh"):
            _speck_pipeline(**kw)
    with pytest.raises(ValueError, match="mesh_smooth_lambda"):
        _speck_pipeline(extract_mesh=True, mesh_smooth_iterations=3, mesh_smooth_lambda=0.0)


def _lattice_run(kw, frames, poses, limit):
    old = pl.MAX_BLOCK_VOXELS
    try:
        if limit is not None:
            pl.MAX_BLOCK_VOXELS = limit
        pipe = DepthToReconstructionPipeline(ReconstructionConfig(**kw))
        pipe.set_frames([c for d, c in frames], [d for d, c in frames])
        pipe.reconstruct(poses=poses)
    finally:
        pl.MAX_BLOCK_VOXELS = old
    return pipe


def _sorted_rows(*cols):
    a = np.concatenate([np.asarray(c, np.float64) for c in cols], axis=1)
    return a[np.lexsort(a.T[::-1])]


def test_smoothed_welded_mesh_equals_the_smoothed_single_lattice_mesh():
    """the SMALL scene on one lattice and on the same lattice forced into blocks: the weld numbers vertices and triangles another
    way, and the smoothed positions and the normals are the same all the same -- matched through the order of the UNSMOOTHED rows"""
    poses, frames = small_scene_frames(n=3)
    cam = {k: SMALL[k] for k in ("fx", "fy", "cx", "cy")}
    base = dict(**cam, voxel_size=0.02, subsample_factor=1, grid_dim=128, outlier_filter=False, extract_mesh=True)
    opts = dict(mesh_smooth_iterations=3, mesh_normals=True)
    plain_one = _lattice_run(base, frames, poses, None)
    limit = plain_one.grid.nvox // 3
    plain_many = _lattice_run(base, frames, poses, limit)
    one = _lattice_run(dict(base, **opts), frames, poses, None)
    many = _lattice_run(dict(base, **opts), frames, poses, limit)
    assert plain_one.stats["blocks"] == one.stats["blocks"] == 1 and plain_many.stats["blocks"] >= 2 and many.stats["blocks"] == plain_many.stats["blocks"]
    ra, rb = _sorted_rows(*plain_one.mesh[:2]), _sorted_rows(*plain_many.mesh[:2])
    assert len(ra) > 1000 and np.array_equal(ra, rb)
    assert not np.array_equal(plain_one.mesh[0], plain_many.mesh[0])              # the weld's order is another one
    for p, q in ((plain_one, one), (plain_many, many)):                          # smoothing renumbers nothing
        assert np.array_equal(p.mesh[1], q.mesh[1]) and np.array_equal(p.mesh[2], q.mesh[2])
    want, info = ref.smooth(plain_one.mesh[0], plain_one.mesh[2], 3)
    _same_bytes(one.mesh[0], want, "single lattice")
    # Every vertex as (unsmoothed position, colour | smoothed position | normal), sorted: the unsmoothed row leads the order, so
    # the two meshes are matched through it; where a few vertices share a row (a zero of the TSDF on a voxel corner gives the
    # same point on several edges) the smoothed values behind it order them, which asks the same of both
    sa = _sorted_rows(*plain_one.mesh[:2], one.mesh[0], one.mesh_normals)
    sb = _sorted_rows(*plain_many.mesh[:2], many.mesh[0], many.mesh_normals)
    assert sa.tobytes() == sb.tobytes(), f"{(sa != sb).any(axis=1).sum()} of {len(sa)} vertices differ between the single and the welded mesh"
    _same_bytes(one.mesh_normals, ref.normals(want, plain_one.mesh[2])[0], "normals")
    assert one.stats["mesh_smooth"] == many.stats["mesh_smooth"] == _smooth_stats(info)
    assert "mesh_smooth_s" in many.timings and "mesh_normals_s" in many.timings


def test_cli_flags(tmp_path):
    from PIL import Image
    poses, frames, _ = speck_scene()
    rgb_dir, depth_dir = tmp_path / "rgb", tmp_path / "depth"
    rgb_dir.mkdir(); depth_dir.mkdir()
    for i, (d, c) in enumerate(frames):
        Image.fromarray(c[..., ::-1]).save(rgb_dir / f"frame_{i:04d}.png")
        np.save(depth_dir / f"frame_{i:04d}_depth.npy", d)
    common = ["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--fx", str(SMALL["fx"]), "--fy", str(SMALL["fy"]),
              "--cx", str(SMALL["cx"]), "--cy", str(SMALL["cy"]), "--no-vis", "--voxel-size", "0.025", "--grid", "128"]
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    exe = [sys.executable, os.path.join(ROOT, "depth_to_reconstruction.py"), *common]

    def run(*extra):
        return subprocess.run(exe + list(extra), env=env, capture_output=True, text=True, timeout=300)
    plain, smooth = tmp_path / "plain.ply", tmp_path / "smooth.ply"
    for r in (run("--output", str(tmp_path / "a.ply"), "--mesh-output", str(plain)),
              run("--output", str(tmp_path / "b.ply"), "--mesh-output", str(smooth), "--mesh-smooth", "3", "--mesh-normals")):
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Mesh smooth: 3 iterations" in r.stdout
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes()
    data = plain.read_bytes()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    nv = int(next(l for l in data[:end].decode().splitlines() if l.startswith("element vertex")).split()[-1])
    nf = int(next(l for l in data[:end].decode().splitlines() if l.startswith("element face")).split()[-1])
    v = np.frombuffer(data, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]), nv, end)
    f = np.frombuffer(data, np.dtype([("k", "u1"), ("i", "<i4", 3)]), nf, end + 15 * nv)
    xyz, col, tris = v["p"].copy(), v["c"].copy(), f["i"].astype(np.uint32)
    want, _ = ref.smooth(xyz, tris, 3)
    fileio.write_ply_mesh(str(tmp_path / "want.ply"), want, col, tris, normals=ref.normals(want, tris)[0])
    assert smooth.read_bytes() == (tmp_path / "want.ply").read_bytes()
    r = run("--output", str(tmp_path / "d.ply"), "--mesh-smooth", "3")
    assert r.returncode == 2 and "--mesh-output" in r.stderr
