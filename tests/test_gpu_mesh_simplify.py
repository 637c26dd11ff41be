"""GPU: vertex-clustering simplification of a mesh (tl3d_mesh_simplify_clusters) against the numpy
restatement of the rules (tests/mesh_simplify_reference.py), bit for bit: the crafted mesh at six cell sizes, topologies on which
hashed clustering goes wrong, the argument checks, the pipeline option on one grid, after the component filter and across blocks,
and the command-line flag."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_components_reference as mcr
import mesh_simplify_reference as msr
import tl3d
from helpers import SMALL
from mesh_simplify_common import (CRAFTED, CRAFTED_ORIGIN, FIGURES, SPECK_GRID, SPECK_MIN_TRIANGLES, TOPOLOGIES, WRAPPED, crafted_mesh,
                                  reference, speck_scene)
from tl3d import _cabi as abi
from tl3d import fileio, synth
from tl3d import pipeline as pl
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_TRIS = np.zeros((0, 3), np.uint32)


def _bare_ctx():
    """a context without a grid: the call needs none"""
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
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _same_bytes(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _assert_simplified(got, want, what=""):
    for k in ("clusters", "vertices_in", "triangles_in", "degenerate_dropped", "duplicates_dropped"):
        assert got[3][k] == want[3][k], (what, k, got[3][k], want[3][k])
    for a, b, name in zip(got[:3], want[:3], ("xyz", "rgb", "tris")):
        if a is None or b is None:
            assert a is None and b is None, f"{what} {name}"
        else:
            _same_bytes(np.asarray(a), np.asarray(b), f"{what} {name}")
    _same_bytes(np.asarray(got[3]["vert_map"]), want[3]["vert_map"], what + " vert_map")


def _raw(ctx, xyz, rgb, tris, cell, origin=None, vert_map=True):
    """the C call itself on host arrays: (rc, counts, out_xyz, out_rgb, out_tri, vert_map), outputs untrimmed"""
    nv, nt = len(xyz), len(tris)
    oxyz, orgb, otri = np.zeros((nv, 3), np.float32), np.zeros((nv, 3), np.uint8), np.zeros((nt, 3), np.uint32)
    vmap = np.zeros(nv, np.uint32) if vert_map else None
    c4 = [C.c_int64(-1) for _ in range(4)]
    o = None if origin is None else (C.c_double * 3)(*origin)
    rc = ctx._lib.tl3d_mesh_simplify_clusters(ctx._h, abi.ptr(xyz), abi.ptr(rgb), nv, abi.ptr(tris), nt, cell, o, abi.ptr(oxyz),
                                              abi.ptr(orgb) if rgb is not None else None, nv, abi.ptr(otri), nt, abi.ptr(vmap),
                                              *[C.byref(c) for c in c4])
    return rc, [c.value for c in c4], oxyz, orgb, otri, vmap


@pytest.mark.parametrize("cell", sorted(CRAFTED))
def test_crafted_mesh(ctx, cell):
    xyz, rgb, tris = crafted_mesh(0)
    want = msr.simplify(xyz, rgb, tris, cell)
    assert (len(want[0]), len(want[2]), want[3]["duplicates_dropped"]) == CRAFTED[cell]
    got = ctx.simplify_mesh(xyz, rgb, tris, cell)
    _assert_simplified(got, want, "host")
    _assert_simplified(ctx.simplify_mesh(xyz, rgb, tris, cell), got, "second run")
    dx, dr, dt, dinfo = ctx.simplify_mesh(_dev(xyz), _dev(rgb), _dev(tris), cell)
    assert dx.is_cuda and dr.is_cuda and dt.is_cuda and dinfo["vert_map"].is_cuda
    _assert_simplified((_host(dx), _host(dr), _host(dt), dict(dinfo, vert_map=_host(dinfo["vert_map"]))), want, "device")
    # without colours
    nx, nr, nt, ninfo = ctx.simplify_mesh(xyz, None, tris, cell)
    assert nr is None
    _assert_simplified((nx, None, nt, ninfo), (want[0], None, want[2], want[3]), "no colours")
    # vert_map is optional
    rc, counts, oxyz, orgb, otri, _ = _raw(ctx, xyz, rgb, tris, cell, vert_map=False)
    kv, kt = len(want[0]), len(want[2])
    assert rc == abi.OK and counts == [kv, kt, want[3]["degenerate_dropped"], want[3]["duplicates_dropped"]]
    _same_bytes(oxyz[:kv], want[0], "xyz"); _same_bytes(orgb[:kv], want[1], "rgb"); _same_bytes(otri[:kt], want[2], "tris")
    # an origin that is no multiple of the cell; a NULL origin is (0, 0, 0)
    _assert_simplified(ctx.simplify_mesh(xyz, rgb, tris, cell, origin=CRAFTED_ORIGIN), msr.simplify(xyz, rgb, tris, cell, CRAFTED_ORIGIN), "shifted")
    _assert_simplified(ctx.simplify_mesh(xyz, rgb, tris, cell, origin=(0.0, 0.0, 0.0)), want, "origin 0")


@pytest.mark.parametrize("name", TOPOLOGIES)
def test_topologies_where_hashed_clustering_goes_wrong(ctx, name):
    (xyz, rgb, tris, cell, origin), want = reference(name)
    assert (len(want[0]), len(want[2]), want[3]["degenerate_dropped"], want[3]["duplicates_dropped"]) == FIGURES[name]
    got = ctx.simplify_mesh(xyz, rgb, tris, cell, origin)
    _assert_simplified(got, want, name)
    _assert_simplified(ctx.simplify_mesh(xyz, rgb, tris, cell, origin), got, name + ", second run")
    if name == "cell finer than the spacing":                       # the triangle list comes back unchanged
        _same_bytes(got[2], tris, "identity")
        assert np.array_equal(got[3]["vert_map"], np.arange(len(xyz)))


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("name", WRAPPED)
def test_vertex_table_half_full_with_chains_that_wrap(ctx, name, kind):
    """the vertex table at its smallest capacity (1024 slots for 512 vertices), every probe sequence starting in its last 8 slots
    and wrapping round the end of the array: 512 distinct cells, and 256 cells that two or more vertices claim"""
    (xyz, rgb, tris, cell, origin), want = reference(name)
    assert (len(want[0]), len(want[2]), want[3]["degenerate_dropped"], want[3]["duplicates_dropped"]) == FIGURES[name]
    for run in ("first run", "second run"):
        if kind == "host":
            got = ctx.simplify_mesh(xyz, rgb, tris, cell, origin)
        else:
            dx, dr, dt, dinfo = ctx.simplify_mesh(_dev(xyz), _dev(rgb), _dev(tris), cell, origin)
            assert dx.is_cuda and dr.is_cuda and dt.is_cuda and dinfo["vert_map"].is_cuda
            got = (_host(dx), _host(dr), _host(dt), dict(dinfo, vert_map=_host(dinfo["vert_map"])))
        _assert_simplified(got, want, f"{name}, {kind}, {run}")


def test_arguments(ctx):
    xyz, rgb, tris = (np.array(a) for a in crafted_mesh(0))
    nv, nt = len(xyz), len(tris)
    lib = ctx._lib
    oxyz, orgb, otri, vmap = np.zeros((nv, 3), np.float32), np.zeros((nv, 3), np.uint8), np.zeros((nt, 3), np.uint32), np.zeros(nv, np.uint32)
    c4 = [C.c_int64(-1) for _ in range(4)]

    def call(xyz=xyz, rgb=rgb, tri=tris, n_tri=nt, n_vert=nv, cell=0.05, origin=None, oxyz=oxyz, vcap=nv, otri=otri, tcap=nt, vmap=vmap):
        o = None if origin is None else (C.c_double * 3)(*origin)
        return lib.tl3d_mesh_simplify_clusters(ctx._h, abi.ptr(xyz), abi.ptr(rgb), n_vert, abi.ptr(tri), n_tri, cell, o, abi.ptr(oxyz),
                                               abi.ptr(orgb), vcap, abi.ptr(otri), tcap, abi.ptr(vmap), *[C.byref(c) for c in c4])

    def untouched():
        return not oxyz.any() and not orgb.any() and not otri.any() and not vmap.any()
    for cell in (0.0, -0.05, float("nan")):
        assert call(cell=cell) == abi.E_INVALID and b"cell size" in lib.tl3d_last_error()
    assert call(origin=(0.0, float("nan"), 0.0)) == abi.E_INVALID and b"origin" in lib.tl3d_last_error()
    # a NaN vertex that no triangle names; a vertex 2^20 cells from the origin: refused by the validation pass
    lone = np.concatenate([xyz, np.array([(0.1, np.nan, 0.1)], np.float32)])
    rc = call(xyz=lone, rgb=np.zeros((nv + 1, 3), np.uint8), n_vert=nv + 1, oxyz=np.zeros((nv + 1, 3), np.float32), vcap=nv + 1,
              vmap=np.zeros(nv + 1, np.uint32))
    assert rc == abi.E_INVALID
    assert b"not finite" in lib.tl3d_last_error()
    far = xyz.copy()
    far[nv // 3, 2] = np.float32(0.05 * (1 << 20)) * np.float32(1.001)
    assert call(xyz=far) == abi.E_INVALID and b"2^20" in lib.tl3d_last_error()
    far[nv // 3, 2] = -np.float32(0.05 * (1 << 20)) * np.float32(1.001)
    assert call(xyz=far) == abi.E_INVALID
    far[nv // 3, 2] = np.float32(0.05 * ((1 << 20) - 2))            # the last cells in range are fine
    assert call(xyz=far) == abi.OK
    oxyz[:], orgb[:], otri[:], vmap[:] = 0, 0, 0, 0
    # an index equal to n_vert
    bad = tris.copy()
    bad[nt // 2, 1] = nv
    assert call(tri=bad) == abi.E_INVALID and b"out of range" in lib.tl3d_last_error()
    # aliased outputs
    assert call(oxyz=xyz) == abi.E_INVALID and b"aliases" in lib.tl3d_last_error()
    assert call(otri=tris) == abi.E_INVALID and b"aliases" in lib.tl3d_last_error()
    assert call(vmap=tris.reshape(-1)[:nv]) == abi.E_INVALID and b"aliases" in lib.tl3d_last_error()
    assert untouched()
    # the context still works afterwards
    want = msr.simplify(xyz, rgb, tris, 0.05)
    _assert_simplified(ctx.simplify_mesh(xyz, rgb, tris, 0.05), want, "after the refusals")
    # short capacities: the true counts are stored, nothing else is
    kv, kt, nd = CRAFTED[0.05]
    figures = [kv, kt, want[3]["degenerate_dropped"], nd]
    for vcap, tcap in ((kv - 1, nt), (nv, kt - 1), (0, 0)):
        assert call(vcap=vcap, tcap=tcap) == abi.E_CAPACITY
        assert [c.value for c in c4] == figures and untouched()
    assert call(vcap=kv, tcap=kt) == abi.OK and [c.value for c in c4] == figures
    _same_bytes(oxyz[:kv], want[0], "xyz"); _same_bytes(orgb[:kv], want[1], "rgb"); _same_bytes(otri[:kt], want[2], "tris")
    _same_bytes(vmap, want[3]["vert_map"], "vert_map")
    assert not oxyz[kv:].any() and not otri[kt:].any()
    # empty inputs
    assert call(n_tri=0, n_vert=0, vcap=0, tcap=0) == abi.OK and [c.value for c in c4] == [0, 0, 0, 0]
    assert call(n_tri=0) == abi.OK and [c.value for c in c4] == [kv, 0, 0, 0]              # vertices are clustered all the same
    _same_bytes(oxyz[:kv], want[0], "xyz without triangles")
    _assert_simplified(ctx.simplify_mesh(xyz, rgb, NO_TRIS, 0.05), msr.simplify(xyz, rgb, NO_TRIS, 0.05), "no triangles")
    empty = ctx.simplify_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), NO_TRIS, 0.05)
    assert len(empty[0]) == 0 and len(empty[2]) == 0 and empty[3]["clusters"] == 0


# ---- pipeline and command line --------------------------------------------------------------------------------------------------
def _read_ply_mesh(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    nv = int(next(l for l in head if l.startswith("element vertex")).split()[-1])
    nf = int(next(l for l in head if l.startswith("element face")).split()[-1])
    v = np.frombuffer(data, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]), nv, end)
    f = np.frombuffer(data, np.dtype([("n", "u1"), ("i", "<i4", 3)]), nf, end + 15 * nv)
    assert len(data) == end + 15 * nv + 13 * nf and (f["n"] == 3).all()
    return v["p"].copy(), v["c"].copy(), f["i"].astype(np.uint32)


def _speck_pipeline(**kw):
    poses, frames, speck = speck_scene()
    dims, voxel, centre = SPECK_GRID["dims"], SPECK_GRID["voxel"], SPECK_GRID["centre"]
    grid = tl3d.GridSpec(dims, tuple(centre[i] - 0.5 * dims[i] * voxel for i in range(3)), voxel, 4 * voxel)
    cam = {k: SMALL[k] for k in ("fx", "fy", "cx", "cy")}
    cfg = ReconstructionConfig(**cam, voxel_size=voxel, subsample_factor=1, **kw)
    pipe = DepthToReconstructionPipeline(cfg)
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    out = pipe.reconstruct(grid=grid, poses=poses)
    return pipe, out


def _info(want, cell):
    return dict({k: v for k, v in want[3].items() if k != "vert_map"}, cell=cell)


def test_pipeline_option(tmp_path):
    cell = 2 * SPECK_GRID["voxel"]
    off, cloud_off = _speck_pipeline(extract_mesh=True)
    on, cloud_on = _speck_pipeline(extract_mesh=True, mesh_simplify_cell=cell)
    # the defaults: no trace of the stage, and the cloud is not touched by it
    assert ReconstructionConfig().mesh_simplify_cell == 0.0
    assert "mesh_simplify" not in off.stats and "mesh_simplify_s" not in off.timings
    assert set(on.stats) - set(off.stats) == {"mesh_simplify"} and set(on.timings) - set(off.timings) == {"mesh_simplify_s"}
    assert np.array_equal(cloud_off[0], cloud_on[0]) and np.array_equal(cloud_off[1], cloud_on[1])
    xyz, rgb, tris = off.mesh
    assert off.stats["mesh_vertices"] == len(xyz) and off.stats["mesh_triangles"] == len(tris)
    off.save_mesh(str(tmp_path / "plain.ply"))
    fileio.write_ply_mesh(str(tmp_path / "plain_want.ply"), xyz, rgb, tris)
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "plain_want.ply").read_bytes()
    # the option: exactly the reference applied to the plain run's mesh, origin (0, 0, 0)
    want = msr.simplify(xyz, rgb, tris, cell)
    print(f"plain {len(xyz)} vertices / {len(tris)} triangles -> {len(want[0])} / {len(want[2])}")
    assert 0 < len(want[0]) < len(xyz) // 2 and 0 < len(want[2]) < len(tris) // 2
    for a, b, name in zip(on.mesh, want[:3], ("xyz", "rgb", "tris")):
        _same_bytes(a, b, name)
    assert on.stats["mesh_simplify"] == _info(want, cell)
    assert on.stats["mesh_vertices"] == len(want[0]) and on.stats["mesh_triangles"] == len(want[2])
    on.save_mesh(str(tmp_path / "simple.ply"))
    for a, b in zip(_read_ply_mesh(tmp_path / "simple.ply"), on.mesh):
        assert np.array_equal(a, b)
    # with the component filter as well: the filter first (specks are judged at full resolution), then the simplification
    both, _ = _speck_pipeline(extract_mesh=True, mesh_simplify_cell=cell, mesh_min_component_triangles=SPECK_MIN_TRIANGLES)
    filtered = mcr.filter_mesh(xyz, rgb, tris, SPECK_MIN_TRIANGLES)
    assert 0 < len(filtered[2]) < len(tris)
    want2 = msr.simplify(*filtered[:3], cell)
    for a, b, name in zip(both.mesh, want2[:3], ("xyz", "rgb", "tris")):
        _same_bytes(a, b, "filtered " + name)
    assert both.stats["mesh_simplify"] == _info(want2, cell) and both.stats["mesh_components"]["triangles_dropped"] == len(tris) - len(filtered[2])
    assert both.stats["mesh_vertices"] == len(want2[0]) and both.stats["mesh_triangles"] == len(want2[2])
    # the option simplifies a mesh: refused without one, and a size must be a size, before anything is fused
    with pytest.raises(ValueError, match="extract_mesh"):
        _speck_pipeline(mesh_simplify_cell=cell)
    for bad in (-0.05, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="mesh_simplify_cell"):
            _speck_pipeline(extract_mesh=True, mesh_simplify_cell=bad)


def test_cli_flag(tmp_path):
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
    plain, simple = tmp_path / "plain.ply", tmp_path / "simple.ply"
    for r in (run("--output", str(tmp_path / "a.ply"), "--mesh-output", str(plain)),
              run("--output", str(tmp_path / "b.ply"), "--mesh-output", str(simple), "--mesh-simplify-cell", "0.05")):
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Mesh simplify" in r.stdout
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes()
    xyz, col, tris = _read_ply_mesh(plain)
    with _bare_ctx() as ctx:
        api = ctx.simplify_mesh(xyz, col, tris, 0.05, origin=(0.0, 0.0, 0.0))
    _assert_simplified(api, msr.simplify(xyz, col, tris, 0.05), "api")
    assert 0 < len(api[2]) < len(tris)
    fileio.write_ply_mesh(str(tmp_path / "want.ply"), *api[:3])
    assert simple.read_bytes() == (tmp_path / "want.ply").read_bytes()
    r = run("--output", str(tmp_path / "d.ply"), "--mesh-simplify-cell", "0.05")
    assert r.returncode == 2 and "--mesh-output" in r.stderr


# ---- across blocks ------------------------------------------------------------------------------------------------------------
def _corridor_run(kw, frames, poses, limit):
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


def _vertex_rows(xyz, rgb):
    a = np.concatenate([np.asarray(xyz, np.float64), np.asarray(rgb, np.float64)], axis=1)
    return a[np.lexsort(a.T[::-1])]


def _triangle_rows(xyz, tris):
    """every triangle as its three positions, rotated so that the smallest position comes first (a welded mesh lists vertices and
    triangles in another order, so another member of a set of duplicates survives: the same triangle, another rotation), sorted"""
    p = np.asarray(xyz, np.float64)[np.asarray(tris, np.int64)]                    # [T, 3, 3]
    first = np.lexsort((p[:, :, 2], p[:, :, 1], p[:, :, 0]), axis=1)[:, 0]
    rot = (first[:, None] + np.arange(3)[None, :]) % 3
    a = np.take_along_axis(p, rot[:, :, None], axis=1).reshape(len(p), 9)
    return a[np.lexsort(a.T[::-1])]


def test_simplified_welded_mesh_equals_the_simplified_single_lattice_mesh():
    """12 VGA frames down the corridor at 2 cm, one lattice and the same lattice forced into blocks: the clusters (positions,
    colours) and the triangles over them are the same sets, because the cell lattice goes through (0, 0, 0) wherever the blocks
    lie and a cluster's sums do not depend on the order of its members"""
    W, H = 640, 480
    cam = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0)
    poses = synth.dolly_poses(12, (0.0, 0.0, 0.0), (0.0, 0.0, 0.1))
    frames = [synth.render(synth.corridor_scene(), p, W, H, **cam) for p in poses]
    base = dict(**cam, voxel_size=0.02, subsample_factor=2, grid_dim=512, outlier_filter=False, extract_mesh=True)
    cell = 0.05
    plain = _corridor_run(base, frames, poses, None)
    one = _corridor_run(dict(base, mesh_simplify_cell=cell), frames, poses, None)
    many = _corridor_run(dict(base, mesh_simplify_cell=cell), frames, poses, plain.grid.nvox // 3)
    assert plain.stats["blocks"] == 1 and one.stats["blocks"] == 1 and many.stats["blocks"] >= 3
    want = msr.simplify(*plain.mesh, cell)
    for a, b, name in zip(one.mesh, want[:3], ("xyz", "rgb", "tris")):
        _same_bytes(a, b, name)
    (ax, ar, at), (bx, br, bt) = one.mesh, many.mesh
    assert len(ax) == len(bx) and len(at) == len(bt) and 0 < len(at) < len(plain.mesh[2])
    assert np.array_equal(_vertex_rows(ax, ar), _vertex_rows(bx, br))
    assert np.array_equal(_triangle_rows(ax, at), _triangle_rows(bx, bt))
    assert one.stats["mesh_simplify"] == many.stats["mesh_simplify"] == _info(want, cell)
    assert many.stats["mesh_vertices"] == len(bx) and many.stats["mesh_triangles"] == len(bt) and "mesh_simplify_s" in many.timings
