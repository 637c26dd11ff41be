"""GPU: quadric placement of the clustered vertices (tl3d_mesh_simplify_quadric) against the restatement
of the rules (tests/mesh_simplify_quadric_reference.py), bit for bit: the crafted mesh at six cell sizes, the meshes with known
answers (a roof's crease, a cube's corner), the carry case of the 128-bit sums, the key table's wrap case and the soup, chunk
edges, the argument checks, the pipeline option on one grid and across blocks, and the command-line flag."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_simplify_quadric_reference as mqr
import mesh_simplify_reference as msr
import tl3d
from helpers import SMALL
from mesh_simplify_common import CRAFTED, CRAFTED_ORIGIN, SPECK_GRID, SPECK_MIN_TRIANGLES, WRAPPED, crafted_mesh, speck_scene
from mesh_simplify_quadric_common import CARRY_FILL, CARRY_TRIS, CORNER, NO_TRIS, ROOFS, reference, roof_crease_clusters, roof_distance
from tl3d import _cabi as abi
from tl3d import synth
from tl3d import pipeline as pl
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ("clusters", "vertices_in", "triangles_in", "degenerate_dropped", "duplicates_dropped")
QUADRIC = ("quadric_placed", "clamped", "corners_skipped")


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


def _assert_quadric(got, want, mean=None, what=""):
    """got against the reference (every array and count); and, given the mean call's result, everything but the positions
    against its bytes"""
    for k in COUNTS + QUADRIC:
        assert got[3][k] == want[3][k], (what, k, got[3][k], want[3][k])
    for a, b, name in zip(got[:3], want[:3], ("xyz", "rgb", "tris")):
        if a is None or b is None:
            assert a is None and b is None, f"{what} {name}"
        else:
            _same_bytes(np.asarray(a), np.asarray(b), f"{what} {name}")
    _same_bytes(np.asarray(got[3]["vert_map"]), want[3]["vert_map"], what + " vert_map")
    if mean is not None:
        for k in COUNTS:
            assert got[3][k] == mean[3][k], (what, "mean", k)
        for a, b, name in zip(got[1:3], mean[1:3], ("rgb", "tris")):
            if a is not None:
                _same_bytes(np.asarray(a), np.asarray(b), f"{what} mean's {name}")
        _same_bytes(np.asarray(got[3]["vert_map"]), np.asarray(mean[3]["vert_map"]), what + " mean's vert_map")


def _quadric(ctx, inp, **kw):
    xyz, rgb, tris, cell, origin = inp
    return ctx.simplify_mesh(xyz, rgb, tris, cell, origin, placement="quadric", **kw)


def _raw(ctx, xyz, rgb, tris, cell, origin=None, reg=mqr.REG, vert_map=True, vcap=None, tcap=None, n_vert=None, n_tri=None, out=None):
    """the C call itself on host arrays: (rc, the seven counts, out_xyz, out_rgb, out_tri, vert_map), outputs untrimmed"""
    nv, nt = len(xyz) if n_vert is None else n_vert, len(tris) if n_tri is None else n_tri
    oxyz, orgb, otri, vmap = out or (np.zeros((len(xyz), 3), np.float32), np.zeros((len(xyz), 3), np.uint8), np.zeros((len(tris), 3), np.uint32),
                                     np.zeros(len(xyz), np.uint32) if vert_map else None)
    c7 = [C.c_int64(-1) for _ in range(7)]
    o = None if origin is None else (C.c_double * 3)(*origin)
    rc = ctx._lib.tl3d_mesh_simplify_quadric(ctx._h, abi.ptr(xyz), abi.ptr(rgb), nv, abi.ptr(tris), nt, cell, o, reg, abi.ptr(oxyz),
                                             abi.ptr(orgb) if rgb is not None else None, nv if vcap is None else vcap, abi.ptr(otri),
                                             nt if tcap is None else tcap, abi.ptr(vmap), *[C.byref(c) for c in c7])
    return rc, [c.value for c in c7], oxyz, orgb, otri, vmap


def _seven(want):
    return [len(want[0]), len(want[2])] + [want[3][k] for k in COUNTS[3:] + QUADRIC]


@pytest.mark.parametrize("cell", sorted(CRAFTED))
def test_crafted_mesh(ctx, cell):
    xyz, rgb, tris = crafted_mesh(0)
    want = mqr.simplify(xyz, rgb, tris, cell)
    assert (len(want[0]), len(want[2]), want[3]["duplicates_dropped"]) == CRAFTED[cell]
    mean = ctx.simplify_mesh(xyz, rgb, tris, cell)
    got = ctx.simplify_mesh(xyz, rgb, tris, cell, placement="quadric")
    print(f"cell {cell}: {want[3]['quadric_placed']} of {want[3]['clusters']} clusters placed, {want[3]['clamped']} clamped, "
          f"{want[3]['corners_skipped']} corners skipped; {int((got[0] != mean[0]).any(axis=1).sum())} positions differ from the mean's")
    _assert_quadric(got, want, mean, "host")
    assert want[3]["quadric_placed"] > 0 and (got[0] != mean[0]).any()
    _assert_quadric(ctx.simplify_mesh(xyz, rgb, tris, cell, placement="quadric"), got, None, "second run")
    dx, dr, dt, dinfo = ctx.simplify_mesh(_dev(xyz), _dev(rgb), _dev(tris), cell, placement="quadric")
    assert dx.is_cuda and dr.is_cuda and dt.is_cuda and dinfo["vert_map"].is_cuda
    _assert_quadric((_host(dx), _host(dr), _host(dt), dict(dinfo, vert_map=_host(dinfo["vert_map"]))), want, mean, "device")
    # without colours
    nx, nr, nt, ninfo = ctx.simplify_mesh(xyz, None, tris, cell, placement="quadric")
    assert nr is None
    _assert_quadric((nx, None, nt, ninfo), (want[0], None, want[2], want[3]), None, "no colours")
    # vert_map is optional
    rc, counts, oxyz, orgb, otri, _ = _raw(ctx, xyz, rgb, tris, cell, vert_map=False)
    kv, kt = len(want[0]), len(want[2])
    assert rc == abi.OK and counts == _seven(want)
    _same_bytes(oxyz[:kv], want[0], "xyz"); _same_bytes(orgb[:kv], want[1], "rgb"); _same_bytes(otri[:kt], want[2], "tris")
    # an origin that is no multiple of the cell; a NULL origin is (0, 0, 0)
    _assert_quadric(ctx.simplify_mesh(xyz, rgb, tris, cell, origin=CRAFTED_ORIGIN, placement="quadric"),
                    mqr.simplify(xyz, rgb, tris, cell, CRAFTED_ORIGIN), ctx.simplify_mesh(xyz, rgb, tris, cell, origin=CRAFTED_ORIGIN), "shifted")
    _assert_quadric(ctx.simplify_mesh(xyz, rgb, tris, cell, origin=(0.0, 0.0, 0.0), placement="quadric"), want, None, "origin 0")
    # another reg is another result, and the reference's
    _assert_quadric(ctx.simplify_mesh(xyz, rgb, tris, cell, placement="quadric", reg=0.25), mqr.simplify(xyz, rgb, tris, cell, reg=0.25), mean,
                    "reg 0.25")


@pytest.mark.parametrize("k", range(len(ROOFS)))
def test_roof_crease_is_kept(ctx, k):
    """the feature: the clusters on the crease end on the crease; the mean call's end a fifth of a cell off"""
    inp, want, _ = reference(f"roof {k}")
    got, mean = _quadric(ctx, inp), ctx.simplify_mesh(*inp)
    crease = roof_crease_clusters(inp[0], got[3]["vert_map"])
    dq, dm = roof_distance(got[0][crease]), roof_distance(mean[0][crease])
    print(f"roof {ROOFS[k]}: quadric {dq.min():.4f}..{dq.max():.4f} cell, mean {dm.min():.4f}..{dm.max():.4f} cell from the crease")
    assert len(crease) >= 3 and dq.max() <= 0.005 and dm.min() >= 0.05
    _assert_quadric(got, want, mean, f"roof {k}")


def test_cube_corner_is_kept(ctx):
    inp, want, _ = reference("corner")
    got, mean = _quadric(ctx, inp), ctx.simplify_mesh(*inp)
    c = np.unique(got[3]["vert_map"][(inp[0] == np.array(CORNER, np.float32)).all(axis=1)])
    assert len(c) == 1
    dq = np.linalg.norm(got[0][c[0]].astype(np.float64) - CORNER)
    dm = np.linalg.norm(mean[0][c[0]].astype(np.float64) - CORNER)
    print(f"corner: quadric {dq:.4f} cell, mean {dm:.4f} cell from the corner")
    assert dq <= 0.005 and dm >= 0.1
    _assert_quadric(got, want, mean, "corner")


@pytest.mark.parametrize("name", ["plane", "spans", "without area", "crease outside"])
def test_edge_rules(ctx, name):
    inp, want, mean = reference(name)
    got = _quadric(ctx, inp)
    _assert_quadric(got, want, ctx.simplify_mesh(*inp), name)
    if name == "without area":                                      # the mean rule: the mean call's bytes
        _same_bytes(got[0], mean[0], "xyz")
    if name == "crease outside":
        assert got[3]["clamped"] == 1


def test_carry_case(ctx):
    """4096 triangles and 2^16 further vertices on one record: terms of both signs whose low words wrap thousands of times (what
    makes it so is asserted on the CPU, test_mesh_simplify_quadric_reference_cpu.py)"""
    inp, want, _ = reference("carry")
    assert len(inp[2]) == CARRY_TRIS and want[3]["n"].max() == CARRY_FILL + CARRY_TRIS
    got = _quadric(ctx, inp)
    _assert_quadric(got, want, ctx.simplify_mesh(*inp), "carry")
    _assert_quadric(_quadric(ctx, inp), got, None, "carry, second run")
    dx, dr, dt, dinfo = ctx.simplify_mesh(_dev(inp[0]), _dev(inp[1]), _dev(inp[2]), inp[3], placement="quadric")
    _assert_quadric((_host(dx), _host(dr), _host(dt), dict(dinfo, vert_map=_host(dinfo["vert_map"]))), want, None, "carry, device")


@pytest.mark.parametrize("name", WRAPPED + ("soup",))
def test_key_table_wrap_case_and_soup(ctx, name):
    inp, want, _ = reference(name)
    got = _quadric(ctx, inp)
    print(f"{name}: {want[3]['quadric_placed']} of {want[3]['clusters']} placed, {want[3]['clamped']} clamped, {want[3]['corners_skipped']} skipped")
    _assert_quadric(got, want, ctx.simplify_mesh(*inp), name)
    _assert_quadric(_quadric(ctx, inp), got, None, name + ", second run")


@pytest.mark.parametrize("n_tri", [0, 2047, 2048, 2049])
def test_chunk_edges(ctx, n_tri):
    xyz, rgb, tris = crafted_mesh(0)
    tris = np.ascontiguousarray(tris[:n_tri])
    want = mqr.simplify(xyz, rgb, tris, 0.04)
    _assert_quadric(ctx.simplify_mesh(xyz, rgb, tris, 0.04, placement="quadric"), want, ctx.simplify_mesh(xyz, rgb, tris, 0.04), f"{n_tri} triangles")
    assert (want[3]["quadric_placed"] == 0) == (n_tri == 0)


def test_arguments(ctx):
    xyz, rgb, tris = (np.array(a) for a in crafted_mesh(0))
    nv, nt = len(xyz), len(tris)
    lib = ctx._lib
    out = (np.zeros((nv, 3), np.float32), np.zeros((nv, 3), np.uint8), np.zeros((nt, 3), np.uint32), np.zeros(nv, np.uint32))

    def call(**kw):
        return _raw(ctx, kw.pop("xyz", xyz), rgb, kw.pop("tris", tris), kw.pop("cell", 0.05), out=kw.pop("out", out), **kw)[:2]

    def untouched():
        return not any(a.any() for a in out)
    for reg in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert call(reg=reg)[0] == abi.E_INVALID and b"reg" in lib.tl3d_last_error()
    assert call(cell=0.0)[0] == abi.E_INVALID and b"cell size" in lib.tl3d_last_error()
    bad = tris.copy()
    bad[nt // 2, 1] = nv
    assert call(tris=bad)[0] == abi.E_INVALID and b"out of range" in lib.tl3d_last_error()
    far = xyz.copy()
    far[nv // 3, 2] = np.float32(0.05 * (1 << 20)) * np.float32(1.001)
    assert call(xyz=far)[0] == abi.E_INVALID and b"2^20" in lib.tl3d_last_error()
    # overlapping outputs
    for alias in ((xyz, out[1], out[2], out[3]), (out[0], out[1], tris, out[3]), (out[0], out[1], out[2], tris.reshape(-1)[:nv])):
        assert call(out=alias)[0] == abi.E_INVALID and b"aliases" in lib.tl3d_last_error()
    assert untouched()
    # short capacities: all seven counts are stored, nothing else is
    want = mqr.simplify(xyz, rgb, tris, 0.05)
    kv, kt = len(want[0]), len(want[2])
    assert want[3]["quadric_placed"] > 0 and want[3]["clamped"] > 0
    for vcap, tcap in ((kv - 1, nt), (nv, kt - 1), (0, 0)):
        rc, counts = call(vcap=vcap, tcap=tcap)
        assert rc == abi.E_CAPACITY and counts == _seven(want) and untouched()
    rc, counts = call(vcap=kv, tcap=kt)
    assert rc == abi.OK and counts == _seven(want)
    _same_bytes(out[0][:kv], want[0], "xyz"); _same_bytes(out[1][:kv], want[1], "rgb"); _same_bytes(out[2][:kt], want[2], "tris")
    _same_bytes(out[3], want[3]["vert_map"], "vert_map")
    assert not out[0][kv:].any() and not out[2][kt:].any()
    # empty inputs
    assert call(n_tri=0, n_vert=0, vcap=0, tcap=0) == (abi.OK, [0] * 7)
    assert call(n_tri=0) == (abi.OK, [kv, 0, 0, 0, 0, 0, 0])        # no triangle: every cluster at its mean
    _same_bytes(out[0][:kv], ctx.simplify_mesh(xyz, rgb, NO_TRIS, 0.05)[0], "xyz without triangles")
    empty = ctx.simplify_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), NO_TRIS, 0.05, placement="quadric")
    assert len(empty[0]) == 0 and len(empty[2]) == 0 and [empty[3][k] for k in QUADRIC] == [0, 0, 0]
    with pytest.raises(ValueError, match="placement"):
        ctx.simplify_mesh(xyz, rgb, tris, 0.05, placement="median")
    # the mean call on the same context afterwards: untouched by the quadric scratch
    _same_bytes(ctx.simplify_mesh(xyz, rgb, tris, 0.05)[0], msr.simplify(xyz, rgb, tris, 0.05)[0], "mean after quadric")


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
    pipe = DepthToReconstructionPipeline(ReconstructionConfig(**cam, voxel_size=voxel, subsample_factor=1, **kw))
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    pipe.reconstruct(grid=grid, poses=poses)
    return pipe


def test_pipeline_option():
    cell = 2 * SPECK_GRID["voxel"]
    base = dict(extract_mesh=True, mesh_min_component_triangles=SPECK_MIN_TRIANGLES)
    assert ReconstructionConfig().mesh_simplify_placement == "mean"
    plain = _speck_pipeline(**base)
    unset = _speck_pipeline(**base, mesh_simplify_cell=cell)
    mean = _speck_pipeline(**base, mesh_simplify_cell=cell, mesh_simplify_placement="mean")
    quadric = _speck_pipeline(**base, mesh_simplify_cell=cell, mesh_simplify_placement="quadric")
    # "mean" is the run without the option, byte for byte, stats included
    for a, b, name in zip(mean.mesh, unset.mesh, ("xyz", "rgb", "tris")):
        _same_bytes(a, b, "mean " + name)
    assert mean.stats["mesh_simplify"] == unset.stats["mesh_simplify"] and "placement" not in unset.stats["mesh_simplify"]
    # "quadric": the reference applied to the filtered mesh, origin (0, 0, 0)
    want = mqr.simplify(*plain.mesh, cell)
    print(f"speck scene: {want[3]['quadric_placed']} of {want[3]['clusters']} placed, {want[3]['clamped']} clamped, {want[3]['corners_skipped']} skipped")
    assert want[3]["quadric_placed"] > 0
    for a, b, name in zip(quadric.mesh, want[:3], ("xyz", "rgb", "tris")):
        _same_bytes(a, b, "quadric " + name)
    assert not np.array_equal(quadric.mesh[0], unset.mesh[0])
    assert quadric.stats["mesh_simplify"] == dict({k: want[3][k] for k in COUNTS + QUADRIC}, cell=cell, placement="quadric")
    assert quadric.stats["mesh_vertices"] == len(want[0]) and quadric.stats["mesh_triangles"] == len(want[2])
    # refused before anything is fused: a value that is no placement, and quadric placement of a mesh that is not simplified
    with pytest.raises(ValueError, match="mesh_simplify_placement"):
        _speck_pipeline(**base, mesh_simplify_cell=cell, mesh_simplify_placement="median")
    with pytest.raises(ValueError, match="mesh_simplify_cell"):
        _speck_pipeline(**base, mesh_simplify_placement="quadric")


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
    """every triangle as its three positions, rotated so that the smallest position comes first, sorted (a welded mesh lists
    vertices and triangles in another order, so another member of a set of duplicates survives)"""
    p = np.asarray(xyz, np.float64)[np.asarray(tris, np.int64)]                    # [T, 3, 3]
    first = np.lexsort((p[:, :, 2], p[:, :, 1], p[:, :, 0]), axis=1)[:, 0]
    rot = (first[:, None] + np.arange(3)[None, :]) % 3
    a = np.take_along_axis(p, rot[:, :, None], axis=1).reshape(len(p), 9)
    return a[np.lexsort(a.T[::-1])]


def test_blocked_run_gives_the_single_lattice_mesh():
    """12 VGA frames down the corridor at 2 cm, one lattice and the same lattice forced into blocks, quadric placement: the same
    vertices and triangles as sets, because a cluster's quadric sums, like its other sums, do not depend on the order of the
    triangles, and the welded mesh has the single lattice's triangles"""
    W, H = 640, 480
    cam = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0)
    poses = synth.dolly_poses(12, (0.0, 0.0, 0.0), (0.0, 0.0, 0.1))
    frames = [synth.render(synth.corridor_scene(), p, W, H, **cam) for p in poses]
    base = dict(**cam, voxel_size=0.02, subsample_factor=2, grid_dim=512, outlier_filter=False, extract_mesh=True, mesh_simplify_cell=0.05,
                mesh_simplify_placement="quadric")
    one = _corridor_run(base, frames, poses, None)
    many = _corridor_run(base, frames, poses, one.grid.nvox // 3)
    assert one.stats["blocks"] == 1 and many.stats["blocks"] >= 3
    (ax, ar, at), (bx, br, bt) = one.mesh, many.mesh
    assert len(ax) == len(bx) and len(at) == len(bt) and len(at) > 0
    assert np.array_equal(_vertex_rows(ax, ar), _vertex_rows(bx, br))
    assert np.array_equal(_triangle_rows(ax, at), _triangle_rows(bx, bt))
    assert one.stats["mesh_simplify"] == many.stats["mesh_simplify"] and one.stats["mesh_simplify"]["quadric_placed"] > 0


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
              run("--output", str(tmp_path / "b.ply"), "--mesh-output", str(simple), "--mesh-simplify-cell", "0.05",
                  "--mesh-simplify-placement", "quadric")):
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "quadric placement" in r.stdout
    xyz, col, tris = _read_ply_mesh(plain)
    want = mqr.simplify(xyz, col, tris, 0.05)
    for a, b in zip(_read_ply_mesh(simple), want[:3]):
        assert np.array_equal(a, b)
    r = run("--output", str(tmp_path / "d.ply"), "--mesh-output", str(simple), "--mesh-simplify-placement", "quadric")
    assert r.returncode == 2 and "--mesh-simplify-cell" in r.stderr
