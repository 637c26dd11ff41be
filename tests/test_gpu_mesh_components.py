"""GPU: connected components of a mesh and the filter built on them (tl3d_mesh_components, tl3d_mesh_filter_components,
DESIGN.md section 4.2.1) against the scipy restatement of the rules (tests/mesh_components_reference.py), bit for bit: the crafted
grid of test_gpu_mesh.py, topologies on which a union-find goes wrong, the argument checks, the pipeline option on one grid and
across blocks, and the command-line flags."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_components_reference as mcr
import tl3d
from helpers import SMALL, make_pair
from mesh_components_common import (DIMS, KEPT, SPECK_GRID, SPECK_MIN_TRIANGLES, TOPOLOGIES, VOXEL, CENTRE, crafted_mesh, crafted_records,
                                    speck_scene, topology)
from tl3d import _cabi as abi
from tl3d import fileio, synth
from tl3d import pipeline as pl
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bare_ctx():
    """a context without a grid: the calls need none"""
    return tl3d.FusionContext(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], n_slots=1, grid=None)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _same_bytes(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what


def _assert_components(got, want, what=""):
    _same_bytes(got[0], want[0], what + " labels")
    _same_bytes(got[1], want[1], what + " counts")
    assert got[2] == want[2], (what, got[2], want[2])


def _assert_filtered(got, want, what=""):
    for a, b, name in zip(got[:3], want[:3], ("xyz", "rgb", "tris")):
        if a is None or b is None:
            assert a is None and b is None, f"{what} {name}"
        else:
            _same_bytes(np.asarray(a), np.asarray(b), f"{what} {name}")
    for k in ("components", "components_kept", "vertices_dropped", "triangles_dropped"):
        assert got[3][k] == want[3][k], (what, k, got[3][k], want[3][k])
    assert np.array_equal(np.asarray(got[3]["keep_vert"]), want[3]["keep_vert"]), what + " keep_vert"


@pytest.fixture(scope="module")
def crafted_ctx():
    """the crafted grid on the device; its meshes at min_weight 0 and 2 are the reference's, so both sides label the same input"""
    ctx, _ = make_pair(dims=DIMS, voxel=VOXEL, centre=CENTRE, channels=tl3d.CH_TSDF)
    rec, _ = crafted_records()
    ctx.upload_grid(tl3d.CH_TSDF, rec)
    meshes = {}
    for mw in (0, 2):
        meshes[mw] = ctx.extract_mesh(min_weight=mw)
        for a, b in zip(meshes[mw], crafted_mesh(mw)):
            assert np.array_equal(a, b)
    yield ctx, meshes
    ctx.close()


@pytest.mark.parametrize("min_weight", [0, 2])
def test_crafted_grid_labels_counts_and_component_count(crafted_ctx, min_weight):
    ctx, meshes = crafted_ctx
    xyz, rgb, tris = meshes[min_weight]
    want = mcr.components(tris, len(xyz))
    assert want[2] == (119 if min_weight == 0 else 1802)
    first = ctx.mesh_components(tris, len(xyz))
    _assert_components(first, want, "host")
    _assert_components(ctx.mesh_components(tris, len(xyz)), first, "second run")
    dl, dc, dn = ctx.mesh_components(_dev(tris), len(xyz))
    assert dl.is_cuda and dc.is_cuda
    _assert_components((_host(dl), _host(dc), dn), want, "device")
    # the counts are optional
    lab, n = np.zeros(len(xyz), np.uint32), C.c_int64(0)
    abi.check(ctx._lib.tl3d_mesh_components(ctx._h, abi.ptr(tris), len(tris), len(xyz), abi.ptr(lab), None, C.byref(n)))
    assert np.array_equal(lab, want[0]) and n.value == want[2]


@pytest.mark.parametrize("largest_only", [False, True])
@pytest.mark.parametrize("min_triangles", sorted(KEPT))
def test_crafted_grid_filter(crafted_ctx, min_triangles, largest_only):
    ctx, meshes = crafted_ctx
    xyz, rgb, tris = meshes[0]
    want = mcr.filter_mesh(xyz, rgb, tris, min_triangles, largest_only)
    figures = (len(want[0]), len(want[2]), want[3]["components_kept"])
    if largest_only:
        assert figures == ((2877, 5445, 1) if min_triangles <= 5445 else (0, 0, 0))
    else:
        assert figures == KEPT[min_triangles]
    got = ctx.filter_mesh(xyz, rgb, tris, min_triangles, largest_only)
    _assert_filtered(got, want, "host")
    _assert_filtered(ctx.filter_mesh(xyz, rgb, tris, min_triangles, largest_only), got, "second run")
    dx, dr, dt, dinfo = ctx.filter_mesh(_dev(xyz), _dev(rgb), _dev(tris), min_triangles, largest_only)
    assert dx.is_cuda and dr.is_cuda and dt.is_cuda
    _assert_filtered((_host(dx), _host(dr), _host(dt), dict(dinfo, keep_vert=_host(dinfo["keep_vert"]))), want, "device")
    if min_triangles == 0 and not largest_only:                    # the identity, isolated vertices included
        _assert_filtered(got, (xyz, rgb, tris, dict(want[3], components_kept=119, vertices_dropped=0, triangles_dropped=0)), "identity")
    # without colours
    nx, nr, nt, ninfo = ctx.filter_mesh(xyz, None, tris, min_triangles, largest_only)
    assert nr is None and np.array_equal(nx, want[0]) and np.array_equal(nt, want[2])


def test_crafted_grid_filter_of_the_sparse_mesh(crafted_ctx):
    """min_weight 2: 1 802 components, 1 704 of them vertices no triangle uses"""
    ctx, meshes = crafted_ctx
    xyz, rgb, tris = meshes[2]
    for mt, largest in ((0, False), (1, False), (3, False), (0, True)):
        _assert_filtered(ctx.filter_mesh(xyz, rgb, tris, mt, largest), mcr.filter_mesh(xyz, rgb, tris, mt, largest), f"{mt} {largest}")
    assert ctx.filter_mesh(xyz, rgb, tris, 1)[3]["vertices_dropped"] == 1704


@pytest.mark.parametrize("name", TOPOLOGIES)
def test_topologies_where_a_union_find_goes_wrong(name):
    tris, n_vert = topology(name)
    want = mcr.components(tris, n_vert)
    with _bare_ctx() as ctx:
        got = ctx.mesh_components(tris, n_vert)
        _assert_components(got, want, name)
        _assert_components(ctx.mesh_components(tris, n_vert), got, name + ", second run")
        if name == "4096 strips interleaved":                      # compaction over 512 chunks: every strip has 254 triangles
            xyz = np.arange(3 * n_vert, dtype=np.float32).reshape(-1, 3)
            s_, j_ = tris[:, 0] % 4096, tris[:, 0] // 4096
            cut = tris[(s_ % 2 == 1) | (j_ < s_ % 200)]            # strips of odd s whole, strip s of even s cut to s % 200 triangles
            for mt in (254, 255, 100):
                _assert_filtered(ctx.filter_mesh(xyz, None, cut, mt), mcr.filter_mesh(xyz, None, cut, mt), f"{name} {mt}")


def test_arguments():
    xyz, rgb, tris = (np.array(a) for a in crafted_mesh(0))
    nv, nt = len(xyz), len(tris)
    with _bare_ctx() as ctx:                                       # (a context created with grid=None)
        lib = ctx._lib
        lab, cnt, n = np.zeros(nv, np.uint32), np.zeros(nv, np.uint32), C.c_int64(0)
        oxyz, orgb, otri, keep = np.zeros((nv, 3), np.float32), np.zeros((nv, 3), np.uint8), np.zeros((nt, 3), np.uint32), np.zeros(nv, np.uint8)
        c4 = [C.c_int64(-1) for _ in range(4)]

        def filt(tri=tris, n_tri=nt, n_vert=nv, mt=10, oxyz=oxyz, vcap=nv, otri=otri, tcap=nt):
            return lib.tl3d_mesh_filter_components(ctx._h, abi.ptr(xyz), abi.ptr(rgb), n_vert, abi.ptr(tri), n_tri, mt, 0, abi.ptr(oxyz),
                                                   abi.ptr(orgb), vcap, abi.ptr(otri), tcap, abi.ptr(keep), *[C.byref(c) for c in c4])
        # an index equal to n_vert: refused by the validation pass (the only kernel that has run: nothing indexed follows it)
        bad = tris.copy()
        bad[nt // 2, 1] = nv
        assert lib.tl3d_mesh_components(ctx._h, abi.ptr(bad), nt, nv, abi.ptr(lab), abi.ptr(cnt), C.byref(n)) == abi.E_INVALID
        assert b"out of range" in lib.tl3d_last_error()
        assert filt(tri=bad) == abi.E_INVALID and b"out of range" in lib.tl3d_last_error()
        assert lib.tl3d_mesh_components(ctx._h, abi.ptr(tris), nt, nv - 1, abi.ptr(lab), abi.ptr(cnt), C.byref(n)) == abi.E_INVALID
        # the context still works afterwards
        _assert_components(ctx.mesh_components(tris, nv), mcr.components(tris, nv), "after a refusal")
        # aliased outputs
        assert lib.tl3d_mesh_components(ctx._h, abi.ptr(tris), nt, nv, abi.ptr(tris.reshape(-1)), abi.ptr(cnt), C.byref(n)) == abi.E_INVALID
        assert filt(oxyz=xyz) == abi.E_INVALID and b"aliases" in lib.tl3d_last_error()
        assert filt(otri=tris) == abi.E_INVALID and b"aliases" in lib.tl3d_last_error()
        # short capacities: the true counts are stored
        kv, kt, kc = KEPT[10]
        for vcap, tcap in ((kv - 1, nt), (nv, kt - 1), (0, 0)):
            assert filt(vcap=vcap, tcap=tcap) == abi.E_CAPACITY
            assert [c.value for c in c4] == [kv, kt, 119, kc]
        assert filt(vcap=kv, tcap=kt) == abi.OK and [c.value for c in c4] == [kv, kt, 119, kc]
        want = mcr.filter_mesh(xyz, rgb, tris, 10)
        assert np.array_equal(oxyz[:kv], want[0]) and np.array_equal(orgb[:kv], want[1]) and np.array_equal(otri[:kt], want[2])
        assert np.array_equal(keep.astype(bool), want[3]["keep_vert"])
        # threshold 5446: an empty mesh, TL3D_OK
        assert filt(mt=5446) == abi.OK and [c.value for c in c4] == [0, 0, 119, 0]
        # empty inputs
        assert lib.tl3d_mesh_components(ctx._h, None, 0, 0, None, None, C.byref(n)) == abi.OK and n.value == 0
        assert lib.tl3d_mesh_components(ctx._h, None, 0, 5, abi.ptr(lab), abi.ptr(cnt), C.byref(n)) == abi.OK and n.value == 5
        assert np.array_equal(lab[:5], np.arange(5)) and not cnt[:5].any()
        assert filt(n_tri=0, n_vert=0, vcap=0, tcap=0) == abi.OK and [c.value for c in c4] == [0, 0, 0, 0]
        for mt, kept in ((0, 6), (1, 0)):                          # vertices without a triangle: all of them, or none
            assert filt(n_tri=0, n_vert=6, mt=mt) == abi.OK and [c.value for c in c4] == [kept, 0, 6, kept]
        got = ctx.filter_mesh(xyz[:6], rgb[:6], np.zeros((0, 3), np.uint32), 0)
        assert np.array_equal(got[0], xyz[:6]) and np.array_equal(got[1], rgb[:6]) and len(got[2]) == 0
        assert ctx.filter_mesh(xyz[:6], rgb[:6], np.zeros((0, 3), np.uint32), 0, largest_only=True)[3]["components_kept"] == 0
        empty = ctx.filter_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.uint32), 3)
        assert len(empty[0]) == 0 and len(empty[2]) == 0 and empty[3]["components"] == 0
        assert ctx.mesh_components(np.zeros((0, 3), np.uint32), 0)[2] == 0


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
    return pipe, out, speck


def test_pipeline_drops_a_flying_speck(tmp_path):
    off, cloud_off, speck = _speck_pipeline(extract_mesh=True)
    on, cloud_on, _ = _speck_pipeline(extract_mesh=True, mesh_min_component_triangles=SPECK_MIN_TRIANGLES)
    assert np.array_equal(cloud_off[0], cloud_on[0]) and np.array_equal(cloud_off[1], cloud_on[1])        # the cloud is not touched
    assert "mesh_components" not in off.stats and "mesh_filter_s" not in off.timings
    xyz, rgb, tris = off.mesh
    labels, counts, n = mcr.components(tris, len(xyz))
    near = np.linalg.norm(xyz - speck, axis=1) < 0.1
    print(f"unfiltered: {len(xyz)} vertices, {len(tris)} triangles, {n} components, largest {np.sort(counts)[-3:]}, near the speck "
          f"{near.sum()} vertices in components of {counts[np.unique(labels[near])]} triangles")
    assert n >= 2 and near.sum() >= 20 and 0 < counts[np.unique(labels[near])].max() < SPECK_MIN_TRIANGLES < counts.max()
    want = mcr.filter_mesh(xyz, rgb, tris, SPECK_MIN_TRIANGLES)
    for a, b, name in zip(on.mesh, want[:3], ("xyz", "rgb", "tris")):
        _same_bytes(a, b, name)
    assert not (np.linalg.norm(on.mesh[0] - speck, axis=1) < 0.1).any()
    info = {k: v for k, v in want[3].items() if k != "keep_vert"}
    assert on.stats["mesh_components"] == info and info["components"] == n and info["components_kept"] >= 1
    assert on.stats["mesh_vertices"] == len(want[0]) and on.stats["mesh_triangles"] == len(want[2]) and "mesh_filter_s" in on.timings
    assert off.stats["mesh_vertices"] == len(xyz) and off.stats["mesh_triangles"] == len(tris)
    on.save_mesh(str(tmp_path / "filtered.ply"))
    for a, b in zip(_read_ply_mesh(tmp_path / "filtered.ply"), on.mesh):
        assert np.array_equal(a, b)
    # largest_only through the pipeline
    big, _, _ = _speck_pipeline(extract_mesh=True, mesh_largest_component=True)
    for a, b in zip(big.mesh, mcr.filter_mesh(xyz, rgb, tris, 0, True)[:3]):
        assert np.array_equal(a, b)
    assert big.stats["mesh_components"]["components_kept"] == 1
    # the options filter a mesh: refused without one, before anything is fused
    for kw in (dict(mesh_min_component_triangles=5), dict(mesh_largest_component=True)):
        with pytest.raises(ValueError, match="extract_mesh"):
            _speck_pipeline(**kw)


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
    plain, small, big = (tmp_path / n for n in ("plain.ply", "small.ply", "big.ply"))
    for r in (run("--output", str(tmp_path / "a.ply"), "--mesh-output", str(plain)),
              run("--output", str(tmp_path / "b.ply"), "--mesh-output", str(small), "--mesh-min-component", "100"),
              run("--output", str(tmp_path / "c.ply"), "--mesh-output", str(big), "--mesh-largest-component")):
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes() == (tmp_path / "c.ply").read_bytes()
    xyz, col, tris = _read_ply_mesh(plain)
    n = mcr.components(tris, len(xyz))[2]
    assert n >= 2
    for path, mt, largest in ((small, 100, False), (big, 0, True)):
        want = mcr.filter_mesh(xyz, col, tris, mt, largest)
        assert 0 < len(want[2]) < len(tris)
        fileio.write_ply_mesh(str(tmp_path / "want.ply"), *want[:3])
        assert path.read_bytes() == (tmp_path / "want.ply").read_bytes()
    for extra in (("--mesh-min-component", "100"), ("--mesh-largest-component",)):
        r = run("--output", str(tmp_path / "d.ply"), *extra)
        assert r.returncode == 2 and "--mesh-output" in r.stderr


# ---- across blocks ------------------------------------------------------------------------------------------------------------
def _sorted_rows(*cols):
    a = np.concatenate([np.asarray(c).reshape(len(c), -1).astype(np.float64) for c in cols], axis=1)
    return a[np.lexsort(a.T[::-1])]


@pytest.fixture(scope="module")
def short_corridor():
    """12 VGA frames down the corridor at 2 cm; the unfiltered single-grid run, its lattice and its components (the reference's)"""
    W, H = 640, 480
    cam = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0)
    poses = synth.dolly_poses(12, (0.0, 0.0, 0.0), (0.0, 0.0, 0.1))
    frames = [synth.render(synth.corridor_scene(), p, W, H, **cam) for p in poses]
    base = dict(**cam, voxel_size=0.02, subsample_factor=2, grid_dim=512, outlier_filter=False, extract_mesh=True)
    plain = _corridor_run(base, frames, poses, None)
    assert plain.stats["blocks"] == 1
    labels, counts, n = mcr.components(plain.mesh[2], len(plain.mesh[0]))
    return base, frames, poses, plain, (labels, counts, n)


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


@pytest.mark.parametrize("option", [dict(mesh_min_component_triangles=100), dict(mesh_largest_component=True)])
def test_filtered_welded_mesh_equals_the_filtered_single_grid_mesh(short_corridor, option):
    base, frames, poses, plain, (labels, counts, n) = short_corridor
    top = np.sort(counts)[-2:]
    print(f"unfiltered: {len(plain.mesh[0])} vertices, {len(plain.mesh[2])} triangles, {n} components, two largest {top}")
    assert n >= 3 and top[1] > top[0]                              # largest_only has one answer
    assert top[1] >= 100 and ((counts > 0) & (counts < 100)).any()         # the threshold keeps something and drops something
    one = _corridor_run(dict(base, **option), frames, poses, None)
    many = _corridor_run(dict(base, **option), frames, poses, plain.grid.nvox // 3)
    assert one.stats["blocks"] == 1 and many.stats["blocks"] >= 3
    want = mcr.filter_mesh(*plain.mesh, option.get("mesh_min_component_triangles", 0), option.get("mesh_largest_component", False))
    for a, b, name in zip(one.mesh, want[:3], ("xyz", "rgb", "tris")):
        _same_bytes(a, b, name)
    (ax, ar, at), (bx, br, bt) = one.mesh, many.mesh
    assert len(ax) == len(bx) and len(at) == len(bt) and 0 < len(at) < len(plain.mesh[2])
    assert np.array_equal(_sorted_rows(ax, ar), _sorted_rows(bx, br))
    assert np.array_equal(_sorted_rows(ax[at[:, 0]], ax[at[:, 1]], ax[at[:, 2]]), _sorted_rows(bx[bt[:, 0]], bx[bt[:, 1]], bx[bt[:, 2]]))
    assert one.stats["mesh_components"] == many.stats["mesh_components"] == {k: v for k, v in want[3].items() if k != "keep_vert"}
    assert many.stats["mesh_vertices"] == len(bx) and many.stats["mesh_triangles"] == len(bt) and "mesh_filter_s" in many.timings
