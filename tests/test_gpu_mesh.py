"""GPU: marching-cubes mesh extraction (tl3d_extract_mesh) against the numpy restatement of the rules
(tests/mesh_reference.py) on fused and crafted grids, dense and sparse; the pipeline option and the command-line flag."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_reference as mr
import tl3d
from helpers import SMALL, make_pair, small_scene_frames, tiny_fused
from tl3d import _cabi as abi
from tl3d import synth
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spec_of(ctx):
    g = ctx.grid
    return tuple(g.dims), tuple(g.origin), g.voxel_size


def _assert_same(got, want):
    for a, b, name in zip(got, want, ("xyz", "rgb", "tris")):
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), name


def test_fused_grid_mesh_equals_reference_and_tsdf_extraction():
    poses, frames = small_scene_frames(n=6, deg=8.0)
    ctx, orc = make_pair(dims=(96, 96, 96), voxel=0.025, centre=(0.0, -0.2, 0.0))
    with ctx:
        for i, ((depth, bgr), pose) in enumerate(zip(frames, poses)):
            ctx.upload(i % 4, depth, bgr)
            ctx.integrate(i % 4, pose)
            ctx.accumulate_centroid(i % 4, pose)
            orc.tsdf_integrate(depth, pose[0], pose[1])
            orc.centroid_accumulate(depth, bgr, pose[0], pose[1])
        dims, origin, voxel = _spec_of(ctx)
        for mw in (0, 2):
            got = ctx.extract_mesh(min_weight=mw)
            want = mr.extract_mesh(orc.tsdf, dims, origin, voxel, min_weight=mw, centroid=orc.centroid)
            assert len(want[2]) > 1000
            _assert_same(got, want)
            # without a usable voxel at exactly sum = 0 the vertices are TSDF mode's points, in the same order
            if not ((orc.tsdf[:, 0] == 0) & (orc.tsdf[:, 1] >= max(1, mw))).any():
                pxyz, prgb = ctx.extract(tl3d.EXTRACT_TSDF, min_weight=mw)
                assert np.array_equal(pxyz, got[0]) and np.array_equal(prgb, got[1])


def _crafted(dims, voxel, origin):
    """{sum, weight} volumes: three spheres, two of them cut by the grid's upper faces, weights 1..3, exact zeros, an
    unobserved slab and column and truncated voxels"""
    rng = np.random.default_rng(7)
    ii, jj, kk = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    p = np.stack([origin[a] + (g + 0.5) * voxel for a, g in enumerate((ii, jj, kk))], axis=-1)
    s1 = np.linalg.norm(p - np.array([0.1, 0.05, 0.3]), axis=-1) - 0.17
    s2 = np.linalg.norm(p - np.array([0.45, 0.2, 0.9]), axis=-1) - 0.3         # cut by the upper x and y faces
    s3 = np.linalg.norm(p - np.array([0.2, 0.1, 1.4]), axis=-1) - 0.2          # cut by the upper z face
    sdf = np.minimum(np.minimum(s1, s2), s3)
    t = np.clip(sdf / (3 * voxel), -1.0, 1.0)
    w = rng.integers(1, 4, size=dims)
    q = np.rint(t * 32767.0).astype(np.int64)
    q[rng.random(dims) < 0.02] = 0                                             # exact zeros
    s = q * w
    s[np.abs(sdf) > 3.5 * voxel] = np.sign(sdf[np.abs(sdf) > 3.5 * voxel]).astype(np.int64) * 32767 * w[np.abs(sdf) > 3.5 * voxel]
    w[:, :, 30:33] = 0                                                         # unobserved slab across a brick face
    s[:, :, 30:33] = 0
    w[5:9, 3:7, :] = 0
    s[5:9, 3:7, :] = 0
    return mr.records_from_volume(s, w)


def test_crafted_grid_mesh_equals_reference():
    dims, voxel = (40, 24, 72), 0.02
    centre = (0.3, 0.2, 0.7)
    ctx, _ = make_pair(dims=dims, voxel=voxel, centre=centre, channels=tl3d.CH_TSDF)
    with ctx:
        dims_, origin, voxel_ = _spec_of(ctx)
        rec = _crafted(dims, voxel, origin)
        assert ((rec[:, 0] == 0) & (rec[:, 1] > 0)).sum() > 100
        ctx.upload_grid(tl3d.CH_TSDF, rec)
        for mw in (0, 2):
            got = ctx.extract_mesh(min_weight=mw)
            want = mr.extract_mesh(rec, dims, origin, voxel, min_weight=mw)
            assert len(want[2]) > (500 if mw == 0 else 100)
            _assert_same(got, want)
            assert (got[1] == 128).all()
            # cells at the upper faces are meshed: some vertex sits in the last voxel layer of each axis
            for a in range(3):
                assert (got[0][:, a] > origin[a] + (dims[a] - 1.5) * voxel).any(), a
        # exact zeros: the mesh has vertices TSDF mode does not emit
        pxyz, _ = ctx.extract(tl3d.EXTRACT_TSDF)
        assert len(pxyz) < len(ctx.extract_mesh()[0])


def test_sparse_grid_mesh_equals_dense():
    poses, frames = small_scene_frames(n=5, deg=4.0)
    dims, voxel, centre = (96, 96, 96), 0.025, (0.0, -0.2, 0.0)
    ctx, orc = make_pair(dims=dims, voxel=voxel, centre=centre, n_slots=5)
    origin = tuple(centre[i] - 0.5 * dims[i] * voxel for i in range(3))
    sp = tl3d.FusionContext(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], n_slots=5, grid=None)
    with ctx, sp:
        for c in (ctx, sp):
            for i, (d, col) in enumerate(frames):
                c.upload(i, d, col)
        geom = tl3d.GridSpec(dims, origin, voxel, 4 * voxel, tl3d.CH_TSDF | tl3d.CH_CENTROID)
        nt, nc = sp.count_bricks(geom, list(range(5)), poses, centroid_subsample=1)
        nbr = 96 ** 3 // 512
        assert 0 < nt < nbr
        sp.attach_grid(tl3d.GridSpec(dims, origin, voxel, 4 * voxel, tl3d.CH_TSDF | tl3d.CH_CENTROID, pool_tsdf=nt + 8,
                                     pool_centroid=nc + 8))
        for c in (ctx, sp):
            for i in range(5):
                c.integrate(i, poses[i])
                c.accumulate_centroid(i, poses[i], subsample=1)
        dense = ctx.download_grid(tl3d.CH_TSDF).reshape(-1, 512, 2)
        free_only = ((dense[:, :, 1] > 0) & (dense[:, :, 0] == 32767 * dense[:, :, 1])).all(axis=1)
        assert free_only.sum() > 10                                   # bricks that saw nothing but free space
        for mw in (0, 2):
            a = sp.extract_mesh(mw)
            b = ctx.extract_mesh(mw)
            assert len(a[2]) > 1000
            _assert_same(a, b)


def test_repeatability_and_short_buffers():
    poses, frames = small_scene_frames(n=3, deg=4.0)
    ctx, _ = make_pair(dims=(64, 64, 64), voxel=0.03)
    with ctx:
        for i, (d, c) in enumerate(frames):
            ctx.upload(i, d, c)
            ctx.integrate(i, poses[i])
            ctx.accumulate_centroid(i, poses[i])
        a = ctx.extract_mesh()
        b = ctx.extract_mesh()
        _assert_same(a, b)
        nv, nt = len(a[0]), len(a[2])
        assert nv > 100 and nt > 100
        lib = abi.load()
        xyz = np.empty((nv, 3), np.float32)
        rgb = np.empty((nv, 3), np.uint8)
        tris = np.empty((nt, 3), np.uint32)
        for vcap, tcap in ((nv - 1, nt), (nv, nt - 1)):
            onv, ont = C.c_int64(0), C.c_int64(0)
            rc = lib.tl3d_extract_mesh(ctx._h, 0, abi.ptr(xyz), abi.ptr(rgb), vcap, abi.ptr(tris), tcap, C.byref(onv), C.byref(ont))
            assert rc == abi.E_CAPACITY and (onv.value, ont.value) == (nv, nt)
        # device outputs
        import torch
        dx = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
        dc = torch.empty((nv, 3), dtype=torch.uint8, device="cuda")
        dt = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
        onv, ont = C.c_int64(0), C.c_int64(0)
        abi.check(lib.tl3d_extract_mesh(ctx._h, 0, abi.ptr(dx), abi.ptr(dc), nv, abi.ptr(dt), nt, C.byref(onv), C.byref(ont)))
        assert np.array_equal(dx.cpu().numpy(), a[0]) and np.array_equal(dc.cpu().numpy(), a[1])
        assert np.array_equal(dt.cpu().numpy().view(np.uint32), a[2])
    cen_only, _ = make_pair(dims=(16, 16, 16), channels=tl3d.CH_CENTROID)
    with cen_only:
        with pytest.raises(abi.Tl3dError) as e:
            cen_only.extract_mesh()
        assert e.value.code == abi.E_STATE


@pytest.mark.parametrize("sparse", [False, True])
def test_keyed_mesh_into_device_tensors_equals_keyed_mesh_into_host_arrays(sparse):
    """tl3d_extract_mesh_keyed with all four arrays on the host (staged on the device, copied back) and all four on the device"""
    import torch
    with tiny_fused(sparse) as ctx:
        lib = ctx._lib
        nv, nt = C.c_int64(0), C.c_int64(0)
        abi.check(lib.tl3d_extract_mesh_keyed(ctx._h, 1, None, None, 0, None, 0, None, C.byref(nv), C.byref(nt)))
        nv, nt = nv.value, nt.value
        assert nv > 100 and nt > 100
        host = (np.full((nv, 3), -1, np.float32), np.full((nv, 3), 7, np.uint8), np.full((nt, 3), 7, np.uint32), np.full(nv, -1, np.int64))
        dev = tuple(torch.from_numpy(h.view(np.int32) if h.dtype == np.uint32 else h).to("cuda:0") for h in host)
        for xyz, rgb, tri, key in (host, dev):
            onv, ont = C.c_int64(0), C.c_int64(0)
            abi.check(lib.tl3d_extract_mesh_keyed(ctx._h, 1, abi.ptr(xyz), abi.ptr(rgb), nv, abi.ptr(tri), nt, abi.ptr(key), C.byref(onv), C.byref(ont)))
            assert (onv.value, ont.value) == (nv, nt)
        # (no synchronisation: device outputs are complete when the call returns, like host outputs)
        for h, d in zip(host, dev):
            assert np.array_equal(d.cpu().numpy().view(np.uint8), h.view(np.uint8))
        assert host[2].max() == nv - 1 and len(np.unique(host[3])) == nv and host[3].min() >= 0
        _assert_same(host[:3], ctx.extract_mesh(1))


# ---- pipeline and command line --------------------------------------------------------------------------------------
CAM = dict(fx=525.0, fy=525.0, cx=320.0, cy=240.0)
W, H = 640, 480


def _object_sequence(n):
    scene = synth.object_scene(with_room=True)
    poses = synth.orbit_poses(n, 1.0, 1.5)
    r0, t0 = poses[0]
    rel = []
    for r, t in poses:
        rr = r @ r0.T
        rel.append((rr, t.reshape(3, 1) - rr @ t0.reshape(3, 1)))
    frames = [synth.render(scene, p, W, H, **CAM) for p in poses]
    return scene, poses, rel, frames


def _scene_distances(scene, p):
    """distance of every point to each analytic surface: the spheres and the six room walls, [n][surfaces]"""
    d = [np.abs(np.linalg.norm(p - np.array(c), axis=1) - r) for c, r in scene.spheres]
    lo, hi = (np.array(x) for x in scene.room)
    d += [np.abs(p[:, a] - lo[a]) for a in range(3)] + [np.abs(hi[a] - p[:, a]) for a in range(3)]
    return np.stack(d, axis=1)


def test_pipeline_mesh_option_keeps_the_cloud_and_meets_the_surface():
    scene, poses, rel, frames = _object_sequence(8)
    out = {}
    for on in (False, True):
        cfg = ReconstructionConfig(**CAM, voxel_size=0.005, subsample_factor=2, grid_dim=512, extract_mesh=on)
        pipe = DepthToReconstructionPipeline(cfg)
        pipe.set_frames([c for d, c in frames], [d for d, c in frames])
        out[on] = (pipe.reconstruct(poses=rel), pipe)
    (pa, ca, qa), pipe_off = out[False]
    (pb, cb, qb), pipe = out[True]
    assert np.array_equal(pa, pb) and np.array_equal(ca, cb)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(qa, qb))
    assert pipe_off.mesh is None and "mesh_s" not in pipe_off.timings and "mesh_vertices" not in pipe_off.stats
    xyz, rgb, tris = pipe.mesh
    assert pipe.stats["mesh_vertices"] == len(xyz) and pipe.stats["mesh_triangles"] == len(tris) and "mesh_s" in pipe.timings
    assert len(tris) > 50000
    v = pipe.grid.voxel_size
    # camera-0 frame -> world
    R0, t0 = poses[0]
    pw = (np.asarray(R0).T @ (xyz.astype(np.float64).T - np.asarray(t0).reshape(3, 1))).T
    ds = np.sort(_scene_distances(scene, pw), axis=1)
    dist = ds[:, 0]
    # region every view covers: the vertex projects into every frame (10 px margin), is that frame's visible surface and is not
    # seen at a grazing angle there (depth range over a 7 x 7 window below 3 voxels); away from creases (a second surface within
    # 3 voxels) and from the grid's faces, where the band is cut by construction
    covered = ds[:, 1] > 3 * v
    lo = np.array(pipe.grid.origin) + 3 * v
    hi = np.array(pipe.grid.origin) + (np.array(pipe.grid.dims) - 3) * v
    covered &= ((xyz > lo) & (xyz < hi)).all(axis=1)
    for (R, t), (depth, _) in zip(poses, frames):
        pc = (np.asarray(R) @ pw.T + np.asarray(t).reshape(3, 1)).T
        z = pc[:, 2]
        u = CAM["fx"] * pc[:, 0] / z + CAM["cx"]
        w_ = CAM["fy"] * pc[:, 1] / z + CAM["cy"]
        ok = (z > 0.1) & (u >= 10) & (u < W - 10) & (w_ >= 10) & (w_ < H - 10)
        ui, vi = np.clip(np.round(u).astype(int), 10, W - 11), np.clip(np.round(w_).astype(int), 10, H - 11)
        ok &= np.abs(depth[vi, ui] - z) < 2 * v
        win = np.stack([depth[vi + dv, ui + du] for dv in range(-3, 4) for du in range(-3, 4)], axis=1)
        ok &= (win.max(axis=1) - win.min(axis=1)) < 3 * v
        covered &= ok
    t = tris.astype(np.int64)
    directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    keys = directed[:, 0] * len(xyz) + directed[:, 1]
    rev = directed[:, 1] * len(xyz) + directed[:, 0]
    open_e = directed[~np.isin(rev, keys)]
    open_cov = covered[open_e[:, 0]] & covered[open_e[:, 1]]
    print(f"mesh: {len(xyz)} vertices, {len(tris)} triangles, distance to the scene mean {dist.mean() / v:.4f} voxel, "
          f"max (covered) {dist[covered].max() / v:.4f} voxel, max (all) {dist.max() / v:.4f}, open edges {len(open_e)} "
          f"({open_cov.sum()} covered), covered {covered.mean():.3f}")
    if open_cov.any():
        print("open covered edge vertices (world):", pw[open_e[open_cov][:8, 0]])
    assert covered.sum() > 5000                     # (7 020 vertices of 265 442 in the first measured run)
    assert not open_cov.any()
    assert dist.mean() < 0.25 * v
    assert dist[covered].max() < 0.75 * v


def test_cli_mesh_output(tmp_path):
    from PIL import Image
    scene, poses, rel, frames = _object_sequence(9)
    rgb_dir, depth_dir = tmp_path / "rgb", tmp_path / "depth"
    rgb_dir.mkdir(); depth_dir.mkdir()
    for i, (d, c) in enumerate(frames):
        Image.fromarray(c[..., ::-1]).save(rgb_dir / f"frame_{i:04d}.png")
        np.save(depth_dir / f"frame_{i:04d}_depth.npy", d)
    common = ["--rgb-folder", str(rgb_dir), "--depth-folder", str(depth_dir), "--fx", "525", "--fy", "525", "--cx", "320", "--cy", "240",
              "--no-vis", "--tsdf-min-weight", "1", "--grid", "512"]
    env = dict(os.environ, TL3D_DIST_BACKEND="gloo", TL3D_SHARE_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    exe = [sys.executable, os.path.join(ROOT, "depth_to_reconstruction.py"), *common]

    def run(*extra):
        r = subprocess.run(exe + list(extra), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r
    plain, with_mesh, mesh1, mesh2, cloud2 = (tmp_path / n for n in ("plain.ply", "m.ply", "mesh1.ply", "mesh2.ply", "two.ply"))
    run("--output", str(plain))
    run("--output", str(with_mesh), "--mesh-output", str(mesh1))
    assert plain.read_bytes() == with_mesh.read_bytes()
    data = mesh1.read_bytes()
    head = data[:data.index(b"end_header\n")].decode("ascii").splitlines()
    nv = int(next(l for l in head if l.startswith("element vertex")).split()[-1])
    nf = int(next(l for l in head if l.startswith("element face")).split()[-1])
    assert nv > 10000 and nf > 10000 and head[1] == "format binary_little_endian 1.0"
    assert len(data) == data.index(b"end_header\n") + len(b"end_header\n") + 15 * nv + 13 * nf
    r2 = run("--output", str(cloud2), "--mesh-output", str(mesh2), "--gpus", "2")
    assert "Merge the per-GPU grids" in r2.stdout
    assert mesh2.read_bytes() == data
    asc = tmp_path / "mesh_ascii.ply"
    run("--output", str(tmp_path / "a.ply"), "--mesh-output", str(asc), "--ascii")
    lines = asc.read_text().splitlines()
    assert lines[1] == "format ascii 1.0" and len(lines) == lines.index("end_header") + 1 + nv + nf
