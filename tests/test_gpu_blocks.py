"""GPU: a lattice fused block by block equals the single lattice bit for bit -- TSDF records of offset grids, brick counts,
detach / attach in one context, block cores (points, TSDF-mode points, welded keyed mesh, statistics), the refusals, and the
pipeline beyond 2^32 voxels."""
import numpy as np
import pytest

import tl3d
from extract_reference import record_index
from helpers import SMALL, small_scene_frames
from tl3d import _cabi as abi
from tl3d import pipeline as pl
from tl3d import synth
from tl3d.config import ReconstructionConfig
from tl3d.fusion import GridSpec
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu

N, VOXEL = 256, 0.01
LATTICE = GridSpec((N, N, N), (-1.28, -1.28, -1.28), VOXEL, 4 * VOXEL)


def _frames():
    return small_scene_frames(n=8, deg=12.0, radius=1.0)


def _ctx(grid=None, n_slots=8):
    return tl3d.FusionContext(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], n_slots=n_slots,
                              grid=grid)


def _upload(ctx, frames):
    for i, (d, c) in enumerate(frames):
        ctx.upload(i, d, c)


def _fuse(ctx, poses):
    ctx.fuse_frames(list(range(len(poses))), poses, centroid_subsample=1)


def _xyz_major(rec, dims):
    """brick-major records -> [nx, ny, nz, ...]"""
    return rec[record_index(dims)]


def _sorted_rows(*cols):
    m = np.concatenate([np.asarray(c).reshape(len(c), -1).astype(np.float64) if np.asarray(c).dtype != np.float32 else
                        np.asarray(c).view(np.int32).reshape(len(c), -1).astype(np.float64) for c in cols], axis=1)
    return m[np.lexsort(m.T[::-1])]


def _blocks(ctx=None, poses=None, limit=136 ** 3):
    """The halo'd blocks of the lattice; with ctx: sparse, pools from the block's own brick count"""
    out = []
    for b in pl.plan_blocks(LATTICE, limit):
        g = b.grid
        if ctx is not None:
            t, c = ctx.count_bricks(g, list(range(len(poses))), poses, centroid_subsample=1)
            g = GridSpec(g.dims, g.origin, g.voxel_size, g.sdf_trunc, g.channels, pool_tsdf=t + 64, pool_centroid=c + 64,
                         voxel_offset=g.voxel_offset)
        out.append(pl.Block(g, b.lo, b.hi))
    return out


@pytest.fixture(scope="module")
def single():
    """The single lattice: TSDF records, points, keyed mesh, statistics."""
    poses, frames = _frames()
    with _ctx(LATTICE) as ctx:
        _upload(ctx, frames)
        counts = ctx.count_bricks(LATTICE, list(range(len(poses))), poses, centroid_subsample=1)
        _fuse(ctx, poses)
        st = ctx.stats()
        tsdf = _xyz_major(ctx.download_grid(tl3d.CH_TSDF), LATTICE.dims)
        cen = ctx.extract(tl3d.EXTRACT_CENTROID, min_count=1, min_weight=1, max_abs_tsdf=0.9)
        tpts = ctx.extract(tl3d.EXTRACT_TSDF)
        mesh = ctx.extract_mesh(keys=True)
    assert len(mesh[2]) > 5000 and len(cen[0]) > 5000
    return dict(poses=poses, frames=frames, counts=counts, st=st, tsdf=tsdf, cen=cen, tpts=tpts, mesh=mesh)


@pytest.mark.parametrize("sparse", [False, True])
def test_offset_blocks_hold_the_single_lattice_records(single, sparse):
    """8 disjoint 128^3 blocks (offsets, no halo): every block's TSDF records are the single grid's over its region, bit for bit,
    and the per-block brick counts sum to the single count."""
    poses, frames = single["poses"], single["frames"]
    nt = nc = 0
    with _ctx() as ctx:
        _upload(ctx, frames)
        for ox in (0, 128):
            for oy in (0, 128):
                for oz in (0, 128):
                    g = GridSpec((128, 128, 128), LATTICE.origin, VOXEL, LATTICE.sdf_trunc, voxel_offset=(ox, oy, oz))
                    t, c = ctx.count_bricks(g, list(range(len(poses))), poses, centroid_subsample=1)
                    nt, nc = nt + t, nc + c
                    if sparse:
                        g = GridSpec(g.dims, g.origin, VOXEL, g.sdf_trunc, pool_tsdf=t + 64, pool_centroid=c + 64, voxel_offset=g.voxel_offset)
                    ctx.attach_grid(g)
                    _fuse(ctx, poses)
                    got = _xyz_major(ctx.download_grid(tl3d.CH_TSDF), g.dims)
                    assert ctx.stats()["pool_refused"] == 0
                    ctx.detach_grid()
                    want = single["tsdf"][ox:ox + 128, oy:oy + 128, oz:oz + 128]
                    assert np.array_equal(got, want), (ox, oy, oz, int(np.sum(np.any(got != want, axis=-1))))
    assert (nt, nc) == tuple(single["counts"])


def test_detach_then_attach_equals_a_fresh_context(single):
    """Three attach -> fuse -> extract -> mesh -> detach cycles on one context (dense, sparse, dense): after each detach the grid,
    its tables and the grid-sized extraction and mesh scratch have gone back to the device, and the last cycle's grid is a fresh
    context's."""
    import torch
    poses, frames = single["poses"], single["frames"]
    b = GridSpec((136, 128, 136), LATTICE.origin, VOXEL, LATTICE.sdf_trunc, voxel_offset=(120, 0, 64))
    with _ctx(b) as fresh:
        _upload(fresh, frames)
        _fuse(fresh, poses)
        want = fresh.download_grid(tl3d.CH_TSDF), fresh.download_grid(tl3d.CH_CENTROID)
    with _ctx() as ctx:
        _upload(ctx, frames)
        ctx.sync()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]

        def extract_and_detach():
            ctx.extract(tl3d.EXTRACT_CENTROID)              # the extraction and the mesh scratch exist before the detach
            ctx.extract_mesh()
            ctx.detach_grid()
            assert torch.cuda.mem_get_info(0)[0] > free0 - (64 << 20)      # the grid and its scratch went back

        ctx.attach_grid(LATTICE)
        _fuse(ctx, poses)
        ctx.sync()
        assert torch.cuda.mem_get_info(0)[0] < free0 - LATTICE.device_bytes() // 2
        extract_and_detach()
        for call in (lambda: ctx.integrate(0, poses[0]), lambda: ctx.extract(tl3d.EXTRACT_CENTROID), lambda: ctx.extract_mesh(),
                     lambda: ctx.grid_ptr(tl3d.CH_TSDF), lambda: ctx.detach_grid(), lambda: ctx.set_block_core()):
            with pytest.raises(abi.Tl3dError) as e:
                call()
            assert e.value.code == abi.E_STATE
        t, c = ctx.count_bricks(b, list(range(len(poses))), poses, centroid_subsample=1)
        ctx.attach_grid(GridSpec(b.dims, b.origin, VOXEL, b.sdf_trunc, pool_tsdf=t + 64, pool_centroid=c + 64, voxel_offset=b.voxel_offset))
        _fuse(ctx, poses)
        assert ctx.stats()["pool_refused"] == 0 and np.array_equal(ctx.download_grid(tl3d.CH_TSDF), want[0])
        extract_and_detach()
        ctx.attach_grid(b)
        with pytest.raises(abi.Tl3dError) as e:
            ctx.attach_grid(b)
        assert e.value.code == abi.E_STATE
        _fuse(ctx, poses)
        assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), want[0])
        assert np.array_equal(ctx.download_grid(tl3d.CH_CENTROID), want[1])
        extract_and_detach()


@pytest.mark.parametrize("sparse", [False, True])
def test_block_cores_give_the_single_lattice_points_and_mesh(single, sparse):
    """Halo'd blocks of the lattice with their cores: centroid and TSDF-mode points, the welded keyed mesh and centroid_points
    equal the single grid's (points sorted, vertices and colours bit for bit, triangles as sets)."""
    poses, frames = single["poses"], single["frames"]
    cen, tp, parts, kept = [], [], [], 0
    with _ctx() as ctx:
        _upload(ctx, frames)
        blocks = _blocks(ctx, poses) if sparse else _blocks()
        assert len(blocks) == 8 and all(b.grid.sparse == sparse for b in blocks)
        for b in blocks:
            ctx.attach_grid(b.grid)
            ctx.set_block_core(LATTICE.dims, b.lo, b.hi)
            ctx.reset_stats()
            _fuse(ctx, poses)
            st = ctx.stats()
            assert st["pool_refused"] == 0
            kept += st["centroid_points"]
            assert st["centroid_points"] + st["centroid_dropped"] == single["st"]["centroid_points"] + single["st"]["centroid_dropped"]
            cen.append(ctx.extract(tl3d.EXTRACT_CENTROID, min_count=1, min_weight=1, max_abs_tsdf=0.9))
            tp.append(ctx.extract(tl3d.EXTRACT_TSDF))
            x, r, t, k = ctx.extract_mesh(keys=True)
            off = np.asarray(b.grid.voxel_offset)
            parts.append((x, r, t, k, off + np.asarray(b.lo), off + np.asarray(b.hi)))
            with pytest.raises(abi.Tl3dError) as e:
                ctx.raycast(poses[0])
            assert e.value.code == abi.E_STATE
            ctx.detach_grid()
    assert kept == single["st"]["centroid_points"]
    for got, want in ((cen, single["cen"]), (tp, single["tpts"])):
        gx, gr = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
        assert len(gx) == len(want[0])
        assert np.array_equal(_sorted_rows(gx, gr), _sorted_rows(*want))
    wx, wr, wt, wk = pl.weld_meshes(parts, LATTICE.dims)
    sx, sr, st_, sk = single["mesh"]
    assert len(wx) == len(sx) and len(wt) == len(st_)
    ow, os_ = np.argsort(wk), np.argsort(sk)
    assert np.array_equal(wk[ow], sk[os_])
    assert np.array_equal(wx[ow], sx[os_]) and np.array_equal(wr[ow], sr[os_])
    tw, ts = wk[wt.astype(np.int64)], sk[st_.astype(np.int64)]
    assert np.array_equal(tw[np.lexsort(tw.T[::-1])], ts[np.lexsort(ts.T[::-1])])


def test_core_and_offset_refusals():
    with _ctx(GridSpec((64, 64, 64), LATTICE.origin, VOXEL, LATTICE.sdf_trunc, voxel_offset=(8, 0, 0))) as ctx:
        with pytest.raises(abi.Tl3dError) as e:
            ctx.raycast((np.eye(3), np.zeros(3)))
        assert e.value.code == abi.E_STATE
        for bad in (((1 << 21, 1 << 20, 1 << 20), (0, 0, 0), (64, 64, 64)),     # 2^61 voxels: keys would overflow
                    ((72, 64, 64), (0, 0, 0), (64, 64, 72)), ((72, 64, 64), (4, 0, 0), (64, 64, 64)), ((64, 64, 64), (0, 0, 0), (64, 64, 64))):
            with pytest.raises(abi.Tl3dError) as e:
                ctx.set_block_core(*bad)
            assert e.value.code == abi.E_INVALID
    with pytest.raises(abi.Tl3dError) as e:
        _ctx(GridSpec((64, 64, 64), LATTICE.origin, VOXEL, LATTICE.sdf_trunc, voxel_offset=((1 << 23) - 56, 0, 0)))
    assert e.value.code == abi.E_INVALID


def _corridor_run(cfg, frames, poses, limit=None, monkeypatch=None):
    if limit is not None:
        monkeypatch.setattr(pl, "MAX_BLOCK_VOXELS", limit)
    pipe = DepthToReconstructionPipeline(cfg)
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    pts, col, _ = pipe.reconstruct(poses=poses)
    return pipe, pts, col


@pytest.fixture(scope="module")
def corridor():
    W, H = 640, 480
    cam = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0)
    scene = synth.corridor_scene()
    poses = synth.dolly_poses(40, (0.0, 0.0, 0.0), (0.0, 0.0, 0.1))
    frames = [synth.render(scene, p, W, H, **cam) for p in poses]
    return cam, poses, frames


def test_pipeline_forced_split_equals_the_single_grid(corridor, monkeypatch):
    """A config-3-sized corridor with the block limit lowered so that it needs >= 3 blocks: points bit for bit (no filter), the
    same kept set with the filter, the same mesh, the same dropped count; render_dir is refused before fusion."""
    cam, poses, frames = corridor
    cfg = ReconstructionConfig(**cam, voxel_size=0.005, subsample_factor=2, grid_dim=1024, outlier_filter=False, extract_mesh=True)
    one, p1, c1 = _corridor_run(cfg, frames, poses)
    assert one.stats["blocks"] == 1 and len(one.blocks) == 1
    limit = one.grid.nvox // 3
    many, p3, c3 = _corridor_run(cfg, frames, poses, limit, monkeypatch)
    assert many.stats["blocks"] >= 3 and all(b.nvox <= limit for b in many.blocks)
    assert many.grid.dims == one.grid.dims and many.grid.origin == one.grid.origin
    assert len(p3) == len(p1) and np.array_equal(_sorted_rows(p3.astype(np.float32), c3), _sorted_rows(p1.astype(np.float32), c1))
    for k in ("points_accumulated", "points_dropped", "voxels"):
        assert many.stats[k] == one.stats[k], k
    (ax, ar, at), (bx, br, bt) = one.mesh, many.mesh
    assert len(ax) == len(bx) and len(at) == len(bt) and len(at) > 10000
    ka, kb = _sorted_rows(ax, ar), _sorted_rows(bx, br)
    assert np.array_equal(ka, kb)
    ta = _sorted_rows(ax[at[:, 0]], ax[at[:, 1]], ax[at[:, 2]])
    tb = _sorted_rows(bx[bt[:, 0]], bx[bt[:, 1]], bx[bt[:, 2]])
    assert np.array_equal(ta, tb)
    # with the outlier filter: one filter over the whole cloud.  Its neighbour sums run in a fixed cell order, but the input order
    # differs (block by block), so a point exactly at the threshold could in principle flip; none may otherwise.
    cfg_f = ReconstructionConfig(**cam, voxel_size=0.005, subsample_factor=2, grid_dim=1024, outlier_filter=True)
    monkeypatch.setattr(pl, "MAX_BLOCK_VOXELS", 1 << 32)
    _, f1, fc1 = _corridor_run(cfg_f, frames, poses)
    _, f3, fc3 = _corridor_run(cfg_f, frames, poses, limit, monkeypatch)
    s1 = {tuple(r) for r in _sorted_rows(f1.astype(np.float32), fc1).tolist()}
    s3 = {tuple(r) for r in _sorted_rows(f3.astype(np.float32), fc3).tolist()}
    assert len(s1 ^ s3) <= max(2, len(s1) // 100000), len(s1 ^ s3)
    cfg_r = ReconstructionConfig(**cam, voxel_size=0.005, subsample_factor=2, grid_dim=1024, render_dir="/nonexistent/never")
    with pytest.raises(ValueError, match="render_dir"):
        _corridor_run(cfg_r, frames, poses, limit, monkeypatch)


def test_a_120_m_corridor_beyond_2_32_voxels():
    """2 m x 2.4 m x 120 m at 5 mm: a lattice of ~4.8e9 voxels, fused in blocks.  Nothing dropped or refused, every metre of the
    corridor holds points on the analytic walls, and the cloud is the restated Open3D merge of the same frames."""
    from oracle import ref_numpy as rn
    W, H = 640, 480
    cam = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0)
    scene = synth.Scene(room=((-1.0, -1.2, -0.5), (1.0, 1.2, 120.0)))
    n = 240
    poses = synth.dolly_poses(n, (0.0, 0.0, 0.0), (0.0, 0.0, 0.5))
    frames = [synth.render(scene, p, W, H, **cam) for p in poses]
    cfg = ReconstructionConfig(**cam, voxel_size=0.005, subsample_factor=2, grid_dim=512, max_depth=4.0, outlier_filter=False)
    pipe = DepthToReconstructionPipeline(cfg)
    pipe.set_frames([c for d, c in frames], [d for d, c in frames])
    pts, col, _ = pipe.reconstruct(poses=poses)
    assert pipe.grid.nvox > 2 ** 32 and pipe.stats["blocks"] >= 2
    assert all(b.device_bytes() < 40 * 2 ** 30 for b in pipe.blocks)
    st = pipe.stats
    assert st["points_dropped"] == 0 and st["pool_refused"] == 0
    far = 120.0
    z = pts[:, 2]
    hist = np.histogram(z, bins=np.arange(2.0, far + 1e-9, 1.0))[0]      # (the walls come into the first camera's view 1.6 m ahead)
    assert np.all(hist > 0), np.nonzero(hist == 0)
    d = np.minimum(np.minimum(np.abs(np.abs(pts[:, 0]) - 1.0), np.abs(np.abs(pts[:, 1]) - 1.2)), np.abs(z - far))
    assert d.mean() < 1e-3 and np.percentile(d, 99) < 4e-3, (d.mean(), np.percentile(d, 99))
    clouds = [rn.backproject(dd, cc, cam["fx"], cam["fy"], cam["cx"], cam["cy"], pose=p, subsample=2, max_depth=4.0)
              for (dd, cc), p in zip(frames, poses)]
    ref_p, _ = rn.merge_open3d(clouds, cfg.voxel_size, sor=False)
    assert abs(len(pts) - len(ref_p)) <= 1e-3 * len(ref_p), (len(pts), len(ref_p))
    # mean Chamfer over 400 000 random points of each side (against the whole other cloud)
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    ia, ib = rng.choice(len(pts), min(len(pts), 400000), replace=False), rng.choice(len(ref_p), min(len(ref_p), 400000), replace=False)
    ch = 0.5 * (cKDTree(ref_p).query(pts[ia])[0].mean() + cKDTree(pts).query(ref_p[ib])[0].mean())
    assert ch < 1e-5, ch
