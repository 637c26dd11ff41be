"""The TSDF prep keeps a frame's depth tiles, their pyramid and its valid pixel with the frame's slot (tl3d.h:
tl3d_tile_cache_info) and builds them again only when the slot's image or the key (scale, depth limits) changed.  Whatever the
cache does -- hit, rebuild, rebuild beside batches in flight, off -- the grid stays the oracle's bit for bit, and the build
counter says what the keys imply.

Geometry: a 64^3 grid of 1/64 m voxels (every voxel centre is exact in f32, so a block at a voxel offset and an oracle at the
shifted origin place them identically), images of 100 x 76 (16-B rows, ragged last regions) and 99 x 77 (scalar path)."""
import functools
import os

import numpy as np
import pytest

import tl3d
from tl3d import synth
from oracle import c_oracle

pytestmark = pytest.mark.gpu

VOX = 1.0 / 64.0
DIMS = (64, 64, 64)
ORIGIN = (-0.5, -0.5, -0.5)
TRUNC = 4 * VOX
SIZES = [(100, 76), (99, 77)]
N = 5


def _cam(w, h):
    return dict(width=w, height=h, fx=0.9 * w, fy=0.9 * w, cx=0.5 * w - 0.5, cy=0.5 * h - 0.5)


def _spec(dims=DIMS, origin=ORIGIN, **kw):
    return tl3d.GridSpec(dims, origin, VOX, TRUNC, tl3d.CH_TSDF, **kw)


def _ctx(w, h, n_slots=N, cache=True, grid="default", **kw):
    """A FusionContext; cache=False: created with TL3D_TILE_CACHE=0 in the environment (read when the context is created)."""
    old = os.environ.get("TL3D_TILE_CACHE")
    if cache:
        os.environ.pop("TL3D_TILE_CACHE", None)
    else:
        os.environ["TL3D_TILE_CACHE"] = "0"
    try:
        c = _cam(w, h)
        return tl3d.FusionContext(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], n_slots=n_slots,
                                  grid=_spec() if grid == "default" else grid, **kw)
    finally:
        if old is None:
            os.environ.pop("TL3D_TILE_CACHE", None)
        else:
            os.environ["TL3D_TILE_CACHE"] = old


def _orc(w, h, dims=DIMS, origin=ORIGIN, **kw):
    c = _cam(w, h)
    return c_oracle.Oracle(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], dims=dims, origin=origin, voxel_size=VOX,
                           sdf_trunc=TRUNC, **kw)


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    """N views of the object scene from outside the grid: free space in front of the spheres, the spheres' surfaces, and the
    bricks behind them and beside the view; scattered holes and out-of-range pixels in the lower half of every image."""
    scene = synth.object_scene(with_room=True)
    poses = synth.orbit_poses(N, 1.0, 15.0)
    rng = np.random.default_rng(w * 1000 + h)
    out = []
    for p in poses:
        d, _ = synth.render(scene, p, **_cam(w, h), want_color=False)
        d = np.ascontiguousarray(d, np.float32)
        r = rng.random(d.shape)
        r[: h // 2] = 1.0
        d[r < 0.02] = 0.0
        d[(r >= 0.02) & (r < 0.03)] = 80.0
        d.setflags(write=False)
        out.append(d)
    return poses, out


def _far(w, h):
    """Nothing but far free space: every voxel in view lies in front of it."""
    return np.full((h, w), 6.0, np.float32)


@functools.lru_cache(maxsize=None)
def _ref(w, h, plan):
    """Oracle grid of a plan: a tuple of (frame index, scale) fused in order (read-only, shared by the tests)."""
    poses, frames = _frames(w, h)
    orc = _orc(w, h)
    for i, sc in plan:
        orc.tsdf_integrate(frames[i], poses[i][0], poses[i][1], scale=sc)
    g = orc.tsdf.copy()
    g.setflags(write=False)
    return g


def _upload_all(ctx, w, h):
    poses, frames = _frames(w, h)
    for i, d in enumerate(frames):
        ctx.upload(i, d)
    return poses


@pytest.mark.parametrize("wh", SIZES)
def test_poses_reach_every_brick_class(wh):
    """Counting mode: the frames give FREE, MIXED and skipped bricks, so hits and rebuilds below feed all three rules."""
    w, h = wh
    with _ctx(w, h) as ctx:
        poses = _upload_all(ctx, w, h)
        ctx.set_profile(count_records=True)
        ctx.fuse_frames(list(range(N)), poses)
        ctx.sync()
        s = ctx.stats()
    nbricks = (DIMS[0] // 8) * (DIMS[1] // 8) * (DIMS[2] // 8)
    free, mixed = s["tsdf_bricks_free"], s["tsdf_bricks_visited"] - s["tsdf_bricks_free"]
    print("bricks: free", free, "mixed", mixed, "skipped", N * nbricks - s["tsdf_bricks_visited"])
    assert free > 0 and mixed > 0 and s["tsdf_bricks_visited"] < N * nbricks


@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("wh", SIZES)
def test_refuse(wh, cache):
    """Five slots fused twice equal the oracle fused twice; the second pass builds nothing (cache off: it builds again)."""
    w, h = wh
    with _ctx(w, h, cache=cache) as ctx:
        poses = _upload_all(ctx, w, h)
        for _ in range(2):
            ctx.fuse_frames(list(range(N)), poses)
            ctx.sync()
        g = ctx.download_grid(tl3d.CH_TSDF)
        builds, hits, nbytes = ctx.tile_cache_info()
    assert np.array_equal(g, _ref(w, h, tuple((i, 1.0) for i in range(N)) * 2))
    if cache:
        assert builds == N and hits >= N
    else:
        assert builds == 2 * N
    assert nbytes > 0


@pytest.mark.parametrize("wh", SIZES)
def test_resets_without_a_build(wh):
    """Batches that find every tile built launch no build kernel: the batch's resets (list cursors, batch list, ticket counters,
    histogram bins) come from the kernel that always runs.  Nine synced passes use every batch scratch at least twice."""
    w, h = wh
    with _ctx(w, h) as ctx:
        poses = _upload_all(ctx, w, h)
        for _ in range(9):
            ctx.fuse_frames(list(range(N)), poses)
            ctx.sync()
        g = ctx.download_grid(tl3d.CH_TSDF)
        builds, hits, _ = ctx.tile_cache_info()
    assert builds == N and hits == 8 * N
    assert np.array_equal(g, _ref(w, h, tuple((i, 1.0) for i in range(N)) * 9))


@pytest.mark.parametrize("writer", ["upload", "raycast"])
@pytest.mark.parametrize("wh", SIZES)
def test_new_image_in_a_slot(wh, writer):
    """Slot 1 holds far free space and is fused; then another image goes into the SAME slot -- a surface inside the grid -- by an
    upload or by a ray cast into the slot, and is fused: stale tiles would call the surface's bricks free space."""
    w, h = wh
    poses, frames = _frames(w, h)
    far = _far(w, h)
    aa = _orc(w, h)
    aa.tsdf_integrate(far, *poses[1])
    aa.tsdf_integrate(far, *poses[1])
    with _ctx(w, h) as ctx:
        orc = _orc(w, h)
        if writer == "raycast":                         # something to cast rays at
            ctx.upload(0, frames[0])
            ctx.integrate(0, poses[0])
            orc.tsdf_integrate(frames[0], *poses[0])
            aa.tsdf_integrate(frames[0], *poses[0])
        ctx.upload(1, far)
        ctx.integrate(1, poses[1])
        orc.tsdf_integrate(far, *poses[1])
        if writer == "upload":
            ctx.upload(1, frames[1])
            b = frames[1]
        else:
            ctx.raycast(poses[0], slot=1)
            b = ctx.download_depth(1)
            assert (b > 0).any()                        # (how much of a surface: the oracle comparison below says enough)
        ctx.integrate(1, poses[1])
        orc.tsdf_integrate(b, *poses[1])
        g = ctx.download_grid(tl3d.CH_TSDF)
        builds, _, _ = ctx.tile_cache_info()
    assert not np.array_equal(orc.tsdf, aa.tsdf), "oracle(A, B) must differ from oracle(A, A)"
    assert np.array_equal(g, orc.tsdf)
    assert builds == (3 if writer == "raycast" else 2)


@pytest.mark.parametrize("wh", SIZES)
def test_key_change(wh):
    """One slot at scale 1.0 and 1.25 back to back (the batch is cut between them), the same with a sync in between, then a count
    with another max_depth followed by a fuse: a build per change of key, the oracle's grid throughout."""
    w, h = wh
    poses, frames = _frames(w, h)
    with _ctx(w, h) as ctx:
        ctx.upload(0, frames[0])
        ctx.integrate(0, poses[0], 1.0)
        ctx.integrate(0, poses[0], 1.25)
        g1 = ctx.download_grid(tl3d.CH_TSDF)
        b1 = ctx.tile_cache_info()[0]
        ctx.integrate(0, poses[0], 1.0)
        ctx.sync()
        ctx.integrate(0, poses[0], 1.25)
        ctx.sync()
        g2 = ctx.download_grid(tl3d.CH_TSDF)
        b2 = ctx.tile_cache_info()[0]
        ctx.count_bricks(_spec(), [0], [poses[0]], centroid_subsample=0, max_depth=1.3)
        b3 = ctx.tile_cache_info()[0]
        ctx.integrate(0, poses[0], 1.25)        # the key of the last fuse, but the count rebuilt the tiles with its own limits
        ctx.integrate(0, poses[0], 1.25)
        g3 = ctx.download_grid(tl3d.CH_TSDF)
        b4, hits, _ = ctx.tile_cache_info()
    plan = ((0, 1.0), (0, 1.25))
    assert np.array_equal(g1, _ref(w, h, plan))
    assert np.array_equal(g2, _ref(w, h, plan * 2))
    assert np.array_equal(g3, _ref(w, h, plan * 2 + ((0, 1.25), (0, 1.25))))
    assert (b1, b2, b3, b4) == (2, 4, 5, 6) and hits == 1
    # the limits are part of what the tiles hold: the count's would have changed the grid
    poses, frames = _frames(w, h)
    near = _orc(w, h, max_depth=1.3)
    near.tsdf_integrate(frames[0], *poses[0], scale=1.25)
    wide = _orc(w, h)
    wide.tsdf_integrate(frames[0], *poses[0], scale=1.25)
    assert not np.array_equal(near.tsdf, wide.tsdf)


@pytest.mark.parametrize("wh", SIZES)
def test_u16_then_f32_into_one_slot(wh):
    w, h = wh
    poses, frames = _frames(w, h)
    mm = np.clip(np.rint(frames[0] * 1000.0), 0, 65535).astype(np.uint16)
    orc = _orc(w, h)
    with _ctx(w, h) as ctx:
        ctx.upload(0, mm)
        ctx.integrate(0, poses[0])
        orc.tsdf_integrate(mm.astype(np.float32) / np.float32(1000.0), *poses[0])
        ctx.upload(0, frames[2])
        ctx.integrate(0, poses[2])
        orc.tsdf_integrate(frames[2], *poses[2])
        g = ctx.download_grid(tl3d.CH_TSDF)
        builds = ctx.tile_cache_info()[0]
    assert np.array_equal(g, orc.tsdf) and builds == 2


@pytest.mark.parametrize("wh", SIZES)
def test_count_then_fuse(wh):
    """The count pass fills the cache and the fusion of the same frames builds nothing; the counts are those of a context with the
    cache off."""
    w, h = wh
    counts = {}
    for cache in (True, False):
        with _ctx(w, h, cache=cache) as ctx:
            poses = _upload_all(ctx, w, h)
            counts[cache] = ctx.count_bricks(_spec(), list(range(N)), poses, centroid_subsample=0)
            after_count = ctx.tile_cache_info()[0]
            ctx.fuse_frames(list(range(N)), poses)
            g = ctx.download_grid(tl3d.CH_TSDF)
            after_fuse = ctx.tile_cache_info()[0]
        assert np.array_equal(g, _ref(w, h, tuple((i, 1.0) for i in range(N))))
        assert (after_count, after_fuse) == ((N, N) if cache else (N, 2 * N))
    assert counts[True] == counts[False] and counts[True][0] > 0


@pytest.mark.parametrize("wh", SIZES)
def test_count_cuts_the_chain_at_a_second_scale(wh):
    """One count of slots [0, 0, 1] at scales [1.0, 1.25, 1.0]: slot 0 needs two sets of tiles, so the call issues two chains and
    builds three times (an uncut chain would share slot 0's build: two).  The counts are those of a context with the cache off and
    of one where the second use has a slot of its own."""
    w, h = wh
    poses, frames = _frames(w, h)
    scales = [1.0, 1.25, 1.0]
    with _ctx(w, h) as ctx:
        _upload_all(ctx, w, h)
        cut = ctx.count_bricks(_spec(), [0, 0, 1], [poses[0], poses[0], poses[1]], scales, centroid_subsample=0)
        builds = ctx.tile_cache_info()[0]
    with _ctx(w, h, cache=False) as ctx:
        _upload_all(ctx, w, h)
        off = ctx.count_bricks(_spec(), [0, 0, 1], [poses[0], poses[0], poses[1]], scales, centroid_subsample=0)
    with _ctx(w, h) as ctx:
        _upload_all(ctx, w, h)
        ctx.upload(2, frames[0])
        own = ctx.count_bricks(_spec(), [0, 2, 1], [poses[0], poses[0], poses[1]], scales, centroid_subsample=0)
    print("counts: cut", cut, "cache off", off, "own slot", own, "builds", builds)
    assert cut[0] > 0 and cut == off and cut == own
    assert builds == 3


def _flight_plan(order):
    """70 integrates cycling over three slots; the scale alternates with every integrate (a slot meets both scales in turn: the
    batches are cut every three frames, a dozen in flight over the prep streams) or with every 32 (three full batches, each
    rebuilding what the one before it reads)."""
    return tuple((i % 3, (1.0, 1.25)[(i if order == "frame" else i // 32) % 2]) for i in range(70))


@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("order", ["frame", "batch"])
@pytest.mark.parametrize("wh", SIZES)
def test_batches_in_flight(wh, order, cache):
    """Rebuilds beside readers, no host wait in between: the oracle's grid, three times over in one process."""
    w, h = wh
    plan = _flight_plan(order)
    ref = _ref(w, h, plan)
    poses, frames = _frames(w, h)
    with _ctx(w, h, n_slots=3, cache=cache) as ctx:
        for i in range(3):
            ctx.upload(i, frames[i])
        for rep in range(3):
            if rep:
                ctx.reset()
            for i, sc in plan:
                ctx.integrate(i, poses[i], sc)
            assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), ref), (order, cache, rep)


@pytest.mark.parametrize("wh", SIZES)
def test_two_blocks_build_once_per_frame(wh):
    """A lattice of 128 x 64 x 64 voxels fused as two blocks of 64^3 (attach_grid at a voxel offset): every frame goes into both
    blocks and its tiles are built once; grids are the oracle's, meshes those of a context with the cache off."""
    w, h = wh
    poses, frames = _frames(w, h)
    origin = (-1.0, -0.5, -0.5)
    meshes = {}
    for cache in (True, False):
        with _ctx(w, h, cache=cache, grid=None) as ctx:
            for i, d in enumerate(frames):
                ctx.upload(i, d)
            meshes[cache] = []
            for bx in (0, 1):
                ctx.attach_grid(_spec(origin=origin, voxel_offset=(64 * bx, 0, 0)))
                ctx.set_block_core((128, 64, 64), (0, 0, 0), (64, 64, 64))
                ctx.fuse_frames(list(range(N)), poses)
                g = ctx.download_grid(tl3d.CH_TSDF)
                meshes[cache].append(ctx.extract_mesh())
                ctx.detach_grid()
                if cache:
                    orc = _orc(w, h, origin=(origin[0] + 64 * bx * VOX, origin[1], origin[2]))
                    for d, p in zip(frames, poses):
                        orc.tsdf_integrate(d, *p)
                    assert orc.tsdf[:, 1].sum() > 0
                    assert np.array_equal(g, orc.tsdf), bx
            builds, hits, _ = ctx.tile_cache_info()
            assert (builds, hits) == ((N, N) if cache else (2 * N, 0))
    for ma, mb in zip(meshes[True], meshes[False]):
        assert len(ma[2]) > 0
        for a, b in zip(ma, mb):
            assert np.array_equal(a, b)
