"""The TSDF update on small grids whose bricks form ragged, sparse or crowded 2x2x2 blocks of neighbours, against the C oracle bit
for bit: grids with odd brick counts, grids of one brick and of two, blocks in which one brick, two bricks one behind the other,
four or all eight are listed, bricks of one block that share no frame, batches of 1 to 41 frames cut anywhere, f32 and 16-bit
frames, dense and sparse layouts, the caches and the batching on and off, replayed and refined passes.  The update kernel takes
the batch list brick by brick, so none of this depends on how bricks are handed to waves; the cases are the ones at which an update
that hands neighbouring bricks out together (not done) could go wrong, and every one of them runs the records'
read-modify-write.

Shapes: grids of 5x5x5 and 9x8x11 bricks, of one brick and of two; images of 96x128 and 160x120; orbit frames with holes and
out-of-range pixels; walls in front of a 2x2x2-brick grid for the crafted blocks."""
import functools
import os

import numpy as np
import pytest

import tl3d
from tl3d import synth
from oracle import c_oracle

pytestmark = pytest.mark.gpu

VOX = 1.0 / 64.0
TRUNC = 4 * VOX
NF = 41                                          # 32 + 9: two launches
CUTS = (1, 2, 31, 32, 41)
SIZES = [(96, 128), (160, 120)]
GRIDS = {"5x5x5": ((40, 40, 40), (-0.3125, -0.3125, -0.3125)), "9x8x11": ((72, 64, 88), (-0.5625, -0.5, -0.6875)),
         "1x1x1": ((8, 8, 8), (0.125, -0.0625, -0.0625)), "2x1x1": ((16, 8, 8), (0.0625, -0.0625, -0.0625))}


def _cam(w, h):
    return dict(width=w, height=h, fx=0.9 * w, fy=0.9 * w, cx=0.5 * w - 0.5, cy=0.5 * h - 0.5)


def _with_env(want, make):
    old = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return make()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ctx(cam, spec, n_slots, caches=True, mind=0.1, maxd=50.0):
    """the cache switches are read when the context is created"""
    env = {"TL3D_CLASS_CACHE": None if caches else "0", "TL3D_TILE_CACHE": None if caches else "0", "TL3D_CLASS_CACHE_ENTRIES": None,
           "TL3D_CLASS_REFINE": None}
    return _with_env(env, lambda: tl3d.FusionContext(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                                                     min_depth=mind, max_depth=maxd, n_slots=n_slots, grid=spec))


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    """NF views of the object scene on an orbit of 8 degrees per frame; holes and out-of-range pixels in the lower half"""
    scene = synth.object_scene(with_room=True)
    poses = synth.orbit_poses(NF, 1.0, 8.0)
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


@functools.lru_cache(maxsize=None)
def _mm(w, h):
    out = []
    for d in _frames(w, h)[1]:
        mm = np.clip(np.rint(np.where(d < 60.0, d, 0.0).astype(np.float64) * 1000.0), 0, 65535).astype(np.uint16)
        mm.setflags(write=False)
        out.append(mm)
    return out


@functools.lru_cache(maxsize=None)
def _refs(w, h, grid, u16=False, passes=1):
    """the oracle's grid after the first n frames, n in CUTS, fused `passes` times over (read-only, shared)"""
    dims, origin = GRIDS[grid]
    poses, frames = _frames(w, h)
    if u16:
        frames = [m.astype(np.float32) / np.float32(1000.0) for m in _mm(w, h)]
    out = {}
    for n in CUTS:
        if passes > 1 and n != 32:
            continue
        c = _cam(w, h)
        orc = c_oracle.Oracle(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], dims=dims, origin=origin, voxel_size=VOX,
                              sdf_trunc=TRUNC)
        for _ in range(passes):
            for i in range(n):
                orc.tsdf_integrate(frames[i], *poses[i])
        g = orc.tsdf.copy()
        g.setflags(write=False)
        out[n] = g
    return out


def _same(got, want, what):
    assert np.array_equal(got, want), (what, int((got != want).any(axis=-1).sum()))


def _spec(grid, **kw):
    dims, origin = GRIDS[grid]
    return tl3d.GridSpec(dims, origin, VOX, TRUNC, tl3d.CH_TSDF, **kw)


def _upload(ctx, w, h, u16=False):
    poses, frames = _frames(w, h)
    for i, d in enumerate(_mm(w, h) if u16 else frames):
        ctx.upload(i, d)
    return poses


# ---- grids, image sizes, batch lengths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("wh", SIZES, ids=["96x128", "160x120"])
def test_batches_of_1_2_31_32_41_frames(wh, grid):
    w, h = wh
    refs = _refs(w, h, grid)
    with _ctx(_cam(w, h), _spec(grid), NF) as ctx:
        poses = _upload(ctx, w, h)
        for n in CUTS:
            ctx.reset()
            ctx.reset_stats()
            ctx.fuse_frames(list(range(n)), poses[:n])
            _same(ctx.download_grid(tl3d.CH_TSDF), refs[n], (grid, wh, n))
            assert ctx.stats()["tsdf_launches"] == (n + 31) // 32, n


@pytest.mark.parametrize("grid", ["5x5x5", "9x8x11"])
def test_u16_frames(grid):
    w, h = SIZES[0]
    refs = _refs(w, h, grid, u16=True)
    with _ctx(_cam(w, h), _spec(grid), NF) as ctx:
        poses = _upload(ctx, w, h, u16=True)
        for n in (2, 32, 41):
            ctx.reset()
            ctx.fuse_frames(list(range(n)), poses[:n])
            _same(ctx.download_grid(tl3d.CH_TSDF), refs[n], (grid, n))


@pytest.mark.parametrize("caches", [True, False], ids=["caches", "no_caches"])
@pytest.mark.parametrize("pairing", [True, False], ids=["batched", "one_per_launch"])
def test_pairing_and_caches_on_and_off(pairing, caches):
    w, h = SIZES[1]
    refs = _refs(w, h, "9x8x11")
    with _ctx(_cam(w, h), _spec("9x8x11"), NF, caches=caches) as ctx:
        poses = _upload(ctx, w, h)
        ctx.set_tsdf_pairing(pairing)
        for n in (2, 32):
            ctx.reset()
            ctx.reset_stats()
            ctx.fuse_frames(list(range(n)), poses[:n])
            _same(ctx.download_grid(tl3d.CH_TSDF), refs[n], (pairing, caches, n))
            assert ctx.stats()["tsdf_launches"] == (1 if pairing else n)


def test_replayed_and_refined_passes():
    """six passes over the same 32 frames: the second replays and refines (8 entries per chain and pass), the sixth replays level 3"""
    w, h = SIZES[0]
    with _ctx(_cam(w, h), _spec("5x5x5"), NF) as ctx:
        poses = _upload(ctx, w, h)
        for k in range(1, 7):
            ctx.fuse_frames(list(range(32)), poses[:32])
            if k in (2, 6):
                _same(ctx.download_grid(tl3d.CH_TSDF), _refs(w, h, "5x5x5", passes=k)[32], k)
        assert ctx.class_cache_info()[1] >= 5 * 32 and ctx.class_refine_info()[0] > 0


@pytest.mark.parametrize("grid", ["5x5x5", "9x8x11"])
def test_sparse_layout_and_a_pool_that_fills(grid):
    w, h = SIZES[0]
    want = _refs(w, h, grid)[32]
    dims = GRIDS[grid][0]
    nb = (dims[0] // 8) * (dims[1] // 8) * (dims[2] // 8)
    for pool in (nb, 24):
        with _ctx(_cam(w, h), _spec(grid, pool_tsdf=pool), NF) as ctx:
            poses = _upload(ctx, w, h)
            ctx.fuse_frames(list(range(32)), poses[:32])
            got = ctx.download_grid(tl3d.CH_TSDF)
        if pool == nb:
            _same(got, want, (grid, "pool holds every brick"))
        else:
            # a refused brick misses the frames that listed it (its free-space observations are still folded in): a record is the
            # oracle's, or holds fewer observations than the oracle's
            differs = (got != want).any(axis=-1)
            assert differs.any(), "the pool was meant to fill"
            assert (got[differs][:, 1] < want[differs][:, 1]).all(), int(differs.sum())


def test_counting_mode_and_where_the_batch_is_cut():
    """The grid does not depend on where the batches are cut (a sync closes the pending batch).  Visited and free-space bricks are
    counted per frame: the same wherever the cuts fall.  Records are read and written once per launch and brick, so a batch of
    several frames counts fewer than the same frames one per launch; with every launch holding one frame the counts are equal."""
    w, h = SIZES[1]
    want = _refs(w, h, "9x8x11")[41]
    seen = {}
    with _ctx(_cam(w, h), _spec("9x8x11"), NF) as ctx:
        poses = _upload(ctx, w, h)
        ctx.set_profile(count_records=True)
        for cuts in ((41,), (1, 40), (7, 2, 32), (20, 21), (1,) * 41):
            ctx.reset()
            ctx.reset_stats()
            i = 0
            for c in cuts:
                ctx.fuse_frames(list(range(i, i + c)), poses[i:i + c])
                ctx.sync()
                i += c
            _same(ctx.download_grid(tl3d.CH_TSDF), want, cuts)
            st = ctx.stats()
            assert st["tsdf_launches"] == sum((c + 31) // 32 for c in cuts), cuts
            assert st["tsdf_records_read"] == st["tsdf_records_written"] > 0
            seen[cuts] = (st["tsdf_bricks_visited"], st["tsdf_bricks_free"], st["tsdf_bricks_free_counted"], st["tsdf_records_read"])
        ctx.set_tsdf_pairing(False)
        ctx.reset()
        ctx.reset_stats()
        ctx.fuse_frames(list(range(41)), poses)
        st = ctx.stats()
        assert st["tsdf_launches"] == 41
        single = (st["tsdf_bricks_visited"], st["tsdf_bricks_free"], st["tsdf_bricks_free_counted"], st["tsdf_records_read"])
    for cuts, s in seen.items():
        assert s[:3] == single[:3], (cuts, s, single)
        assert s[3] <= single[3], (cuts, s, single)
    assert seen[(1,) * 41] == single


# ---- crafted blocks: walls in front of a grid of 2x2x2 bricks -----------------------------------------------------------------------
W, H = 96, 128
CAM = dict(width=W, height=H, fx=100.0, fy=100.0, cx=47.5, cy=63.5)
G_DIMS, G_ORIGIN, G_VOX, G_TRUNC = (16, 16, 16), (-0.16, -0.16, 0.84), 0.02, 0.04
FRONT = (np.eye(3), np.zeros(3))                                                   # at the origin, looking along +z: layer z0 is near
BACK = (np.diag([-1.0, 1.0, -1.0]), np.array([0.0, 0.0, 2.0]))                      # at (0, 0, 2), looking along -z: layer z1 is near


def _wall(z, u0=0, u1=W, v0=0, v1=H):
    d = np.zeros((H, W), np.float32)
    d[v0:v1, u0:u1] = z
    return d


def _crafted(frames, trunc=G_TRUNC):
    """(grid, visited bricks, free bricks) of the frames [(depth, pose)] fused in one batch -- the grid checked against the oracle"""
    orc = c_oracle.Oracle(W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], dims=G_DIMS, origin=G_ORIGIN, voxel_size=G_VOX, sdf_trunc=trunc)
    with _ctx(CAM, tl3d.GridSpec(G_DIMS, G_ORIGIN, G_VOX, trunc, tl3d.CH_TSDF), len(frames)) as ctx:
        ctx.set_profile(count_records=True)
        for i, (d, p) in enumerate(frames):
            ctx.upload(i, d)
            orc.tsdf_integrate(d, *p)
        ctx.fuse_frames(list(range(len(frames))), [p for _, p in frames])
        got = ctx.download_grid(tl3d.CH_TSDF)
        st = ctx.stats()
    _same(got, orc.tsdf, "crafted")
    assert orc.tsdf.any()
    return got, st["tsdf_bricks_visited"] - st["tsdf_bricks_free"], st["tsdf_bricks_free"]


def test_a_block_with_all_eight_bricks_listed():
    """a wall on the plane between the two layers, the band 6 voxels either way: all eight bricks are cut"""
    _, listed, _ = _crafted([(_wall(1.0), FRONT)] * 3, trunc=0.12)
    assert listed == 3 * 8


def test_a_block_with_one_brick_listed():
    """a wall inside the near layer, seen only through the pixels of brick (0, 0, 0): the other seven have no valid pixel or lie behind"""
    _, listed, _ = _crafted([(_wall(0.90, 0, 40, 0, 56), FRONT)] * 2)
    assert listed == 2 * 1


def test_bricks_of_one_block_that_share_no_frame():
    """Frames from the front list the near layer's four bricks, frames from the back the far layer's: no brick of the block shares
    a frame with one of the other layer.  Then the two bricks (0, 0, 0) and (0, 0, 1), one behind the other, each through its own
    pixels and from its own side -- bricks 0 and 4 of the block and nothing between them.  (A hand-out that gave bricks j and j + 4
    of a block's LISTED bricks to one wave would see these two as entries 0 and 1: "one wave with two bricks beside a wave with
    none" cannot occur in a list that holds only listed bricks, so there is no such case here.)"""
    front, back = (_wall(0.90), FRONT), (_wall(0.90), BACK)
    _, listed, _ = _crafted([front, back, front, back, back])
    assert listed == 5 * 4
    _, listed, _ = _crafted([front, front])
    assert listed == 2 * 4
    _, listed, _ = _crafted([(_wall(0.90, 0, 40, 0, 56), FRONT), back, front])
    assert listed == 1 + 4 + 4
    _, listed, _ = _crafted([(_wall(0.90, 0, 40, 0, 56), FRONT), (_wall(0.90, 56, 96, 0, 56), BACK)])
    assert listed == 1 + 1
