"""The TSDF prep keeps the result of a frame's brick cull and sub-brick classification with the frame's slot (tl3d.h:
tl3d_class_cache_info) under a key -- pose, scale, depth limits, grid geometry, and the slot's tiles being the ones it was made
from -- and replays it when a batch meets the slot again with that key.  Whatever the cache does -- replay, save, save beside
batches in flight, overflow, off -- the grid stays the oracle's bit for bit, and the counters say what the keys imply.

Geometry (that of test_gpu_tile_cache.py): a 64^3 grid of 1/64 m voxels, images of 100 x 76 and 99 x 77, five orbit frames with
holes and out-of-range pixels (FREE, MIXED and skipped bricks: that file's first test), and one ragged grid of 72 x 64 x 88
voxels whose brick counts (9, 8, 11) are no multiples of the 4-brick cell."""
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
RAGGED = (72, 64, 88)
RAGGED_ORIGIN = (-0.5625, -0.5, -0.6875)
TRUNC = 4 * VOX
SIZES = [(100, 76), (99, 77)]
N = 5
GRIDS = [(SIZES[0], DIMS, ORIGIN), (SIZES[1], DIMS, ORIGIN), (SIZES[0], RAGGED, RAGGED_ORIGIN)]


def _cam(w, h):
    return dict(width=w, height=h, fx=0.9 * w, fy=0.9 * w, cx=0.5 * w - 0.5, cy=0.5 * h - 0.5)


def _spec(dims=DIMS, origin=ORIGIN, **kw):
    return tl3d.GridSpec(dims, origin, VOX, TRUNC, tl3d.CH_TSDF, **kw)


def _ctx(w, h, n_slots=N, cache=True, grid="default", entries=None, **kw):
    """A FusionContext; cache=False: created with TL3D_CLASS_CACHE=0, entries: with TL3D_CLASS_CACHE_ENTRIES (both are read when
    the context is created)."""
    want = {"TL3D_CLASS_CACHE": None if cache else "0", "TL3D_CLASS_CACHE_ENTRIES": None if entries is None else str(entries)}
    old = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        c = _cam(w, h)
        return tl3d.FusionContext(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], n_slots=n_slots,
                                  grid=_spec() if grid == "default" else grid, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _orc(w, h, dims=DIMS, origin=ORIGIN, **kw):
    c = _cam(w, h)
    return c_oracle.Oracle(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], dims=dims, origin=origin, voxel_size=VOX,
                           sdf_trunc=TRUNC, **kw)


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    """N views of the object scene from outside the grid; scattered holes and out-of-range pixels in the lower half of every image."""
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


def _pose(w, h, i, kind="o"):
    """Frame i's pose; "alt": the next frame's (another view of the grid); "ulp": one f32 ulp off in one element of t."""
    poses, _ = _frames(w, h)
    if kind == "alt":
        return poses[(i + 1) % N]
    r, t = poses[i]
    if kind == "ulp":
        t = np.array(t, np.float64)
        flat = t.reshape(-1)                                # (a view: t is contiguous)
        was = np.float32(flat[0])
        flat[0] = float(np.nextafter(was, np.float32(np.inf)))
        assert np.float32(flat[0]) != was
    return r, t


@functools.lru_cache(maxsize=None)
def _ref(w, h, plan, dims=DIMS, origin=ORIGIN):
    """Oracle grid of a plan: a tuple of (frame index, pose kind, scale) fused in order (read-only, shared by the tests)."""
    _, frames = _frames(w, h)
    orc = _orc(w, h, dims=dims, origin=origin)
    for i, kind, sc in plan:
        r, t = _pose(w, h, i, kind)
        orc.tsdf_integrate(frames[i], r, t, scale=sc)
    g = orc.tsdf.copy()
    g.setflags(write=False)
    return g


ONCE = tuple((i, "o", 1.0) for i in range(N))


def _upload_all(ctx, w, h):
    poses, frames = _frames(w, h)
    for i, d in enumerate(frames):
        ctx.upload(i, d)
    return poses


def _info(ctx):
    return ctx.class_cache_info()[:3]


@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("wh,dims,origin", GRIDS)
def test_refusion(wh, dims, origin, cache):
    """Five slots fused two and three times equal the oracle fused as often; from the second pass on every frame is replayed and
    none classified (cache off: classified every time, never replayed)."""
    w, h = wh
    with _ctx(w, h, cache=cache, grid=_spec(dims, origin)) as ctx:
        poses = _upload_all(ctx, w, h)
        seen = [(0, 0, 0)]
        for k in range(1, 4):
            ctx.fuse_frames(list(range(N)), poses)
            seen.append(_info(ctx))
            if k >= 2:
                assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), _ref(w, h, ONCE * k, dims, origin)), k
        nbytes = ctx.class_cache_info()[3]
    print("info per pass:", seen, "bytes", nbytes)
    for k in range(1, 4):
        d = tuple(a - b for a, b in zip(seen[k], seen[k - 1]))
        assert d == ((N, 0, 0) if (k == 1 or not cache) else (0, N, 0)), (k, seen)
    assert nbytes > 0 if cache else nbytes == 0


@pytest.mark.parametrize("wh", SIZES)
def test_key_changes(wh):
    """One slot, one entry: a pose one ulp off, another scale, other depth limits (through count_bricks) and a new image under the
    same pose are misses, and so is every return to the first key after one of them; the same key twice in a row is a replay."""
    w, h = wh
    _, frames = _frames(w, h)
    p, pu = _pose(w, h, 0), _pose(w, h, 0, "ulp")
    plan = []
    with _ctx(w, h) as ctx:
        ctx.upload(0, frames[0])

        def step(kind, scale, expect):
            before = _info(ctx)
            ctx.integrate(0, _pose(w, h, 0, kind), scale)
            plan.append((0, kind, scale))
            after = _info(ctx)
            assert tuple(a - b for a, b in zip(after, before)) == expect, (len(plan), before, after)

        miss, hit = (1, 0, 0), (0, 1, 0)
        step("o", 1.0, miss)
        step("o", 1.0, hit)
        step("ulp", 1.0, miss)
        step("ulp", 1.0, hit)
        step("o", 1.0, miss)
        step("o", 1.25, miss)
        step("o", 1.0, miss)
        step("o", 1.0, hit)
        g1 = ctx.download_grid(tl3d.CH_TSDF)
        plan1 = tuple(plan)
        before = _info(ctx)
        ctx.count_bricks(_spec(), [0], [p], centroid_subsample=0, max_depth=1.3)        # other limits: tiles and classes anew
        assert tuple(a - b for a, b in zip(_info(ctx), before)) == miss
        step("o", 1.0, miss)
        step("o", 1.0, hit)
        g2 = ctx.download_grid(tl3d.CH_TSDF)
        plan2 = tuple(plan)
        ctx.upload(0, frames[2])                          # a new image under the same pose
        before = _info(ctx)
        ctx.integrate(0, p, 1.0)
        assert tuple(a - b for a, b in zip(_info(ctx), before)) == miss
        g3 = ctx.download_grid(tl3d.CH_TSDF)
    assert not (np.array(p[1]) == np.array(pu[1])).all()
    assert np.array_equal(g1, _ref(w, h, plan1))
    assert np.array_equal(g2, _ref(w, h, plan2))
    orc = _orc(w, h)
    for i, kind, sc in plan2:
        orc.tsdf_integrate(frames[i], *_pose(w, h, i, kind), scale=sc)
    orc.tsdf_integrate(frames[2], *p, scale=1.0)
    assert np.array_equal(g3, orc.tsdf)
    assert not np.array_equal(g3, _ref(w, h, plan2 + ((0, "o", 1.0),))), "the new image must matter"


@pytest.mark.parametrize("wh", SIZES)
def test_geometry_changes(wh):
    """The same frames and poses into grids of the same dims at another origin and at another voxel offset, then the grids in
    turn as the blocks of a lattice are: every change of grid is a miss for every frame, every grid is the oracle's."""
    w, h = wh
    poses, frames = _frames(w, h)
    o2 = (ORIGIN[0] + 3 * VOX, ORIGIN[1], ORIGIN[2] - 5 * VOX)
    off = (8, 0, 16)
    grids = {"a": (_spec(), ORIGIN), "b": (_spec(origin=o2), o2),
             "c": (_spec(voxel_offset=off), tuple(ORIGIN[k] + off[k] * VOX for k in range(3)))}
    with _ctx(w, h, grid=None) as ctx:
        for i, d in enumerate(frames):
            ctx.upload(i, d)
        for n, name in enumerate("abcacbb", 1):
            spec, oo = grids[name]
            ctx.attach_grid(spec)
            ctx.fuse_frames(list(range(N)), poses)
            g = ctx.download_grid(tl3d.CH_TSDF)
            ctx.detach_grid()
            assert np.array_equal(g, _ref(w, h, ONCE, DIMS, oo)), (n, name)
            # (the last attach meets the grid of the one before it: the only replays)
            assert _info(ctx) == ((N * n, 0, 0) if n < 7 else (N * 6, N, 0)), (n, name)
    assert not np.array_equal(_ref(w, h, ONCE, DIMS, grids["a"][1]), _ref(w, h, ONCE, DIMS, grids["c"][1]))


@pytest.mark.parametrize("wh", SIZES)
def test_count_then_fuse(wh):
    """The count fills level 1 (lists); the fusion into a sparse grid of exactly that size replays it, adds the sub-brick masks
    and equals the oracle; after reset() a second fusion replays level 2 and takes its pool slots again."""
    w, h = wh
    with _ctx(w, h, cache=False, grid=None) as off:
        poses = _upload_all(off, w, h)
        want = off.count_bricks(_spec(), list(range(N)), poses, centroid_subsample=0)
        assert _info(off) == (N, 0, 0)
    with _ctx(w, h, grid=None) as ctx:
        _upload_all(ctx, w, h)
        got = ctx.count_bricks(_spec(), list(range(N)), poses, centroid_subsample=0)
        assert got == want and got[0] > 0
        assert _info(ctx) == (N, 0, 0)
        ctx.attach_grid(_spec(pool_tsdf=got[0]))
        ctx.fuse_frames(list(range(N)), poses)
        g1 = ctx.download_grid(tl3d.CH_TSDF)
        s1 = ctx.stats()
        assert _info(ctx) == (N, N, 0)
        ctx.reset()
        ctx.fuse_frames(list(range(N)), poses)
        g2 = ctx.download_grid(tl3d.CH_TSDF)
        s2 = ctx.stats()
        assert _info(ctx) == (N, 2 * N, 0)
        again = ctx.count_bricks(_spec(), list(range(N)), poses, centroid_subsample=0)     # level 2 serves a count as well
        assert again == want and _info(ctx) == (N, 3 * N, 0)
    for s in (s1, s2):
        assert s["pool_refused"] == 0 and s["pool_slots_tsdf"] == got[0]
    assert np.array_equal(g1, _ref(w, h, ONCE))
    assert np.array_equal(g2, _ref(w, h, ONCE))


@pytest.mark.parametrize("wh", SIZES)
def test_mixed_batches(wh):
    """Replays and classifications in one chain; one slot twice in a batch with one pose (complete entry: both replay; no entry: the
    first saves, the second is classified) and with two poses (one of them is served)."""
    w, h = wh
    poses, _ = _frames(w, h)
    plan = []

    def fuse(ctx, items, expect):
        before = _info(ctx)
        ctx.fuse_frames([i for i, _ in items], [_pose(w, h, i, kind) for i, kind in items])
        plan.extend((i, kind, 1.0) for i, kind in items)
        after = _info(ctx)
        assert tuple(a - b for a, b in zip(after, before)) == expect, (items, before, after)

    with _ctx(w, h) as ctx:
        _upload_all(ctx, w, h)
        fuse(ctx, [(0, "o"), (1, "o"), (2, "o")], (3, 0, 0))
        fuse(ctx, [(i, "o") for i in range(N)], (2, 3, 0))
        fuse(ctx, [(0, "o"), (0, "o")], (0, 2, 0))
        fuse(ctx, [(1, "o"), (1, "alt")], (1, 1, 0))
        fuse(ctx, [(1, "o"), (2, "o")], (0, 2, 0))                      # (the entry of slot 1 is still the first pose's)
        fuse(ctx, [(3, "alt"), (3, "alt")], (2, 0, 0))
        fuse(ctx, [(3, "alt"), (4, "o"), (3, "o")], (1, 2, 0))
        g = ctx.download_grid(tl3d.CH_TSDF)
    assert np.array_equal(g, _ref(w, h, tuple(plan)))


@pytest.mark.parametrize("wh", SIZES)
def test_overflow(wh):
    """A buffer of one entry holds no frame: nothing is ever replayed, every classification is counted as overflowed, the grid is exact."""
    w, h = wh
    with _ctx(w, h, entries=1) as ctx:
        poses = _upload_all(ctx, w, h)
        for _ in range(3):
            ctx.fuse_frames(list(range(N)), poses)
            ctx.sync()
        g = ctx.download_grid(tl3d.CH_TSDF)
        assert _info(ctx) == (3 * N, 0, 3 * N)
    assert np.array_equal(g, _ref(w, h, ONCE * 3))


def _flight_plan():
    """70 integrates cycling over the five slots; a slot keeps a pose for two visits, then takes the other: every second visit saves over
    the entry the visit before it replayed."""
    return tuple((i % N, ("o", "alt")[(i // (2 * N)) % 2], 1.0) for i in range(70))


@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("pairing", [True, False])
@pytest.mark.parametrize("wh", SIZES)
def test_rewrites_beside_readers(wh, pairing, cache):
    """Saves over entries that earlier batches replay, no host wait in between: three batches with every slot several times in
    each, or 70 one-frame batches in turn over the prep streams; the oracle's grid, twice over in one process."""
    w, h = wh
    plan = _flight_plan()
    ref = _ref(w, h, plan)
    with _ctx(w, h, cache=cache) as ctx:
        _upload_all(ctx, w, h)
        ctx.set_tsdf_pairing(pairing)
        for rep in range(2):
            if rep:
                ctx.reset()
            for i, kind, sc in plan:
                ctx.integrate(i, _pose(w, h, i, kind), sc)
            assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), ref), (pairing, cache, rep)
        c, r, o = _info(ctx)
    assert c + r == 2 * len(plan) and o == 0
    assert (r > 0) if cache else (r == 0)


@pytest.mark.parametrize("wh", SIZES)
def test_stats_of_a_replayed_pass(wh):
    """Counting mode: bricks visited and free, records read and written of a replayed pass are those of the classified pass."""
    w, h = wh
    keys = ("tsdf_bricks_visited", "tsdf_bricks_free", "tsdf_records_read", "tsdf_records_written")
    with _ctx(w, h) as ctx:
        poses = _upload_all(ctx, w, h)
        ctx.set_profile(count_records=True)
        got = []
        for _ in range(2):
            ctx.reset()
            ctx.reset_stats()
            ctx.fuse_frames(list(range(N)), poses)
            ctx.sync()
            s = ctx.stats()
            got.append(tuple(s[k] for k in keys))
        assert _info(ctx) == (N, N, 0)
    print(dict(zip(keys, got[0])))
    assert got[0] == got[1] and all(v > 0 for v in got[0])


def test_u16_frames():
    w, h = SIZES[0]
    poses, frames = _frames(w, h)
    orc = _orc(w, h)
    with _ctx(w, h) as ctx:
        for i, d in enumerate(frames):
            mm = np.clip(np.rint(d * 1000.0), 0, 65535).astype(np.uint16)
            ctx.upload(i, mm)
            for _ in range(2):
                orc.tsdf_integrate(mm.astype(np.float32) / np.float32(1000.0), *poses[i])
        for _ in range(2):
            ctx.fuse_frames(list(range(N)), poses)
            ctx.sync()
        g = ctx.download_grid(tl3d.CH_TSDF)
        assert _info(ctx) == (N, N, 0)
    assert np.array_equal(g, orc.tsdf)


def test_one_frame_per_launch():
    w, h = SIZES[1]
    with _ctx(w, h) as ctx:
        poses = _upload_all(ctx, w, h)
        ctx.set_tsdf_pairing(False)
        for _ in range(2):
            ctx.fuse_frames(list(range(N)), poses)
        g = ctx.download_grid(tl3d.CH_TSDF)
        assert _info(ctx) == (N, N, 0)
    assert np.array_equal(g, _ref(w, h, ONCE * 2))
