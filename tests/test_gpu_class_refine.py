"""The first fusion batch that replays a slot's classification entry (and holds the slot once) refines its sub-brick masks by the
update's own per-voxel tile test (tl3d.h: tl3d_class_refine_info; kernels_tsdf.hip: class_refine_kernel) and leaves the entry at
level 3.  Whatever the refinement does, the grid stays the C oracle's bit for bit; on the crafted frames of class_refine_common the
counters are what the numpy model (class_refine_reference, pinned by tests/test_class_refine_reference_cpu.py) says they must be.

Shapes: camera A and the one-brick grid of prep_classes_common for the crafted frames; the five orbit frames, the 64^3 grid and the
ragged 9 x 8 x 11-brick grid of test_gpu_class_cache.py for everything about keys, chains and streams."""
import functools
import os

import numpy as np
import pytest

import tl3d
from oracle import c_oracle

import class_refine_common as cc
from test_class_refine_reference_cpu import TABLE
from test_gpu_class_cache import GRIDS, N, ONCE, SIZES, _cam, _frames, _orc, _pose, _ref, _spec, _upload_all

pytestmark = pytest.mark.gpu

CASES = cc.cases()
KEYS = ("seen", "dropped", "free", "both")


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


def _env(refine=True, class_cache=True, tile_cache=True):
    """the switches are read when the context is created"""
    return {"TL3D_CLASS_REFINE": None if refine else "0", "TL3D_CLASS_CACHE": None if class_cache else "0",
            "TL3D_TILE_CACHE": None if tile_cache else "0", "TL3D_CLASS_CACHE_ENTRIES": None}


def _crafted_ctx(s, n_slots=1, grid=True, **kw):
    spec = tl3d.GridSpec(s.dims, s.origin, s.voxel, s.trunc, tl3d.CH_TSDF) if grid is True else grid
    return _with_env(_env(**kw), lambda: tl3d.FusionContext(s.W, s.H, s.fx, s.fy, s.cx, s.cy, min_depth=s.mind, max_depth=s.maxd,
                                                            n_slots=n_slots, grid=spec))


def _orbit_ctx(w, h, grid="default", **kw):
    c = _cam(w, h)
    return _with_env(_env(**kw), lambda: tl3d.FusionContext(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], n_slots=N,
                                                            grid=_spec() if grid == "default" else grid))


@functools.lru_cache(maxsize=None)
def _crafted_oracle(name):
    """the C oracle's grid of one crafted frame (read-only, shared)"""
    case = next(c for c in CASES if c.name == name)
    s = case.s
    orc = c_oracle.Oracle(s.W, s.H, s.fx, s.fy, s.cx, s.cy, min_depth=s.mind, max_depth=s.maxd, dims=s.dims, origin=s.origin,
                          voxel_size=s.voxel, sdf_trunc=s.trunc)
    orc.tsdf_integrate(case.depth, *case.pose, 1.0)
    g = orc.tsdf.copy()
    g.setflags(write=False)
    return g


def _refined(ctx):
    """(seen, dropped, free, both kinds, masks that did not fit) -- and what must hold between them"""
    r = ctx.class_refine_info()
    assert r[0] >= r[1] + r[2] + r[3] and r[4] == 0, r
    return r


def _delta(a, b):
    return tuple(x - y for x, y in zip(a, b))


# ---- 2. frames that reach each class, one at a time (and 1., three passes of one frame) -------------------------------------------
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_crafted_frame_three_passes(case, u16):
    """The first pass saves (level 2), the second refines, the third replays level 3: three times the oracle's grid; the refine
    counters move in the second pass only, by exactly what the model counts: the pairs left open are the model's open pairs, the
    others are dropped, FREE or decided with both kinds of lane as the model says."""
    seen, opn, dropped, free, both = TABLE[case.name]
    want = _crafted_oracle(case.name)
    with _crafted_ctx(case.s) as ctx:
        ctx.upload(0, case.u16 if u16 else case.depth)
        moved = []
        for k in range(3):
            if k:
                ctx.reset()
            c0, r0 = ctx.class_cache_info()[:2], _refined(ctx)
            ctx.integrate(0, case.pose)
            g = ctx.download_grid(tl3d.CH_TSDF)
            assert np.array_equal(g, want), (k, int((g != want).any(axis=1).sum()))
            assert _delta(ctx.class_cache_info()[:2], c0) == ((1, 0) if k == 0 else (0, 1)), k
            moved.append(_delta(_refined(ctx), r0))
    print(case.name, "refine counters per pass:", moved)
    assert moved[0] == (0, 0, 0, 0, 0) and moved[2] == (0, 0, 0, 0, 0), moved
    got = dict(zip(KEYS, moved[1]))
    assert got["seen"] - got["dropped"] - got["free"] - got["both"] == opn, (got, TABLE[case.name])
    assert got == dict(seen=seen, dropped=dropped, free=free, both=both), (got, TABLE[case.name])


def test_every_class_is_counted():
    """all crafted frames through one context: every class's counter ends above zero (nothing passes by refining nothing)"""
    s = CASES[0].s
    with _crafted_ctx(s, n_slots=len(CASES)) as ctx:
        for i, c in enumerate(CASES):
            ctx.upload(i, c.depth)
        for _ in range(3):                                  # save, then eight entries per chain are refined
            ctx.reset()
            ctx.fuse_frames(list(range(len(CASES))), [c.pose for c in CASES])
        r = _refined(ctx)
    tot = tuple(int(x) for x in np.sum([TABLE[c.name] for c in CASES], axis=0))
    assert all(v > 0 for v in r[:4]), r
    assert r[:4] == (tot[0], tot[2], tot[3], tot[4]) and r[0] - r[1] - r[2] - r[3] == tot[1], (r, tot)


def _total(cs):
    t = np.sum([TABLE[c.name] for c in cs], axis=0) if cs else np.zeros(5, int)
    return (int(t[0]), int(t[2]), int(t[3]), int(t[4]), 0)


def test_a_chain_refines_eight_frames():
    """Twenty slots in one batch: the second pass refines the first eight, the third the next eight, the fourth the last four, the
    fifth none; the grid is the oracle's every time."""
    s = CASES[0].s
    frames = [CASES[i % len(CASES)] for i in range(20)]
    want = np.zeros_like(_crafted_oracle(CASES[0].name))
    for c in frames:
        want = want + _crafted_oracle(c.name)
    with _crafted_ctx(s, n_slots=len(frames)) as ctx:
        for i, c in enumerate(frames):
            ctx.upload(i, c.depth)
        moved = []
        for k in range(5):
            if k:
                ctx.reset()
            r0 = _refined(ctx)
            ctx.fuse_frames(list(range(len(frames))), [c.pose for c in frames])
            assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), want), k
            moved.append(_delta(_refined(ctx), r0))
        assert ctx.class_cache_info()[:3] == (20, 80, 0)
    assert moved == [(0,) * 5, _total(frames[:8]), _total(frames[8:16]), _total(frames[16:]), (0,) * 5], moved


# ---- 1. three passes in batches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("pairing", [True, False], ids=["batches", "single"])
def test_crafted_batches_three_passes(pairing, sparse, u16):
    """All crafted frames into one grid, in one batch (pairing on) or one launch per frame (off), four times with reset() between:
    the sum of the oracle's grids each time; nothing is refined in the first pass, every frame in the second (one frame per
    chain) or eight per chain in the second and third (one batch), nothing after that."""
    s = CASES[0].s
    want = np.zeros_like(_crafted_oracle(CASES[0].name))
    for c in CASES:
        want = want + _crafted_oracle(c.name)
    slots, poses = list(range(len(CASES))), [c.pose for c in CASES]
    with _crafted_ctx(s, n_slots=len(CASES), grid=None if sparse else True) as ctx:
        for i, c in enumerate(CASES):
            ctx.upload(i, c.u16 if u16 else c.depth)
        if sparse:
            spec = tl3d.GridSpec(s.dims, s.origin, s.voxel, s.trunc, tl3d.CH_TSDF)
            nb = ctx.count_bricks(spec, slots, poses, centroid_subsample=0)[0]
            assert nb == 1
            ctx.attach_grid(tl3d.GridSpec(s.dims, s.origin, s.voxel, s.trunc, tl3d.CH_TSDF, pool_tsdf=nb))
        ctx.set_tsdf_pairing(pairing)
        moved, cls = [], []
        for k in range(4):
            if k:
                ctx.reset()
            c0, r0 = ctx.class_cache_info()[:2], _refined(ctx)
            ctx.fuse_frames(slots, poses)
            g = ctx.download_grid(tl3d.CH_TSDF)
            assert np.array_equal(g, want), (k, int((g != want).any(axis=1).sum()))
            moved.append(_delta(_refined(ctx), r0))
            cls.append(_delta(ctx.class_cache_info()[:2], c0))
        assert ctx.stats()["pool_refused"] == 0
    n = len(CASES)
    # (sparse: the count filled level 1, so the first fusion is a replay that adds the masks: level 1 -> 2, not refined)
    assert cls == ([(0, n)] * 4 if sparse else [(n, 0)] + [(0, n)] * 3), cls
    want_moved = [(0,) * 5, _total(CASES[:8]), _total(CASES[8:]), (0,) * 5] if pairing else [(0,) * 5, _total(CASES), (0,) * 5, (0,) * 5]
    assert moved == want_moved, (moved, want_moved)


@pytest.mark.parametrize("pairing", [True, False], ids=["batches", "single"])
@pytest.mark.parametrize("wh,dims,origin", GRIDS)
def test_orbit_three_passes(wh, dims, origin, pairing):
    """The five orbit frames into the 64^3 and the ragged grid: each pass adds the oracle's frames; the refinement sees pairs and
    decides some of them in the second pass only; classified / replayed move as without it."""
    w, h = wh
    with _orbit_ctx(w, h, grid=_spec(dims, origin)) as ctx:
        poses = _upload_all(ctx, w, h)
        ctx.set_tsdf_pairing(pairing)
        moved = []
        for k in range(1, 4):
            c0, r0 = ctx.class_cache_info()[:3], _refined(ctx)
            ctx.fuse_frames(list(range(N)), poses)
            assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), _ref(w, h, ONCE * k, dims, origin)), k
            assert _delta(ctx.class_cache_info()[:3], c0) == ((N, 0, 0) if k == 1 else (0, N, 0)), k
            moved.append(_delta(_refined(ctx), r0))
    print("refine counters per pass:", moved)
    assert moved[0] == (0,) * 5 and moved[2] == (0,) * 5
    assert moved[1][0] > 0 and moved[1][1] + moved[1][2] > 0, moved


# ---- 4. a slot twice in a chain ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", SIZES)
def test_slot_twice_in_a_chain_is_not_refined(wh):
    w, h = wh
    plan = []

    def fuse(ctx, items):
        c0, r0 = ctx.class_cache_info()[:3], _refined(ctx)
        ctx.fuse_frames([i for i, _ in items], [_pose(w, h, i, kind) for i, kind in items])
        plan.extend((i, kind, 1.0) for i, kind in items)
        return _delta(ctx.class_cache_info()[:3], c0), _delta(_refined(ctx), r0)

    with _orbit_ctx(w, h) as ctx:
        _upload_all(ctx, w, h)
        assert fuse(ctx, [(0, "o"), (1, "o"), (2, "o")]) == ((3, 0, 0), (0,) * 5)
        assert fuse(ctx, [(0, "o"), (0, "o")]) == ((0, 2, 0), (0,) * 5)              # level 2, twice: both replay, nothing refined
        cls, ref = fuse(ctx, [(0, "o"), (3, "o")])                                    # once: slot 0 is refined now, slot 3 saved
        assert cls == (1, 1, 0) and ref[0] > 0, (cls, ref)
        cls, ref = fuse(ctx, [(0, "o"), (0, "o"), (3, "o")])                          # level 3 twice replays; slot 3 is refined
        assert cls == (0, 3, 0) and ref[0] > 0, (cls, ref)
        assert fuse(ctx, [(0, "o"), (3, "o")]) == ((0, 2, 0), (0,) * 5)
        assert fuse(ctx, [(1, "o"), (1, "o")]) == ((0, 2, 0), (0,) * 5)              # slot 1 is still at level 2
        cls, ref = fuse(ctx, [(1, "o")])
        assert cls == (0, 1, 0) and ref[0] > 0, (cls, ref)
        g = ctx.download_grid(tl3d.CH_TSDF)
    assert np.array_equal(g, _ref(w, h, tuple(plan)))


# ---- 5. key change, new image, tile-key change --------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", SIZES)
def test_key_changes_fall_back_to_a_save(wh):
    """One slot: a new key (pose one ulp off, another scale: new tiles too) or a new image is a save; the replay after it refines
    again; the one after that replays level 3.  The grid is the oracle's throughout."""
    w, h = wh
    _, frames = _frames(w, h)
    plan = []
    with _orbit_ctx(w, h) as ctx:
        ctx.upload(0, frames[0])

        def step(kind, scale, cls, refines):
            c0, r0 = ctx.class_cache_info()[:3], _refined(ctx)
            ctx.integrate(0, _pose(w, h, 0, kind), scale)
            plan.append((0, kind, scale))
            assert _delta(ctx.class_cache_info()[:3], c0) == cls, (len(plan), kind, scale)
            d = _delta(_refined(ctx), r0)
            assert (d[0] > 0) if refines else (d == (0,) * 5), (len(plan), kind, scale, d)

        miss, hit = (1, 0, 0), (0, 1, 0)
        for kind, scale in (("o", 1.0), ("ulp", 1.0), ("o", 1.0), ("o", 1.25), ("o", 1.0)):
            step(kind, scale, miss, False)
            step(kind, scale, hit, True)
            step(kind, scale, hit, False)
        g1 = ctx.download_grid(tl3d.CH_TSDF)
        plan1 = tuple(plan)
        ctx.upload(0, frames[2])                              # a new image under the same pose
        for cls, refines in ((miss, False), (hit, True), (hit, False)):
            c0, r0 = ctx.class_cache_info()[:3], _refined(ctx)
            ctx.integrate(0, _pose(w, h, 0), 1.0)
            assert _delta(ctx.class_cache_info()[:3], c0) == cls
            d = _delta(_refined(ctx), r0)
            assert (d[0] > 0) if refines else (d == (0,) * 5), d
        g2 = ctx.download_grid(tl3d.CH_TSDF)
    assert np.array_equal(g1, _ref(w, h, plan1))
    orc = _orc(w, h)
    for i, kind, sc in plan1:
        orc.tsdf_integrate(frames[i], *_pose(w, h, i, kind), scale=sc)
    for _ in range(3):
        orc.tsdf_integrate(frames[2], *_pose(w, h, 0), scale=1.0)
    assert np.array_equal(g2, orc.tsdf)


# ---- 6. rewrites beside readers ----------------------------------------------------------------------------------------------------------
def _flight_plan3():
    """70 integrates cycling over the five slots; a slot keeps a pose for THREE visits (save, refine, replay), then takes the other"""
    return tuple((i % N, ("o", "alt")[(i // (3 * N)) % 2], 1.0) for i in range(70))


@pytest.mark.parametrize("pairing", [True, False])
@pytest.mark.parametrize("wh", SIZES)
def test_refinements_beside_readers(wh, pairing):
    """Refinements land between replays of other slots on the other prep streams, no host wait in between; twice over in one
    process: the oracle's grid."""
    w, h = wh
    plan = _flight_plan3()
    ref = _ref(w, h, plan)
    with _orbit_ctx(w, h) as ctx:
        _upload_all(ctx, w, h)
        ctx.set_tsdf_pairing(pairing)
        for rep in range(2):
            if rep:
                ctx.reset()
            for i, kind, sc in plan:
                ctx.integrate(i, _pose(w, h, i, kind), sc)
            assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), ref), (pairing, rep)
        c, r, o = ctx.class_cache_info()[:3]
        seen = _refined(ctx)[0]
    assert c + r == 2 * len(plan) and o == 0 and r > 0
    if not pairing:
        assert seen > 0                       # (one frame per chain: the second visit of a pose refines)


# ---- 7. counting mode -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wh", SIZES)
def test_stats_of_refined_passes(wh):
    """Counting mode: bricks visited and free, records read and written of the refining pass and of a level-3 replay are those of
    the classifying pass."""
    w, h = wh
    keys = ("tsdf_bricks_visited", "tsdf_bricks_free", "tsdf_records_read", "tsdf_records_written")
    with _orbit_ctx(w, h) as ctx:
        poses = _upload_all(ctx, w, h)
        ctx.set_profile(count_records=True)
        got, seen = [], []
        for _ in range(3):
            ctx.reset()
            ctx.reset_stats()
            ctx.fuse_frames(list(range(N)), poses)
            ctx.sync()
            s = ctx.stats()
            got.append(tuple(s[k] for k in keys))
            seen.append(_refined(ctx)[0])
    print(dict(zip(keys, got[0])), seen)
    assert got[0] == got[1] == got[2] and all(v > 0 for v in got[0])
    assert seen[0] == 0 and seen[1] > 0 and seen[2] == seen[1]


# ---- 8. the switch ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", ["TL3D_CLASS_REFINE", "TL3D_CLASS_CACHE", "TL3D_TILE_CACHE"])
def test_switched_off_nothing_is_refined(off):
    w, h = SIZES[0]
    kw = {"TL3D_CLASS_REFINE": dict(refine=False), "TL3D_CLASS_CACHE": dict(class_cache=False), "TL3D_TILE_CACHE": dict(tile_cache=False)}[off]
    with _orbit_ctx(w, h, **kw) as ctx:
        poses = _upload_all(ctx, w, h)
        for k in range(1, 4):
            ctx.fuse_frames(list(range(N)), poses)
            assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), _ref(w, h, ONCE * k)), k
        assert ctx.class_refine_info() == (0, 0, 0, 0, 0)
        assert ctx.class_cache_info()[:3] == ((N, 2 * N, 0) if off == "TL3D_CLASS_REFINE" else (3 * N, 0, 0))
    s = CASES[0].s
    with _crafted_ctx(s, **kw) as ctx:
        ctx.upload(0, CASES[0].depth)
        for _ in range(3):
            ctx.reset()
            ctx.integrate(0, CASES[0].pose)
            assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), _crafted_oracle(CASES[0].name))
        assert ctx.class_refine_info() == (0, 0, 0, 0, 0)
