"""The TSDF prep's brick and sub-brick classes on crafted frames (prep_classes_common): every frame holds ONE pixel that alone
decides whether a brick / sub-brick may be skipped or called free space, placed under each level of the tile pyramid the
classifiers can reach, in ragged tiles, at the ends of the lookup windows and at the image border.

SOUNDNESS  a classifier that misses the pixel writes (+32767, +1) on -- or leaves out -- the voxel over it: the downloaded TSDF
           channel is compared bit for bit with the C oracle's, one frame at a time and in batches, dense and sparse, paired
           or not, with the tile and the class cache on and off, classified and replayed, from f32 and from 16-bit uploads.
TIGHTNESS  counting mode, one frame per launch: the bricks the fusion visits are at most, and the bricks it calls free at least,
           what the model of prep_classes_reference says (its answers under every perturbation a robust case survives).  On the
           one-brick cases that is "free == 1 without the pixel, free == 0 and visited == 1 with it": the tile that holds the
           pixel was looked at.  A tighter classifier still passes, a looser one fails.
tests/test_prep_classes_reference_cpu.py shows on the CPU that the cases are decisive and robust and which model fault each catches.
"""
import functools
import os

import numpy as np
import pytest

import tl3d
import prep_classes_common as pc
import prep_classes_reference as pr
from oracle import c_oracle

pytestmark = pytest.mark.gpu

ALL = pc.all_cases()
GROUPS = {}                                       # cases that share camera and grid: one context, one batch sequence
for _c in ALL:
    GROUPS.setdefault(f"{_c.cam}_{_c.s.dims[0]}", []).append(_c)


def _ids(cases):
    return [c.name for c in cases]


def _spec(s, **kw):
    return tl3d.GridSpec(s.dims, s.origin, s.voxel, s.trunc, tl3d.CH_TSDF, **kw)


def _ctx(s, n_slots=1, grid=True, tile_cache=True, class_cache=True):
    """A FusionContext; the caches are switched off through the environment, which is read when the context is created."""
    want = {"TL3D_TILE_CACHE": None if tile_cache else "0", "TL3D_CLASS_CACHE": None if class_cache else "0"}
    old = {k: os.environ.get(k) for k in want}
    for k, v in want.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return tl3d.FusionContext(s.W, s.H, s.fx, s.fy, s.cx, s.cy, min_depth=s.mind, max_depth=s.maxd, n_slots=n_slots,
                                  grid=_spec(s) if grid else None)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _oracle(name, planted):
    """the C oracle's grid of the case's frame (read-only, shared)"""
    case = next(c for c in ALL if c.name == name)
    s = case.s
    orc = c_oracle.Oracle(s.W, s.H, s.fx, s.fy, s.cx, s.cy, min_depth=s.mind, max_depth=s.maxd, dims=s.dims, origin=s.origin,
                          voxel_size=s.voxel, sdf_trunc=s.trunc)
    orc.tsdf_integrate(case.depth if planted else case.base, *case.pose, 1.0)
    g = orc.tsdf.copy()
    g.setflags(write=False)
    return g


def _image(case, planted, u16):
    if u16:
        return case.u16 if planted else case.u16_base
    return case.depth if planted else case.base


def _target_records(case):
    """records of the case's target brick / sub-brick"""
    nbx, nby, _ = case.s.nb
    b = ((case.brick[2] * nby + case.brick[1]) * nbx + case.brick[0]) * 512
    return slice(b, b + 512) if case.sub is None else slice(b + 64 * case.sub, b + 64 * case.sub + 64)


# ---- one frame at a time ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_single_frame(case, u16):
    """The image WITHOUT the decisive pixel goes into the slot first, then the image with it into the same slot: the tiles and the
    classes have to be made anew.  A third fusion after reset() replays the cached classes."""
    with _ctx(case.s) as ctx:
        ctx.upload(0, _image(case, False, u16))
        ctx.integrate(0, case.pose)
        assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), _oracle(case.name, False)), "without the pixel"
        for replay in (False, True):
            ctx.reset()
            if not replay:
                ctx.upload(0, _image(case, True, u16))
            before = ctx.class_cache_info()[:2]
            ctx.integrate(0, case.pose)
            g = ctx.download_grid(tl3d.CH_TSDF)
            want = _oracle(case.name, True)
            assert np.array_equal(g, want), (replay, int((g != want).any(axis=1).sum()))
            after = ctx.class_cache_info()[:2]
            assert (after[0] - before[0], after[1] - before[1]) == ((0, 1) if replay else (1, 0)), (replay, before, after)
    if case.pixel is not None:                     # the frame is decisive for the grid as well: the pixel changes the target's records
        r = _target_records(case)
        assert not np.array_equal(_oracle(case.name, True)[r], _oracle(case.name, False)[r])


# ---- batches -----------------------------------------------------------------------------------------------------------------------------
CACHES = [(True, True), (False, True), (True, False), (False, False)]


@pytest.mark.parametrize("tile_cache,class_cache", CACHES, ids=["caches", "no_tile_cache", "no_class_cache", "no_cache"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_batches(group, sparse, tile_cache, class_cache):
    """All frames of one camera, with and without their pixels, into one grid in batches of up to 32 (pairing on) and one launch
    per frame (off), then once more after reset() (replayed where the class cache is on), f32 and 16-bit: the sum of the
    oracle's grids every time.  Sparse: a pool of exactly the bricks count_bricks announces, all of which the fusion takes (on the
    one-brick grids that is the whole grid; the 125-brick grid of the cell-list cases has bricks without records)."""
    cases = GROUPS[group]
    frames = [(c, p) for c in cases for p in ((True, False) if c.pixel is not None else (True,))]
    want = np.zeros_like(_oracle(cases[0].name, True))
    for c, p in frames:
        want = want + _oracle(c.name, p)
    s = cases[0].s
    slots, poses = list(range(len(frames))), [c.pose for c, _ in frames]
    with _ctx(s, n_slots=len(frames), grid=not sparse, tile_cache=tile_cache, class_cache=class_cache) as ctx:
        for u16 in (False, True):
            for i, (c, p) in enumerate(frames):
                ctx.upload(i, _image(c, p, u16))
            if sparse and not u16:
                nt, _ = ctx.count_bricks(_spec(s), slots, poses, centroid_subsample=0)
                assert 1 <= nt <= s.nb[0] * s.nb[1] * s.nb[2]
                ctx.attach_grid(_spec(s, pool_tsdf=nt))
            for pairing in (True, False):
                ctx.set_tsdf_pairing(pairing)
                for again in (False, True):
                    ctx.reset()
                    ctx.reset_stats()
                    ctx.fuse_frames(slots, poses)
                    g = ctx.download_grid(tl3d.CH_TSDF)
                    assert np.array_equal(g, want), (u16, pairing, again, int((g != want).any(axis=1).sum()))
                    st = ctx.stats()
                    assert st["tsdf_launches"] == ((len(frames) + 31) // 32 if pairing else len(frames))
                    if sparse:
                        assert st["pool_refused"] == 0 and st["pool_slots_tsdf"] == nt, (nt, st["pool_slots_tsdf"], st["pool_refused"])
        classified, replayed, _ = ctx.class_cache_info()[:3]
    # (classes are kept with the tiles they were made from: without the tile cache nothing is replayed)
    assert (replayed > 0) == (class_cache and tile_cache) and classified > 0


# ---- tightness -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_counts(name, planted):
    """(most bricks a classifier as tight as the model visits, fewest it calls free; the model's own visited, free)"""
    case = next(c for c in ALL if c.name == name)
    return pr.robust_counts(case.s, case.depth if planted else case.base, *case.pose)


def measure(ctx, case, planted):
    """counting mode, the frame alone in a launch, into a sparse grid of count_bricks' size:
    (visited, free, count_bricks, pool slots taken, pool refusals)"""
    s = case.s
    ctx.upload(0, _image(case, planted, False))
    nt, _ = ctx.count_bricks(_spec(s), [0], [case.pose], centroid_subsample=0)
    ctx.attach_grid(_spec(s, pool_tsdf=max(1, nt)))
    try:
        ctx.set_profile(count_records=True)
        ctx.set_tsdf_pairing(False)
        ctx.reset_stats()
        ctx.integrate(0, case.pose)
        ctx.sync()
        st = ctx.stats()
        g = ctx.download_grid(tl3d.CH_TSDF)
    finally:
        ctx.detach_grid()
    assert np.array_equal(g, _oracle(case.name, planted))
    return st["tsdf_bricks_visited"], st["tsdf_bricks_free"], nt, st["pool_slots_tsdf"], st["pool_refused"]


def report_line(case, planted, got):
    vis_hi, free_lo, vis, free = model_counts(case.name, planted)
    return (f"{case.name:58s} {'with' if planted else 'without':7s} level {case.level:2d} window {case.window[0]}x{case.window[1]}  "
            f"model visited {vis:3d} free {free:3d} (bounds <= {vis_hi:3d}, >= {free_lo:3d})   GPU visited {got[0]:3d} free {got[1]:3d} "
            f"count_bricks {got[2]:3d} slots {got[3]:3d}")


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_counts_are_within_the_models(case):
    with _ctx(case.s, grid=False) as ctx:
        for planted in ((False, True) if case.pixel is not None else (True,)):
            visited, free, nt, slots, refused = got = measure(ctx, case, planted)
            print(report_line(case, planted, got))
            vis_hi, free_lo, _, _ = model_counts(case.name, planted)
            assert visited <= vis_hi and free >= free_lo, (planted, got, (vis_hi, free_lo))
            # (a pool of as many bricks as the grid has is a dense channel: every brick has its slot from the start)
            nbricks = case.s.nb[0] * case.s.nb[1] * case.s.nb[2]
            assert nt <= vis_hi and slots == (nt if max(1, nt) < nbricks else nbricks) and refused == 0, (planted, got)
            if case.s.nb == (1, 1, 1) and case.pixel is not None:
                # robust cases: the model's answer is the only one there is
                if planted or case.kind == "sub":
                    assert (visited, free, nt) == (1, 0, 1), (planted, got)
                else:
                    assert (visited, free, nt) == ((1, 1, 0) if case.rule != "skip_far" else (0, 0, 0)), (planted, got)
