"""The TSDF update's pair loop at every trip count: the batches of tests/update_trip_counts_common.py (one frame fused 1 ... 14 times
in a batch, on a grid of 3 x 3 x 3 bricks whose bricks hold 0 to 8 MIXED sub-bricks) against the C oracle, bit for bit -- f32 and
16-bit frames, dense and sparse grids, 32 frames per launch and one, counting mode, and three passes over resident frames, whose
replayed and refined masks give the bricks other pair counts.  tests/test_update_trip_counts_reference_cpu.py shows which loop
paths these batches take."""
import functools

import numpy as np
import pytest

import tl3d
from oracle import c_oracle

import update_trip_counts_common as tc

pytestmark = pytest.mark.gpu

NS = tuple(range(1, tc.N_MAX + 1))
NBRICKS = (tc.DIMS[0] // 8) * (tc.DIMS[1] // 8) * (tc.DIMS[2] // 8)


@functools.lru_cache(maxsize=None)
def _refs(name, passes=1):
    """{n: the oracle's grid after the image was fused n * passes times} (read-only, shared)"""
    c = tc.CAM
    orc = c_oracle.Oracle(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], min_depth=tc.MIND, max_depth=tc.MAXD, dims=tc.DIMS,
                          origin=tc.ORIGIN, voxel_size=tc.VOX, sdf_trunc=tc.TRUNC)
    out, done = {}, 0
    for n in NS:
        while done < n * passes:
            orc.tsdf_integrate(tc.image_f32(name), *tc.POSE)
            done += 1
        g = orc.tsdf.copy()
        g.setflags(write=False)
        out[n] = g
    return out


def _ctx(sparse=False):
    c = tc.CAM
    kw = dict(pool_tsdf=NBRICKS) if sparse else {}
    spec = tl3d.GridSpec(tc.DIMS, tc.ORIGIN, tc.VOX, tc.TRUNC, tl3d.CH_TSDF, **kw)
    return tl3d.FusionContext(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], min_depth=tc.MIND, max_depth=tc.MAXD,
                              n_slots=tc.N_MAX, grid=spec)


def _upload(ctx, name, u16):
    img = tc.image_mm(name) if u16 else tc.image_f32(name)
    for i in range(tc.N_MAX):
        ctx.upload(i, img)


def _same(got, want, what):
    assert np.array_equal(got, want), (what, int((got != want).any(axis=-1).sum()))


@pytest.mark.parametrize("pairing", [True, False], ids=["batched", "one_per_launch"])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_every_trip_count_against_the_oracle(u16, sparse, pairing):
    with _ctx(sparse) as ctx:
        ctx.set_tsdf_pairing(pairing)
        for name in tc.IMAGES:
            refs = _refs(name)
            assert refs[1].any()
            _upload(ctx, name, u16)
            for n in NS:
                ctx.reset()
                ctx.reset_stats()
                ctx.fuse_frames(list(range(n)), [tc.POSE] * n)
                _same(ctx.download_grid(tl3d.CH_TSDF), refs[n], (name, n))
                assert ctx.stats()["tsdf_launches"] == (1 if pairing else n)


def _bricks_all_free(grid, n):
    """bricks of the oracle's grid whose 512 records are all n observations of tsdf = 1: what a frame may have listed as free space"""
    b = grid.reshape(tc.DIMS[2] // 8, 8, tc.DIMS[1] // 8, 8, tc.DIMS[0] // 8, 8, 2)
    full = (b[..., 0] == 32767 * n) & (b[..., 1] == n)
    return int(full.all(axis=(1, 3, 5)).sum())


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_counting_mode_counts_the_records_that_change(u16):
    """One batch on a fresh grid reads and writes every record it changes once.  The records that change are the oracle's records
    with a weight, less the 512 of every brick the frames listed as free space whole: those are counted per brick and folded in
    later, not read and written by the update (and can only be bricks the oracle fills with tsdf = 1 throughout)."""
    with _ctx() as ctx:
        ctx.set_profile(count_records=True)
        for name in tc.IMAGES:
            refs = _refs(name)
            _upload(ctx, name, u16)
            for n in NS:
                ctx.reset()
                ctx.reset_stats()
                ctx.fuse_frames(list(range(n)), [tc.POSE] * n)
                _same(ctx.download_grid(tl3d.CH_TSDF), refs[n], (name, n))
                st = ctx.stats()
                free, rest = divmod(st["tsdf_bricks_free"], n)
                assert rest == 0 and free <= _bricks_all_free(refs[n], n), (name, n, st["tsdf_bricks_free"])
                changed = int((refs[n][..., 1] != 0).sum()) - 512 * free
                assert st["tsdf_records_read"] == st["tsdf_records_written"] == changed > 0, (name, n)


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_three_passes_over_resident_frames(u16):
    """the second pass replays the frames' cached masks and refines them, the third replays the refined ones: bricks lose the pairs
    the tiles decide whole, and the loop runs at other trip counts"""
    with _ctx() as ctx:
        for name in tc.IMAGES:
            _upload(ctx, name, u16)
            for n in NS:
                ctx.reset()
                for k in (1, 2, 3):
                    ctx.fuse_frames(list(range(n)), [tc.POSE] * n)
                    _same(ctx.download_grid(tl3d.CH_TSDF), _refs(name, passes=k)[n], (name, n, k))
