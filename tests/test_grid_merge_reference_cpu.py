"""The integer model of the merge primitives (grid_merge_common.py) checked on its own: no GPU, no library.  What the GPU tests
compare the kernels with must itself be pinned to something independent -- Python-integer sums, the record geometry of
mesh_reference.record_coords, and inputs that are known to tell a right sum from a wrong one."""
import numpy as np
import pytest

import grid_merge_common as gm
from grid_merge_common import CH_CENTROID, CH_TSDF, Q
from mesh_reference import record_coords


@pytest.mark.parametrize("layout_sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("sparse", [True, False], ids=["rows", "whole_channel"])
def test_merge_of_three_ranks_is_the_python_sum_of_their_folded_images(layout_sparse, sparse):
    want = gm.python_sum_of_folded_images(gm.rank_states(layout_sparse))
    states = gm.rank_states(layout_sparse)
    gm.merge(states, sparse=sparse)
    for s in states:
        s.check()
        assert s.refused == 0
        for channel in (CH_TSDF, CH_CENTROID):
            assert np.array_equal(s.image(channel), want[channel])
    # the inputs do what the issue asks of them: a brick on exactly one rank, on all, on none; count-only bricks on every rank
    held = [set(np.nonzero(s.rec[CH_TSDF][:, 1].reshape(16, 512).any(axis=1))[0]) for s in gm.rank_states(False)]
    assert held[0] & held[1] & held[2] and (held[0] - held[1] - held[2]) and set(range(16)) - (held[0] | held[1] | held[2])
    for r, s in enumerate(gm.rank_states(False)):
        assert set(np.nonzero(s.free)[0]) - held[r], "no count-only brick on rank %d" % r
    assert want[CH_TSDF][512 * 3:512 * 4].any() == 0 and (want[CH_TSDF][512 * 12:512 * 13] == (3 * Q, 3)).all()


def test_whole_channel_merge_counts_free_space_once():
    """Every rank holds the SUMMED counts when the whole-channel path reads the records; were they folded on every rank the sum
    would hold them once per rank.  The model of the sequence without that precaution must differ from the Python sum here,
    or the states could not show the error."""
    want = gm.python_sum_of_folded_images(gm.rank_states(False))
    states = gm.rank_states(False)
    total = sum(s.free.astype(np.int64) for s in states)
    for s in states:
        s.free[:] = total
        s.fold()
    wrong = gm.sum_rows(CH_TSDF, [s.rec[CH_TSDF] for s in states])
    assert not np.array_equal(wrong, want[CH_TSDF])
    assert (wrong[512 * 4:512 * 5] == (3 * 111 * Q, 3 * 111)).all() and (want[CH_TSDF][512 * 4:512 * 5] == (111 * Q, 111)).all()


def test_sub_brick_is_the_4x4x4_cube_of_the_record_geometry():
    """sub-brick s of a brick = records [64 s, 64 s + 64) = the cube (i >> 2) | (j >> 2) << 1 | (k >> 2) << 2 of the brick"""
    dims = (16, 24, 8)
    i, j, k = record_coords(dims)
    idx = np.arange(len(i))
    cube = ((i & 7) >> 2) | (((j & 7) >> 2) << 1) | (((k & 7) >> 2) << 2)
    assert np.array_equal((idx & 511) >> 6, cube)
    brick = (i >> 3) + (dims[0] // 8) * ((j >> 3) + (dims[1] // 8) * (k >> 3))
    assert np.array_equal(idx >> 9, brick)
    # and that is the row the model packs for id 8 b + s: 64 records, 4 x 4 x 4 distinct coordinates inside one cube
    s = gm.RankState(dims, channels=CH_TSDF)
    s.rec[CH_TSDF][:, 1] = idx + 1
    for b, sb in ((0, 0), (2, 5), (5, 7)):
        row = s.pack(CH_TSDF, [8 * b + sb], free_apart=True, sub=True)[0]
        recs = row[:, 1] - 1
        assert len(recs) == 64 and (brick[recs] == b).all() and (cube[recs] == sb).all()
        assert len({(int(i[r]), int(j[r]), int(k[r])) for r in recs}) == 64
        assert np.ptp(i[recs]) == 3 and np.ptp(j[recs]) == 3 and np.ptp(k[recs]) == 3


@pytest.mark.parametrize("channel", [CH_TSDF, CH_CENTROID])
@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("layout_sparse", [False, True])
def test_pack_then_unpack_into_an_empty_state_gives_those_rows_and_nothing_else(channel, sub, layout_sparse):
    pools = dict(pool_tsdf=6, pool_centroid=6) if layout_sparse else {}
    src = gm.RankState(**pools)
    img = gm.copy_image(channel, src, [1, 7, 15], seed=3)
    src.load(channel, img)
    ids = [9, 11, 56, 63, 120, 127] if sub else [1, 4, 15]               # rows with records and rows without (brick 4 / sub-brick 63 of 7 ...)
    rows = src.pack(channel, ids, sub=sub)
    n = 64 if sub else 512
    for row, i in zip(rows, ids):
        assert np.array_equal(row, img[n * i:n * i + n])                  # id 8 b + s -> records [512 b + 64 s, + 64) = [64 id, + 64)
    dst = gm.RankState(**pools)
    dst.unpack(channel, ids, rows, sub=sub)
    want = np.zeros_like(img)
    for i in ids:
        want[n * i:n * i + n] = img[n * i:n * i + n]
    assert np.array_equal(dst.rec[channel], want)
    dst.check()
    if layout_sparse:                                                     # slots only for the bricks that received anything
        assert dst.n_slots(channel) == len({(i >> 3 if sub else i) for i in ids if want[n * i:n * i + n].any()}) and dst.refused == 0


def test_unpack_sets_and_a_full_pool_refuses_once_per_brick():
    s = gm.RankState(pool_tsdf=2, pool_centroid=2)
    img = gm.copy_image(CH_TSDF, s, [3, 5, 6], seed=4)
    rows = img.reshape(-1, 64, 2)
    s.unpack(CH_TSDF, [24, 25, 40], rows[[24, 25, 40]], free_apart=True, sub=True)
    assert s.n_slots(CH_TSDF) == 2 and s.refused == 0
    s.unpack(CH_TSDF, [26, 48, 49, 100], rows[[26, 48, 49, 100]], free_apart=True, sub=True)     # brick 6: refused, counted once; 12: zeros
    assert s.n_slots(CH_TSDF) == 2 and s.refused == 1 and not s.rec[CH_TSDF][512 * 6:512 * 7].any()
    assert np.array_equal(s.rec[CH_TSDF][64 * 26:64 * 27], img[64 * 26:64 * 27])
    s.unpack(CH_TSDF, [24], rows[[40]], free_apart=True, sub=True)                                 # set, not add
    assert np.array_equal(s.rec[CH_TSDF][64 * 24:64 * 25], img[64 * 40:64 * 41])


def test_touched_with_and_without_the_counts_apart():
    for layout_sparse in (False, True):
        s = gm.rank_states(layout_sparse)[0]
        counts = s.free.copy()
        count_only = [4, 5, 12]
        m = s.touched(np.zeros(128, np.uint8), CH_TSDF, free_apart=True, sub=True)
        assert np.array_equal(s.free, counts) and not m.reshape(16, 8)[count_only].any()
        assert set(np.nonzero(m.reshape(16, 8).any(axis=1))[0]) == set(gm.RANK_TSDF_BRICKS[0])
        assert 0 < m.reshape(16, 8)[2].sum() < 8                                  # a surface crosses a few sub-bricks, not all
        pre = np.zeros(16, np.uint8)
        pre[3] = 1                                                                # the call ORs
        m = s.touched(pre, CH_TSDF, free_apart=False)
        if layout_sparse:                                                         # no records: the counts stay pending and mark nothing
            assert set(np.nonzero(m)[0]) == set(gm.RANK_TSDF_BRICKS[0]) | {3} and np.array_equal(s.free[count_only], counts[count_only])
        else:
            assert set(np.nonzero(m)[0]) == set(gm.RANK_TSDF_BRICKS[0]) | {3} | set(count_only) and not s.free.any()
            assert s.touched(np.zeros(128, np.uint8), CH_TSDF, sub=True).reshape(16, 8)[count_only].all()
        assert s.free[1] == 0                                                     # folded into the records of brick 1
        mc = s.touched(np.zeros(16, np.uint8), CH_CENTROID)
        assert set(np.nonzero(mc)[0]) == set(gm.RANK_CENTROID_BRICKS[0])
        m0 = s.touched(np.zeros(16, np.uint8))
        assert np.array_equal(m0, mc | s.touched(np.zeros(16, np.uint8), CH_TSDF))


def test_max_weight_is_records_plus_pending_counts():
    s = gm.RankState(channels=CH_TSDF)
    t = np.zeros((s.nvox, 2), np.int32)
    t[512 * 9 + 17] = (-5 * Q, 5)
    t[8191] = (0, 4)
    s.load(CH_TSDF, t)
    assert s.max_weight() == 5
    s.free[15] = 3
    assert s.max_weight() == 7                                                    # record + count in the last brick
    s.free[2] = 9
    assert s.max_weight() == 9                                                    # a count-only brick
    s.fold()
    assert s.max_weight() == 9 and not s.free.any()


def test_add_wraps_per_lane_and_the_crafted_inputs_tell_the_lane_widths_apart():
    nvox = 16 * 512
    a, b = gm.add_images(CH_TSDF, nvox, [1, 2, 7], [1, 5, 7])
    s = gm.RankState()
    s.load(CH_TSDF, a)
    s.add(CH_TSDF, b)
    right = s.rec[CH_TSDF]
    assert right.tolist() == [[((int(x) + int(y) + (1 << 31)) % (1 << 32)) - (1 << 31) for x, y in zip(ra, rb)] for ra, rb in zip(a.tolist(), b.tolist())]
    assert right[:, 1].max() == gm.MAX_WEIGHT and right[:, 0].min() == -2147418112 and right[:, 0].max() == 2147418112
    wrong = gm.add_i32_in_64bit_lanes(a, b)
    # a < 0 < b with |a| > b stays below zero: no carry leaves the low half, both lane widths agree there ...
    for pa, pb in gm.TSDF_PAIRS_NO_CARRY:
        assert pa < 0 < pb and -pa > pb
        hit = (a[:, 0] == pa) & (b[:, 0] == pb) & (a[:, 1] == 1)
        assert hit.any() and np.array_equal(right[hit], wrong[hit])
    # ... and the pairs that reach zero or add two negative sums carry: the 64-bit lane puts one observation too many into the weight
    for pa, pb in gm.TSDF_PAIRS_CARRY:
        hit = (a[:, 0] == pa) & (b[:, 0] == pb) & (a[:, 1] == 1)
        assert hit.any() and (right[hit, 1] == 2).all() and (wrong[hit, 1] == 3).all() and np.array_equal(right[hit, 0], wrong[hit, 0])

    a, b = gm.add_images(CH_CENTROID, nvox, [1, 2, 7], [1, 5, 7])
    s = gm.RankState()
    s.load(CH_CENTROID, a)
    s.add(CH_CENTROID, b)
    right = s.rec[CH_CENTROID]
    assert right.tolist() == [[(int(x) + int(y)) % (1 << 64) for x, y in zip(ra, rb)] for ra, rb in zip(a.tolist(), b.tolist())]
    wrong = gm.add_u64_in_32bit_lanes(a, b)
    both = (a[:, 1] != 0) & (b[:, 1] != 0)
    assert both.sum() == 16 and (right[both] != wrong[both]).all()                # every word of every crafted record carries
    assert ((right[both, 1] >> np.uint64(32)) == (1 << 20) + 1).all()             # counts 2^20 - 1 - k and 1 + k, plus the carry of the low half
    assert (((a[both, 1] >> np.uint64(32)) + (b[both, 1] >> np.uint64(32))) == 1 << 20).all()


def test_add_refuses_past_the_weight_limit_and_changes_nothing():
    s = gm.RankState(channels=CH_TSDF)
    t = np.zeros((s.nvox, 2), np.int32)
    t[100] = (0, 40000)
    s.load(CH_TSDF, t)
    o = np.zeros_like(t)
    o[8191] = (0, gm.MAX_WEIGHT - 40000 + 1)
    with pytest.raises(gm.HeadroomError):
        s.add(CH_TSDF, o)
    assert np.array_equal(s.rec[CH_TSDF], t)
    o[8191, 1] -= 1
    s.add(CH_TSDF, o)
    assert s.max_weight() == 40000 and s.rec[CH_TSDF][8191, 1] == gm.MAX_WEIGHT - 40000


def test_sparse_add_draws_slots_on_receipt_only_for_rows_that_hold_something():
    s = gm.RankState(pool_tsdf=3, pool_centroid=3)
    a, b = gm.add_images(CH_TSDF, s.nvox, [1, 2], [1, 5])
    s.load(CH_TSDF, a)
    s.free[9] = 6                                                                 # count-only, no slot: stays pending through the add
    assert s.n_slots(CH_TSDF) == 2
    s.add(CH_TSDF, b)
    s.check()
    assert s.n_slots(CH_TSDF) == 3 and s.refused == 0 and s.free[9] == 6
    assert np.array_equal(s.rec[CH_TSDF][512 * 5:512 * 6], b[512 * 5:512 * 6])
    assert (s.image(CH_TSDF)[512 * 9:512 * 10] == (6 * Q, 6)).all()
