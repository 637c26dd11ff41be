"""The multi-GPU merge primitives (csrc/kernels_grid.hip: max_weight_kernel, max_weight_dense_kernel, touched_bricks_kernel<SUB>,
brick_rows_kernel<MODE, IS_TSDF, SUB>; the entry points tl3d_grid_max_weight, _touched_bricks, _pack_bricks, _unpack_bricks and the
sparse forms of tl3d_grid_add / _upload / _download) on crafted grids against the integer model of grid_merge_common.py.

Nothing is integrated: contents go in with upload_grid, pending free-space counts through grid_tensor(CH_FREE), so a result depends
on these kernels alone.  Every comparison is np.array_equal against the model -- which knows the layout from the documentation,
not from the kernels' address arithmetic, so an addressing error that pack and unpack share cannot cancel.

Which test reaches which kernel (brick_rows_kernel<MODE, IS_TSDF, SUB> as R<m, t, s>):
  R<0,*,0> / R<1,*,0> with an id list   test_pack_bricks / test_unpack_bricks [whole]     (more rows than workgroups: the big TSDF grid)
  R<0,*,1> / R<1,*,1>                   the same [sub]; more rows than workgroups: test_rows_beyond_the_workgroup_cap
  R<0,*,0> / R<1,*,0> without a list    download / upload of every test on the sparse layout
  R<2,*,0>                              test_sparse_add_*, test_add_headroom_*           (R<2,*,1> is instantiated but no entry point launches it)
  touched_bricks_kernel<false / true>   test_touched_*; second pass of its brick loop: test_big_tsdf_grid_second_pass
  max_weight_kernel                     test_max_weight_placements, test_big_tsdf_grid_second_pass
  max_weight_dense_kernel               test_add_headroom_* (the other grid of tl3d_grid_add; 128^3: beyond its first pass)
"""
import numpy as np
import pytest

import grid_merge_common as gm
from grid_merge_common import CH_CENTROID, CH_TSDF, DIMS, PROBE_POSITIONS, Q

pytestmark = pytest.mark.gpu

BOTH = CH_TSDF | CH_CENTROID
CH_FREE, CH_SUB = 4, 8
LAYOUTS = {"dense": (0, 0), "sparse": (6, 6)}                         # pools per channel (of 16 bricks)
CAM = (64, 48, 60.0, 60.0, 31.5, 23.5)
BIG_TSDF = (256, 256, 136)                                            # 17 408 bricks: more than one pass of the one-wave-per-brick kernels covers


def _imports():
    import torch
    import tl3d
    from tl3d import _cabi as abi
    assert (abi.CH_TSDF, abi.CH_CENTROID, abi.CH_FREE, abi.CH_SUB, abi.TSDF_MAX_WEIGHT) == (CH_TSDF, CH_CENTROID, CH_FREE, CH_SUB, gm.MAX_WEIGHT)
    return torch, tl3d, abi


def to_torch_words(rows):
    """model rows [n, records, words] -> the [n, 32-bit or 64-bit words] block the library takes"""
    import torch
    rows = np.ascontiguousarray(rows)
    flat = rows.reshape(rows.shape[0], -1)
    return torch.from_numpy(flat.view(np.int64) if rows.dtype == np.uint64 else flat)


class Rig:
    """a FusionContext and the model of what it holds, driven together"""

    def __init__(self, dims=DIMS, channels=BOTH, pools=(0, 0)):
        torch, tl3d, abi = _imports()
        self.torch, self.abi = torch, abi
        self.dims, self.channels, self.pools = tuple(dims), channels, tuple(pools)
        spec = tl3d.GridSpec(self.dims, (0.0, 0.0, 0.0), 0.01, 0.04, channels, pool_tsdf=pools[0], pool_centroid=pools[1])
        self.ctx = tl3d.FusionContext(*CAM, n_slots=1, grid=spec)
        self.dev = torch.device("cuda", self.ctx.device)
        self.stream = torch.cuda.ExternalStream(self.ctx.stream_ptr(), device=self.dev)
        self.model = gm.RankState(self.dims, channels, *self.pools)
        self.nbricks = self.model.nbricks

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    def on_stream(self):
        return self.torch.cuda.stream(self.stream)

    def reset(self):
        self.ctx.reset()
        self.model = gm.RankState(self.dims, self.channels, *self.pools)

    def upload(self, channel, image):
        self.ctx.upload_grid(channel, image)
        self.model.load(channel, image)

    def download(self, channel):
        return self.ctx.download_grid(channel), self.model.image(channel)

    def set_counts(self, counts):
        c = np.zeros(self.nbricks, np.uint32)
        if isinstance(counts, dict):
            for b, n in counts.items():
                c[b] = n
        else:
            c[:] = counts
        with self.on_stream():
            self.ctx.grid_tensor(CH_FREE).copy_(self.torch.from_numpy(c.view(np.int32)))
            self.stream.synchronize()
        self.model.free[:] = c

    def counts(self):
        with self.on_stream():
            return self.ctx.grid_tensor(CH_FREE).cpu().numpy().view(np.uint32).copy()

    def touched(self, flags, pre=None):
        """(map the library leaves, map the model leaves), both starting from `pre` (default zeros)"""
        sub = bool(flags & CH_SUB)
        host = np.zeros(self.nbricks * (8 if sub else 1), np.uint8) if pre is None else pre.copy()
        with self.on_stream():
            m = self.torch.from_numpy(host.copy()).to(self.dev)
            self.ctx.touched_bricks(m, flags)
            got = m.cpu().numpy()
        return got, self.model.touched(host, flags & BOTH, free_apart=bool(flags & CH_FREE), sub=sub)

    def _ids(self, ids):
        return self.torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(self.dev)

    def pack(self, flags, ids):
        """(rows the library packs, rows the model packs) as [n, 512 or 64, words]"""
        channel, sub = flags & BOTH, bool(flags & CH_SUB)
        words = (64 if sub else 512) * gm.WORDS[channel]
        with self.on_stream():
            block = self.torch.full((len(ids), words), -1, dtype=self.torch.int32 if channel == CH_TSDF else self.torch.int64, device=self.dev)
            self.ctx.pack_bricks(flags, self._ids(ids), block)
            got = block.cpu().numpy()
        got = got.view(gm.DTYPE[channel]).reshape(len(ids), -1, gm.WORDS[channel])
        return got, self.model.pack(channel, ids, free_apart=bool(flags & CH_FREE), sub=sub)

    def unpack(self, flags, ids, rows):
        channel, sub = flags & BOTH, bool(flags & CH_SUB)
        with self.on_stream():
            self.ctx.unpack_bricks(flags, self._ids(ids), to_torch_words(rows).to(self.dev))
            self.stream.synchronize()
        self.model.unpack(channel, ids, rows, free_apart=bool(flags & CH_FREE), sub=sub)

    def add(self, channel, image):
        self.ctx.add_grid(channel, image)
        self.model.add(channel, image)

    def pool_figures(self):
        """(slots in use of the channels behind a brick table, refusals): library, model"""
        st = self.ctx.stats()
        behind = [c for c in (CH_TSDF, CH_CENTROID) if self.channels & c and self.model.cap[c] < self.nbricks]
        name = {CH_TSDF: "pool_slots_tsdf", CH_CENTROID: "pool_slots_centroid"}
        return ([st[name[c]] for c in behind], st["pool_refused"]), ([self.model.n_slots(c) for c in behind], self.model.refused)

    def assert_same(self):
        """everything a host can read back: both channels' images (this folds, on both sides), the counts, the pool figures"""
        for c in (CH_TSDF, CH_CENTROID):
            if self.channels & c:
                got, want = self.download(c)
                assert np.array_equal(got, want), "channel %d differs from the model in %d records" % (c, int((got != want).any(axis=1).sum()))
        if self.channels & CH_TSDF:
            assert np.array_equal(self.counts(), self.model.free)
        if self.model.sparse:
            got, want = self.pool_figures()
            assert got == want
        self.model.check()


def sentinel(channel, nvox):
    """a record-dependent pattern with a non-zero weight / count everywhere: what must survive where a call has no business"""
    i = np.arange(nvox, dtype=np.int64)
    if channel == CH_TSDF:
        return np.stack([-(i + 1), 0x01000000 + i], axis=1).astype(np.int32)
    u = i.astype(np.uint64)
    return np.stack([u | np.uint64(0xa5 << 56), ((u + np.uint64(1)) << np.uint64(32)) | np.uint64(0x5a), ~u, u * np.uint64(3)], axis=1)


def in_bricks(image, bricks):
    out = np.zeros_like(image)
    for b in bricks:
        out[512 * b:512 * b + 512] = image[512 * b:512 * b + 512]
    return out


# ---- touched_bricks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_touched_probes_mark_exactly_their_brick_and_sub_brick(layout):
    """one record with nothing but a weight (a count) at each probe position of the first, a middle (index = 3 mod 4) and the last
    brick: per channel and with mask 0, per brick and per sub-brick.  Exactly the one expected byte appears next to a byte set
    beforehand (the call ORs), and nothing when the other channel alone is asked for."""
    with Rig(pools=LAYOUTS[layout]) as rig:
        for channel in (CH_TSDF, CH_CENTROID):
            other = BOTH & ~channel
            for brick in gm.probe_bricks(rig.nbricks):
                for pos in PROBE_POSITIONS:
                    rig.reset()
                    rig.upload(channel, gm.probe(channel, rig.model.nvox, 512 * brick + pos))
                    for sub in (0, CH_SUB):
                        target = 8 * brick + pos // 64 if sub else brick
                        pre = np.zeros(rig.nbricks * (8 if sub else 1), np.uint8)
                        pre[(target + 5) % len(pre)] = 1
                        for mask in (channel, 0, channel | CH_FREE):
                            got, want = rig.touched(mask | sub, pre)
                            assert np.array_equal(got, want), (channel, brick, pos, sub, mask)
                            assert sorted(np.nonzero(got)[0]) == sorted([target, (target + 5) % len(pre)]) and got[target] == 1
                        got, want = rig.touched(other | sub, pre)
                        assert np.array_equal(got, want) and np.array_equal(got, pre), (channel, brick, pos, sub)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_touched_count_only_bricks_with_and_without_the_counts_apart(layout):
    with Rig(pools=LAYOUTS[layout]) as rig:
        rig.upload(CH_TSDF, gm.copy_image(CH_TSDF, rig.model, [1, 2], seed=1, sub_bricks={1: [0, 3], 2: [7]}))
        counts = {4: 3, 12: 1, 15: 65536, 1: 2}                       # 4, 12, 15: nothing but a count; 1: a count next to records
        rig.set_counts(counts)
        for flags in (CH_TSDF | CH_FREE, CH_TSDF | CH_FREE | CH_SUB, CH_FREE, CH_FREE | CH_SUB):
            got, want = rig.touched(flags)
            assert np.array_equal(got, want)
            per_brick = got.reshape(rig.nbricks, -1)
            assert not per_brick[[4, 12, 15]].any() and per_brick[1].any() and per_brick[2].any()
            assert np.array_equal(rig.counts(), rig.model.free) and rig.counts()[15] == 65536       # pending counts stayed pending
        got, want = rig.touched(CH_TSDF | CH_SUB)                     # counts not apart: folded first
        assert np.array_equal(got, want)
        if layout == "dense":
            assert got.reshape(rig.nbricks, 8)[[1, 4, 12, 15]].all() and not rig.counts().any()
        else:                                                         # a brick without records keeps its count and marks nothing
            assert not got.reshape(rig.nbricks, 8)[[4, 12, 15]].any()
            assert rig.counts().tolist() == [counts.get(b, 0) if b != 1 else 0 for b in range(rig.nbricks)]
        got, want = rig.touched(CH_TSDF)
        assert np.array_equal(got, want) and np.array_equal(rig.counts(), rig.model.free)
        rig.assert_same()


@pytest.mark.parametrize("channel", [CH_TSDF, CH_CENTROID])
def test_touched_on_a_sparse_grid_skips_bricks_without_a_slot_and_bricks_a_full_pool_refused(channel):
    with Rig(pools=(2, 2)) as rig:
        img = gm.copy_image(channel, rig.model, [3, 5, 6], seed=2)
        rig.upload(channel, in_bricks(img, [3, 5]))                   # the pool is full now
        rig.unpack(channel, [6], img.reshape(rig.nbricks, 512, -1)[[6]])          # one row, one refusal: nothing races
        assert rig.pool_figures() == (([2, 0] if channel == CH_TSDF else [0, 2], 1),) * 2
        for flags in (channel, channel | CH_SUB, 0, CH_SUB):
            got, want = rig.touched(flags)
            assert np.array_equal(got, want)
            assert sorted(np.nonzero(got.reshape(rig.nbricks, -1).any(axis=1))[0]) == [3, 5]
        rig.assert_same()


# ---- pack_bricks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("unit", ["whole", "sub"])
@pytest.mark.parametrize("channel", [CH_TSDF, CH_CENTROID])
def test_pack_bricks_rows_are_the_models_slices_of_the_uploaded_image(channel, unit, layout):
    sub = CH_SUB if unit == "sub" else 0
    n = 64 if sub else 512
    with Rig(pools=LAYOUTS[layout]) as rig:
        img = gm.copy_image(channel, rig.model, [1, 7, 15], seed=5, sub_bricks={7: [1, 6]})
        rig.upload(channel, img)
        # ascending, not contiguous; bricks with records, without (no slot on the sparse layout), partly filled
        ids = [0, 8, 9, 15, 57, 58, 62, 63, 64, 120, 126, 127] if sub else [0, 1, 4, 7, 14, 15]
        for lst in (ids, ids[1:2], ids[-1:], ids[2:]):
            got, want = rig.pack(channel | sub, lst)
            assert np.array_equal(got, want)
            for row, i in zip(got, lst):
                assert np.array_equal(row, img[n * i:n * i + n])     # id 8 b + s <-> records [512 b + 64 s, + 64) = [64 id, + 64)
        rig.assert_same()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("unit", ["whole", "sub"])
def test_pack_bricks_with_pending_counts_records_alone_or_the_fold(unit, layout):
    sub = CH_SUB if unit == "sub" else 0
    with Rig(pools=LAYOUTS[layout]) as rig:
        t = np.zeros((rig.model.nvox, 2), np.int32)
        for b in (1, 7):
            for pos in PROBE_POSITIONS:
                t[512 * b + pos] = (-Q * (pos + 1), pos + 1)
        rig.upload(CH_TSDF, t)
        rig.set_counts({1: 5, 4: 2, 15: 1})
        ids = [8, 9, 15, 32, 39, 56, 63, 120, 127] if sub else [1, 4, 7, 15]
        k4 = ids.index(32 if sub else 4)                              # a row of brick 4, which holds nothing but a count
        got, want = rig.pack(CH_TSDF | CH_FREE | sub, ids)
        assert np.array_equal(got, want) and np.array_equal(rig.counts(), rig.model.free) and rig.counts()[1] == 5
        assert got[0][0].tolist() == [-Q, 1] and not got[k4].any()                     # the records alone
        got, want = rig.pack(CH_TSDF | sub, ids)
        assert np.array_equal(got, want) and np.array_equal(rig.counts(), rig.model.free)
        assert got[0][0].tolist() == [4 * Q, 6] and got[0][2].tolist() == [5 * Q, 5]  # brick 1: record + 5 observations of free space
        if layout == "dense":
            assert (got[k4] == (2 * Q, 2)).all() and not rig.counts().any()             # brick 4: the fold of its count
        else:
            assert not got[k4].any() and rig.counts()[4] == 2                           # no records: zeros, the count stays pending
        rig.assert_same()


def test_pack_and_unpack_of_no_rows_with_null_pointers_do_nothing():
    with Rig() as rig:
        img = gm.copy_image(CH_TSDF, rig.model, [2], seed=6)
        rig.upload(CH_TSDF, img)
        lib, h = rig.ctx._lib, rig.ctx._h
        for flags in (CH_TSDF, CH_TSDF | CH_SUB, CH_CENTROID | CH_SUB, CH_TSDF | CH_FREE):
            assert lib.tl3d_grid_pack_bricks(h, flags, None, 0, None) == 0
            assert lib.tl3d_grid_unpack_bricks(h, flags, None, 0, None) == 0
        rig.assert_same()


# ---- unpack_bricks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("unit", ["whole", "sub"])
@pytest.mark.parametrize("channel", [CH_TSDF, CH_CENTROID])
def test_unpack_bricks_sets_the_listed_rows_and_nothing_else(channel, unit, layout):
    """into a grid full of a sentinel (sparse layout: four bricks of it, which is what the pool leaves room for next to the arrivals):
    the listed rows become the block -- set, not added --, every other record keeps the sentinel, no neighbouring sub-brick moves;
    a sparse grid draws a slot exactly for the bricks without one that receive a non-zero row"""
    sub = CH_SUB if unit == "sub" else 0
    with Rig(pools=LAYOUTS[layout]) as rig:
        sent = sentinel(channel, rig.model.nvox)
        if layout == "sparse":
            sent = in_bricks(sent, [1, 2, 7, 15])
        rig.upload(channel, sent)
        src = gm.copy_image(channel, rig.model, [1, 5, 9, 15], seed=7, sub_bricks={9: [2]})
        n = 64 if sub else 512
        # rows over the sentinel (1, 15), rows of zeros over the sentinel (2), arrivals in bricks without a slot (5, 9), zeros there (12)
        ids = [8, 15, 17, 40, 47, 74, 75, 96, 126, 127] if sub else [1, 2, 5, 9, 12, 15]
        rows = src.reshape(-1, n, gm.WORDS[channel])[ids]
        before = rig.pool_figures()[0]
        rig.unpack(channel | sub, ids, rows)
        got, want = rig.download(channel)
        assert np.array_equal(got, want)
        expect = sent.copy()
        for i in ids:
            expect[n * i:n * i + n] = src[n * i:n * i + n]
        assert np.array_equal(got, expect)
        if layout == "sparse":
            after = rig.pool_figures()[0]
            assert sum(after[0]) - sum(before[0]) == 2 and after[1] == 0              # bricks 5 and 9; not 12 (zeros)
        rig.assert_same()


@pytest.mark.parametrize("unit", ["whole", "sub"])
@pytest.mark.parametrize("channel", [CH_TSDF, CH_CENTROID])
def test_unpack_bricks_with_the_pool_one_slot_short_refuses_counts_and_keeps_the_rest_exact(channel, unit):
    sub = CH_SUB if unit == "sub" else 0
    n = 64 if sub else 512
    with Rig(pools=(3, 3)) as rig:
        src = gm.copy_image(channel, rig.model, [1, 2, 5, 9], seed=8)
        rows = src.reshape(-1, n, gm.WORDS[channel])
        rig.upload(channel, in_bricks(sentinel(channel, rig.model.nvox), [1, 2]))
        first = [8, 41, 46] if sub else [1, 5]                        # brick 5 takes the last slot
        rig.unpack(channel | sub, first, rows[first])
        assert rig.pool_figures()[0] == rig.pool_figures()[1] and rig.pool_figures()[0][1] == 0
        second = [17, 40, 72, 79, 96] if sub else [2, 5, 9, 12]       # brick 9 (both its rows) is refused, once; 12 receives zeros
        rig.unpack(channel | sub, second, rows[second])
        got, want = rig.pool_figures()
        assert got == want and got[1] == 1
        got, want = rig.download(channel)
        assert np.array_equal(got, want) and not got[512 * 9:512 * 10].any()
        for i in first + second:
            if (i >> 3 if sub else i) != 9:
                assert np.array_equal(got[n * i:n * i + n], src[n * i:n * i + n])
        rig.assert_same()


@pytest.mark.parametrize("channel", [CH_TSDF, CH_CENTROID])
def test_rows_beyond_the_workgroup_cap(channel):
    """128^3: 32 768 sub-brick rows, of which four in five are listed -- more rows than brick_rows_kernel gets workgroups, so the
    later rows are reached by its stride loop; packed from one grid against the image, unpacked into a second one full of a sentinel"""
    dims = (128, 128, 128)
    rng = np.random.default_rng(9)
    with Rig(dims, channels=channel) as src, Rig(dims, channels=channel) as dst:
        nvox = src.model.nvox
        img = gm.random_records(channel, nvox, rng)
        img.reshape(-1, 64, gm.WORDS[channel])[rng.random(nvox // 64) < 0.3] = 0
        src.upload(channel, img)
        ids = np.nonzero(np.arange(nvox // 64) % 5 != 0)[0]
        assert len(ids) > 16384
        got, want = src.pack(channel | CH_SUB, ids)
        assert np.array_equal(got, want) and np.array_equal(got, img.reshape(-1, 64, gm.WORDS[channel])[ids])
        sent = sentinel(channel, nvox)
        dst.upload(channel, sent)
        dst.unpack(channel | CH_SUB, ids, got)
        expect = sent.reshape(-1, 64, gm.WORDS[channel]).copy()
        expect[ids] = got
        got, want = dst.download(channel)
        assert np.array_equal(got, want) and np.array_equal(got, expect.reshape(nvox, -1))


# ---- grid_add on a sparse grid (brick_rows_kernel MODE 2) -----------------------------------------------------------------------
@pytest.mark.parametrize("channel", [CH_TSDF, CH_CENTROID])
def test_sparse_add_equals_the_dense_add_and_the_model_on_the_carry_cases(channel):
    """TSDF sums that pass zero (a 64-bit lane would carry into the weight) and the int32 extremes at the weight limit; centroid words
    whose low halves sum past 2^32 (a 32-bit lane would drop the carry), counts up to 2^20.  The grid holds bricks the image lacks
    and the other way round; on the sparse layout the latter draw their slots on receipt."""
    a, b = gm.add_images(channel, DIMS[0] * DIMS[1] * DIMS[2], [1, 2, 7], [1, 5, 7])
    results = []
    for layout in LAYOUTS:
        with Rig(pools=LAYOUTS[layout]) as rig:
            rig.upload(channel, a)
            if channel == CH_TSDF:
                rig.set_counts({2: 4, 9: 6})                          # fold before the sum (brick 2); stay pending without records (sparse: 9)
            rig.add(channel, b)                                       # TSDF: 40 000 + 25 536 observations: exactly the limit, accepted
            got, want = rig.download(channel)
            assert np.array_equal(got, want)
            results.append(got)
            rig.assert_same()
    assert np.array_equal(results[0], results[1])
    wrong = gm.add_i32_in_64bit_lanes(a, b) if channel == CH_TSDF else gm.add_u64_in_32bit_lanes(a, b)
    crafted = np.zeros(len(a), bool)
    crafted[512:1024] = crafted[512 * 7:512 * 8] = True               # (no counts in bricks 1 and 7)
    assert (results[0][crafted] != wrong[crafted]).any(axis=1).sum() >= 10
    if channel == CH_TSDF:
        assert results[0][:, 0].min() == -2147418112 and results[0][:, 1].max() == gm.MAX_WEIGHT


# ---- headroom ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_max_weight_placements(layout):
    """the maximum in either half of a 16-byte record pair, in the last record of the last brick, in a brick that adds a pending
    count to its records, in a brick that holds nothing but a count -- each against a lower weight in the other places"""
    with Rig(pools=LAYOUTS[layout]) as rig:
        nvox = rig.model.nvox
        for records, counts, expect in (
                ({512 * 9 + 16: 7, 512 * 9 + 17: 6, nvox - 1: 5}, {}, 7),              # .y of the int4
                ({512 * 9 + 16: 6, 512 * 9 + 17: 7, nvox - 1: 5}, {}, 7),              # .w of the int4
                ({512 * 9 + 16: 6, 512 * 9 + 17: 5, nvox - 1: 7}, {}, 7),              # last record of the last brick
                ({512 * 9 + 16: 7, 512 * 3 + 255: 5}, {3: 3, 9: 0}, 8),                # record + pending count beats the largest record
                ({512 * 9 + 16: 7, 512 * 3 + 255: 5}, {3: 3, 12: 9}, 9),               # a count-only brick (sparse: it has no records at all)
                ({512 * 9 + 16: 7}, {15: 65536}, 65536),
                ({}, {}, 0)):
            rig.reset()
            t = np.zeros((nvox, 2), np.int32)
            for rec, w in records.items():
                t[rec] = (-Q * w, w)
            rig.upload(CH_TSDF, t)
            rig.set_counts(counts)
            assert rig.ctx.max_weight() == rig.model.max_weight() == expect
            assert np.array_equal(rig.counts(), rig.model.free)                       # measuring folds nothing
        rig.assert_same()


@pytest.mark.parametrize("layout", ["dense", "sparse"])
def test_big_tsdf_grid_second_pass(layout):
    """17 408 bricks: max_weight_kernel and touched_bricks_kernel launch 4096 workgroups of four waves, so bricks from 16 384 on are
    reached by the second trip of their loops; the probes sit there.  On the sparse layout the upload and the download go through
    brick_rows_kernel without an id list, 17 408 rows for 16 384 workgroups."""
    with Rig(BIG_TSDF, channels=CH_TSDF, pools=(64, 0) if layout == "sparse" else (0, 0)) as rig:
        nvox, nbr = rig.model.nvox, rig.nbricks
        assert nbr > 16384 + 8
        bricks = gm.probe_bricks(nbr, first=16384)
        t = np.zeros((nvox, 2), np.int32)
        t[512 * 100 + 5] = (0, 3)                                      # first pass: a lower weight
        for n, (b, pos) in enumerate(zip(bricks, (1, 64, 511))):
            t[512 * b + pos] = (-Q * (10 + n), 10 + n)                 # the maximum: last record of the last brick, an odd record
        rig.upload(CH_TSDF, t)
        assert rig.ctx.max_weight() == rig.model.max_weight() == 12
        rig.set_counts({bricks[1]: 5, 16385: 2})
        assert rig.ctx.max_weight() == rig.model.max_weight() == 16
        for flags in (CH_TSDF | CH_FREE, CH_TSDF | CH_FREE | CH_SUB):
            got, want = rig.touched(flags)
            assert np.array_equal(got, want)
            unit = 8 if flags & CH_SUB else 1
            assert sorted(np.nonzero(got)[0]) == sorted([100 * unit] + [b * unit + (pos // 64 if unit == 8 else 0) for b, pos in zip(bricks, (1, 64, 511))])
        ids = np.arange(nbr)                                            # whole-brick rows, more of them than workgroups
        got, want = rig.pack(CH_TSDF | CH_FREE, ids)
        assert np.array_equal(got, want) and np.array_equal(got.reshape(nvox, 2), t)
        rig.assert_same()


@pytest.mark.parametrize("layout", ["dense", "sparse"])
def test_add_headroom_is_exact_at_the_limit_and_a_refusal_changes_nothing(layout):
    """128^3: the other grid of tl3d_grid_add is measured by max_weight_dense_kernel, 2048 workgroups x 256 lanes x 2 records per
    trip, so its last record is found in the second trip and in the .w half.  One observation past TL3D_TSDF_MAX_WEIGHT: E_STATE and
    the grid as it was; exactly at the limit: accepted and summed."""
    dims = (128, 128, 128)
    _, tl3d, abi = _imports()
    with Rig(dims, channels=CH_TSDF, pools=(40, 0) if layout == "sparse" else (0, 0)) as rig:
        nvox = rig.model.nvox
        assert nvox // 2 > 2048 * 256
        t = np.zeros((nvox, 2), np.int32)
        t[512 * 3000 + 17] = (Q * 30000, 30000)
        t[512 * 3000 + 18] = (-Q * 200, 200)
        rig.upload(CH_TSDF, t)
        rig.set_counts({3000: 7, 11: 2})                                # own maximum: record + count = 30 007
        o = np.zeros((nvox, 2), np.int32)
        o[12] = (Q * 35000, 35000)                                      # first trip, .y half: not the maximum
        o[nvox - 1] = (-Q * (gm.MAX_WEIGHT - 30007 + 1), gm.MAX_WEIGHT - 30007 + 1)
        with pytest.raises(tl3d.Tl3dError) as err:
            rig.ctx.add_grid(CH_TSDF, o)
        assert err.value.code == abi.E_STATE
        with pytest.raises(gm.HeadroomError):
            rig.model.add(CH_TSDF, o)
        got, want = rig.download(CH_TSDF)
        assert np.array_equal(got, want) and got[512 * 3000 + 17].tolist() == [Q * 30007, 30007] and not got[nvox - 1].any()
        o[nvox - 1] = (-Q * (gm.MAX_WEIGHT - 30007), gm.MAX_WEIGHT - 30007)
        o[512 * 3000 + 17] = (-Q * 5, 5)
        rig.add(CH_TSDF, o)
        got, want = rig.download(CH_TSDF)
        assert np.array_equal(got, want) and got[nvox - 1, 1] == gm.MAX_WEIGHT - 30007 and got[512 * 3000 + 17].tolist() == [Q * 30002, 30012]
        rig.assert_same()


# ---- three simulated ranks -----------------------------------------------------------------------------------------------------
def _rank_rigs(layout, ranks=(0, 1, 2)):
    rigs = []
    for r in ranks:
        rig = Rig(pools=gm.RANK_POOLS if layout == "sparse" else (0, 0))
        t, c, counts = gm.rank_inputs(r)
        rig.upload(CH_TSDF, t)
        rig.upload(CH_CENTROID, c)
        rig.set_counts(counts)
        rigs.append(rig)
    return rigs


@pytest.mark.parametrize("layout", LAYOUTS)
def test_three_simulated_ranks_merge_to_the_model_and_to_the_plain_sum(layout):
    """one process, three contexts, no process group: the primitives in the order allreduce_context_grids calls them (the counts, the
    sub-brick maps, pack / unpack with CH_FREE | CH_SUB), every collective a torch sum or maximum over the three device tensors.
    Every rank ends with the model's merge, which is also rank 0 after add_grid of the other ranks' downloads."""
    torch, _, _ = _imports()
    rigs = _rank_rigs(layout)
    plain = _rank_rigs(layout)
    try:
        models = [r.model for r in rigs]
        nbr = rigs[0].nbricks

        def settle():                                                  # three streams and torch's own: nothing overlaps.  (Not ctx.sync():
            torch.cuda.synchronize()                                   # tl3d_sync folds the pending counts, the merge must not.)

        assert sum(r.ctx.max_weight() for r in rigs) == sum(m.max_weight() for m in gm.rank_states(layout == "sparse")) <= gm.MAX_WEIGHT
        cnts = [r.ctx.grid_tensor(CH_FREE) for r in rigs]
        settle()
        total = cnts[0] + cnts[1] + cnts[2]
        for c in cnts:
            c.copy_(total)
        settle()
        sent = {}
        for channel, words, dt in ((CH_TSDF, 128, torch.int32), (CH_CENTROID, 256, torch.int64)):
            chf = channel | (CH_FREE if channel == CH_TSDF else 0)
            maps = [torch.zeros(8 * nbr, dtype=torch.uint8, device=r.dev) for r in rigs]
            settle()
            for r, m in zip(rigs, maps):
                r.ctx.touched_bricks(m, chf | CH_SUB)
            settle()
            idx = torch.nonzero(torch.stack(maps).max(dim=0).values, as_tuple=False).flatten().to(torch.int32)
            assert 0 < idx.numel() < 4 * nbr
            blocks = [torch.empty((idx.numel(), words), dtype=dt, device=r.dev) for r in rigs]
            settle()
            for r, b in zip(rigs, blocks):
                r.ctx.pack_bricks(chf | CH_SUB, idx, b)
            settle()
            block = blocks[0] + blocks[1] + blocks[2]
            settle()
            for r in rigs:
                r.ctx.unpack_bricks(chf | CH_SUB, idx, block)
            settle()
            sent[channel] = idx.cpu().numpy()
        trace = []
        gm.merge(models, sparse=True, trace=trace)
        assert np.array_equal(sent[CH_TSDF], np.nonzero(np.maximum.reduce(trace[2][1]))[0])
        assert np.array_equal(sent[CH_CENTROID], np.nonzero(np.maximum.reduce(trace[4][1]))[0])
        want = gm.python_sum_of_folded_images(gm.rank_states(layout == "sparse"))
        for r in rigs:
            assert np.array_equal(r.counts(), r.model.free)            # the summed counts (pending where the brick has no records)
            r.assert_same()
            assert np.array_equal(r.model.image(CH_TSDF), want[CH_TSDF]) and np.array_equal(r.model.image(CH_CENTROID), want[CH_CENTROID])
        # the same scan merged the plain way: rank 0 += what ranks 1 and 2 download
        for other in plain[1:]:
            for channel in (CH_TSDF, CH_CENTROID):
                plain[0].add(channel, other.ctx.download_grid(channel))
        for channel in (CH_TSDF, CH_CENTROID):
            assert np.array_equal(plain[0].ctx.download_grid(channel), want[channel])
        plain[0].assert_same()
    finally:
        for r in rigs + plain:
            r.ctx.close()


class ScriptedPeers:
    """torch.distributed as ONE rank of three sees it, the two peers played by the model: every all_reduce first checks what this
    rank puts in against the model's figure for it, then hands back the model's reduction over all three"""

    class ReduceOp:
        SUM, MAX = "sum", "max"

    def __init__(self, rank, trace):
        self.rank, self.trace, self.k = rank, trace, 0

    def is_initialized(self):
        return True

    def get_world_size(self):
        return 3

    def get_rank(self):
        return self.rank

    def get_backend(self):
        return "nccl"

    def all_reduce(self, t, op="sum"):
        import torch
        kind, parts = self.trace[self.k]
        assert kind == op, (self.k, kind, op)
        own = t.detach().cpu().numpy()
        mine = np.ascontiguousarray(parts[self.rank])
        assert own.nbytes == mine.nbytes and own.tobytes() == mine.tobytes(), "collective %d: this rank's contribution differs from the model's" % self.k
        if op == "max":
            out = np.maximum.reduce(parts)
        elif own.dtype.itemsize == 8 and own.size > 1:
            out = gm.sum_rows(CH_CENTROID, [np.ascontiguousarray(p).view(np.uint64) for p in parts])
        elif own.dtype.itemsize == 8:
            out = sum(np.asarray(p, np.int64) for p in parts)
        else:
            out = gm.sum_rows(CH_TSDF, [np.ascontiguousarray(p).view(np.int32) for p in parts])
        t.copy_(torch.from_numpy(np.ascontiguousarray(out).view(own.dtype).reshape(own.shape)))
        self.k += 1


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("path", ["rows", "whole_channel"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_allreduce_context_grids_as_one_rank_of_three(layout, path, rank):
    """tl3d.distributed.allreduce_context_grids itself, on one rank whose peers are the model: each of its collectives carries what
    the model says this rank contributes, and with the model's reductions handed back the rank ends with the sum of the three folded
    images.  whole_channel (sparse=False): the summed free-space counts enter the TSDF sum once, not once per rank."""
    from tl3d.distributed import allreduce_context_grids
    models = gm.rank_states(layout == "sparse")
    trace = []
    gm.merge(models, sparse=path == "rows", trace=trace)
    want = gm.python_sum_of_folded_images(gm.rank_states(layout == "sparse"))
    rig = _rank_rigs(layout, ranks=(rank,))[0]
    with rig:
        peers = ScriptedPeers(rank, trace)
        info = allreduce_context_grids(rig.ctx, peers, sparse=path == "rows")
        assert peers.k == len(trace) and info["bricks_total"] == rig.nbricks
        rig.model = models[rank]
        rig.assert_same()
        for channel in (CH_TSDF, CH_CENTROID):
            assert np.array_equal(rig.ctx.download_grid(channel), want[channel])


# ---- argument refusals (host-side checks: none of these reaches the device) ------------------------------------------------------
def test_argument_refusals_leave_the_grid_and_the_map_alone():
    torch, tl3d, abi = _imports()
    with Rig(channels=CH_TSDF) as rig:
        img = gm.copy_image(CH_TSDF, rig.model, [1, 15], seed=10)
        rig.upload(CH_TSDF, img)
        nbr = rig.nbricks
        dev = rig.dev

        def refused(code, fn, *args):
            with pytest.raises(tl3d.Tl3dError) as err:
                fn(*args)
            assert err.value.code == code, err.value

        with rig.on_stream():
            for n, flags in ((nbr + 1, CH_TSDF), (nbr - 1, CH_TSDF), (nbr, CH_TSDF | CH_SUB), (8 * nbr, CH_TSDF), (8 * nbr + 8, CH_SUB)):
                m = torch.zeros(n, dtype=torch.uint8, device=dev)
                refused(abi.E_INVALID, rig.ctx.touched_bricks, m, flags)               # a map of the wrong length
                assert not m.cpu().numpy().any()
            host_map = np.zeros(nbr, np.uint8)
            refused(abi.E_INVALID, rig.ctx.touched_bricks, host_map, CH_TSDF)          # a host pointer as the map
            assert not host_map.any()
            m = torch.zeros(nbr, dtype=torch.uint8, device=dev)
            refused(abi.E_STATE, rig.ctx.touched_bricks, m, CH_CENTROID)               # a channel the grid lacks
            refused(abi.E_STATE, rig.ctx.touched_bricks, m, BOTH)
            refused(abi.E_INVALID, rig.ctx.touched_bricks, m, 16)
            assert not m.cpu().numpy().any()
            ids = torch.tensor([1, 15], dtype=torch.int32, device=dev)
            block = torch.full((2, 1024), -1, dtype=torch.int32, device=dev)
            cblock = torch.full((2, 2048), -1, dtype=torch.int64, device=dev)
            for fn in (rig.ctx.pack_bricks, rig.ctx.unpack_bricks):
                refused(abi.E_INVALID, fn, CH_TSDF, np.array([1, 15], np.int32), block)          # a host pointer as the id list
                refused(abi.E_INVALID, fn, CH_TSDF, ids, np.full((2, 1024), -1, np.int32))       # ... as the block
                refused(abi.E_STATE, fn, CH_CENTROID, ids, cblock)
                refused(abi.E_INVALID, fn, BOTH, ids, block)                                     # exactly one channel
            # more rows than the grid has (the list itself is never read: the count alone refuses)
            many = torch.zeros(nbr + 1, dtype=torch.int32, device=dev)
            refused(abi.E_INVALID, rig.ctx.pack_bricks, CH_TSDF, many, torch.empty((nbr + 1, 1024), dtype=torch.int32, device=dev))
            many = torch.zeros(8 * nbr + 1, dtype=torch.int32, device=dev)
            refused(abi.E_INVALID, rig.ctx.pack_bricks, CH_TSDF | CH_SUB, many, torch.empty((8 * nbr + 1, 128), dtype=torch.int32, device=dev))
            assert (block.cpu().numpy() == -1).all()
        rig.assert_same()
