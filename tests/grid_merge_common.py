"""Crafted rank states and an integer model of the multi-GPU merge primitives (include/tl3d.h: tl3d_grid_max_weight,
tl3d_grid_touched_bricks, tl3d_grid_pack_bricks / _unpack_bricks, tl3d_grid_add / _upload / _download and the sequence
tl3d.distributed.allreduce_context_grids builds from them), for the CPU and the GPU tests.

numpy and Python integers only, no library: every operation is a slice, a reshape or an elementwise integer operation in int64
with an explicit wrap to the stored width, written from the documented layout and not from the kernels' address arithmetic:

  record order  brick-major; brick b = records [512 b, 512 b + 512); sub-brick s of it = records [512 b + 64 s, + 64)
  TSDF record   int32 {sum of quantised tsdf, weight};  centroid record  uint64 {sx | sy << 32, sz | n << 32, sr | sg << 32, sb}
  free-space    one uint32 count per brick, pending until something reads the TSDF channel: fold = every record of the brick
                += count x (32767, 1).  A brick of a SPARSE grid that holds no records keeps its count; readers add it.
  sparse grid   a channel keeps records for at most `pool` bricks; a brick draws a slot when it first receives a row with a
                non-zero word; with the pool exhausted the row is dropped and the refusal counted (once per brick).

The model hands slots out in ascending row order.  The library hands them out in whatever order its workgroups run, so a test
may exhaust a pool only with a call whose refusals do not depend on that order.
"""
import numpy as np

CH_TSDF, CH_CENTROID = 1, 2
Q = 32767                                               # TL3D_TSDF_QSCALE
MAX_WEIGHT = 65536                                      # TL3D_TSDF_MAX_WEIGHT
M32 = np.uint64(0xffffffff)
S32 = np.uint64(32)

DIMS = (32, 16, 16)                                     # 4 x 2 x 2 = 16 bricks: the default grid of the tests
PROBE_POSITIONS = (0, 1, 63, 64, 127, 128, 510, 511)    # both halves of a 16-byte record pair, the lane 31 / 32 boundary of a wave, both ends
WORDS = {CH_TSDF: 2, CH_CENTROID: 4}
DTYPE = {CH_TSDF: np.int32, CH_CENTROID: np.uint64}


class HeadroomError(Exception):
    """the sum would take a TSDF weight past MAX_WEIGHT: the library refuses with TL3D_E_STATE and changes nothing"""


def wrap_i32(x):
    """int64 values -> what an int32 lane holds after the same sum"""
    x = np.asarray(x, np.int64)
    return (((x + (1 << 31)) & 0xffffffff) - (1 << 31)).astype(np.int32)


def add_u64(a, b):
    """a + b mod 2^64, lane by lane, without ever leaving the range of the type: 32-bit halves and an explicit carry"""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    lo = (a & M32) + (b & M32)
    hi = (a >> S32) + (b >> S32) + (lo >> S32)
    return ((hi & M32) << S32) | (lo & M32)


def add_u64_in_32bit_lanes(a, b):
    """the WRONG centroid sum: every 32-bit half on its own, the carry out of the low half dropped"""
    a, b = np.asarray(a, np.uint64), np.asarray(b, np.uint64)
    return ((((a >> S32) + (b >> S32)) & M32) << S32) | (((a & M32) + (b & M32)) & M32)


def add_i32_in_64bit_lanes(a, b):
    """the WRONG TSDF sum: {sum, weight} added as one uint64 lane, so a carry out of the sum lands in the weight"""
    a64 = np.ascontiguousarray(a, np.int32).view(np.uint32).astype(np.uint64)
    b64 = np.ascontiguousarray(b, np.int32).view(np.uint32).astype(np.uint64)
    s = add_u64(a64[:, 0] | (a64[:, 1] << S32), b64[:, 0] | (b64[:, 1] << S32))
    return np.stack([s & M32, s >> S32], axis=1).astype(np.uint32).view(np.int32)


class RankState:
    """What one rank's grid holds.  Records of a brick without a slot are zero (an invariant, see check())."""

    def __init__(self, dims=DIMS, channels=CH_TSDF | CH_CENTROID, pool_tsdf=0, pool_centroid=0):
        self.dims = tuple(int(d) for d in dims)
        self.nvox = self.dims[0] * self.dims[1] * self.dims[2]
        assert all(d % 8 == 0 for d in self.dims)
        self.nbricks = self.nvox // 512
        self.channels = channels
        self.sparse = bool(pool_tsdf or pool_centroid)
        self.rec = {c: np.zeros((self.nvox, WORDS[c]), DTYPE[c]) for c in (CH_TSDF, CH_CENTROID) if channels & c}
        self.free = np.zeros(self.nbricks, np.uint32) if channels & CH_TSDF else None
        self.cap, self.slots, self.full = {}, {}, {}
        for c, pool in ((CH_TSDF, pool_tsdf), (CH_CENTROID, pool_centroid)):
            if channels & c:
                behind_table = self.sparse and 0 < pool < self.nbricks     # a pool of every brick is a dense channel
                self.cap[c] = pool if behind_table else self.nbricks
                self.slots[c] = np.full(self.nbricks, not behind_table)
                self.full[c] = np.zeros(self.nbricks, bool)
        self.refused = 0

    # ---- bookkeeping ----------------------------------------------------------------------------------------------------
    def n_slots(self, channel):
        return int(self.slots[channel].sum())

    def check(self):
        for c, a in self.rec.items():
            assert not a.reshape(self.nbricks, -1)[~self.slots[c]].any(), "records in a brick without a slot"
            assert self.n_slots(c) <= self.cap[c]

    def _place(self, channel, brick, row):
        """may `row` be written to `brick`?  The sparse rule: a brick without a slot draws one only for a row that holds something,
        while the pool lasts; a refusal is counted once and sticks to the brick."""
        if self.slots[channel][brick]:
            return True
        if not row.any() or self.full[channel][brick]:
            return False
        if self.n_slots(channel) >= self.cap[channel]:
            self.full[channel][brick] = True
            self.refused += 1
            return False
        self.slots[channel][brick] = True
        return True

    # ---- free-space counts ----------------------------------------------------------------------------------------------
    def fold(self):
        """records += count x (32767, 1) for every record of the brick, then the count goes to 0 (bricks with records only)"""
        if self.free is None:
            return
        t = self.rec[CH_TSDF]
        for b in np.nonzero(self.free)[0]:
            if not self.slots[CH_TSDF][b]:
                continue
            c = int(self.free[b])
            r = t[512 * b:512 * b + 512].astype(np.int64)
            r[:, 0] += c * Q
            r[:, 1] += c
            t[512 * b:512 * b + 512] = wrap_i32(r)
            self.free[b] = 0

    def max_weight(self):
        """per brick the largest record weight plus the pending count; the maximum over the bricks"""
        w = np.maximum(self.rec[CH_TSDF][:, 1].astype(np.int64).reshape(self.nbricks, 512).max(axis=1), 0)
        return int((w + self.free.astype(np.int64)).max())

    # ---- whole-channel copies and sums ----------------------------------------------------------------------------------
    def load(self, channel, image):
        """tl3d_grid_upload: the channel becomes `image`; an upload of the TSDF channel clears the counts"""
        image = np.ascontiguousarray(image, DTYPE[channel]).reshape(self.nvox, WORDS[channel])
        if channel == CH_TSDF:
            self.free[:] = 0
        for b in range(self.nbricks):
            row = image[512 * b:512 * b + 512]
            if self._place(channel, b, row):
                self.rec[channel][512 * b:512 * b + 512] = row

    def image(self, channel):
        """tl3d_grid_download: the dense image a reader sees, counts folded in (for real where there are records)"""
        self.fold()
        out = self.rec[channel].copy()
        if channel == CH_TSDF:
            c = np.repeat(self.free.astype(np.int64), 512)
            out = wrap_i32(out.astype(np.int64) + np.stack([c * Q, c], axis=1))
        return out

    def add(self, channel, image):
        """tl3d_grid_add: channel += image.  int32 lanes for the TSDF channel, uint64 lanes for the centroid channel, both wrapping;
        the slot rule of unpack; a TSDF sum that could pass MAX_WEIGHT is refused before anything is written."""
        image = np.ascontiguousarray(image, DTYPE[channel]).reshape(self.nvox, WORDS[channel])
        self.fold()
        if channel == CH_TSDF and self.max_weight() + max(0, int(image[:, 1].max())) > MAX_WEIGHT:
            raise HeadroomError
        a = self.rec[channel]
        for b in range(self.nbricks):
            sl = slice(512 * b, 512 * b + 512)
            if not self._place(channel, b, image[sl]):
                continue
            if channel == CH_TSDF:
                a[sl] = wrap_i32(a[sl].astype(np.int64) + image[sl].astype(np.int64))
            else:
                a[sl] = add_u64(a[sl], image[sl])

    # ---- the sparse form of the merge -----------------------------------------------------------------------------------
    def touched(self, m, channels=0, free_apart=False, sub=False):
        """m |= 1 for every brick (sub: every sub-brick, 8 per brick) with a record whose TSDF weight or centroid count (word 1 >> 32)
        is not 0, in the selected channels (0: all the grid has); without free_apart the counts are folded first"""
        channels = channels or self.channels
        assert m.shape == (self.nbricks * (8 if sub else 1),) and m.dtype == np.uint8
        if not free_apart:
            self.fold()
        n = 64 if sub else 512
        if channels & CH_TSDF:
            m |= (self.rec[CH_TSDF][:, 1].reshape(-1, n) != 0).any(axis=1).astype(np.uint8)
        if channels & CH_CENTROID:
            m |= ((self.rec[CH_CENTROID][:, 1].reshape(-1, n) >> S32) != 0).any(axis=1).astype(np.uint8)
        return m

    def _rows(self, ids, sub):
        for i in ids:
            i = int(i)
            yield (i >> 3, 512 * (i >> 3) + 64 * (i & 7), 64) if sub else (i, 512 * i, 512)

    def pack(self, channel, ids, free_apart=False, sub=False):
        """rows [n, 512 or 64, words] of the listed bricks / sub-bricks; zeros where a sparse grid holds no slot"""
        if not free_apart:
            self.fold()
        a = self.rec[channel]
        rows = [a[lo:lo + n] for _, lo, n in self._rows(ids, sub)]
        return np.stack(rows) if rows else np.zeros((0, 64 if sub else 512, WORDS[channel]), DTYPE[channel])

    def unpack(self, channel, ids, rows, free_apart=False, sub=False):
        """sets exactly the listed rows (ascending, unique ids)"""
        ids = [int(i) for i in ids]
        assert all(x < y for x, y in zip(ids, ids[1:])) and (not ids or ids[-1] < self.nbricks * (8 if sub else 1))
        if not free_apart:
            self.fold()
        a = self.rec[channel]
        for (b, lo, n), row in zip(self._rows(ids, sub), rows):
            if self._place(channel, b, row):
                a[lo:lo + n] = row


def sum_rows(channel, blocks):
    """the SUM all-reduce of packed blocks"""
    if channel == CH_TSDF:
        return wrap_i32(sum(b.astype(np.int64) for b in blocks))
    out = np.zeros_like(blocks[0])
    for b in blocks:
        out = add_u64(out, b)
    return out


def merge(states, sparse=True, trace=None):
    """The sequence tl3d.distributed.allreduce_context_grids performs on every rank, an all-reduce written as a sum or a maximum
    over the list of states: the headroom check; the free-space counts summed (they stay pending); per channel the sub-brick map
    MAX-reduced and the listed rows packed (records only), summed and unpacked -- or, on a dense grid of which half or more is
    listed (or with sparse=False), the whole channel summed in place.  The whole-channel sum reads the records, which folds the
    counts: only rank 0 may still hold the summed counts then, or they would enter the sum once per rank.
    trace: a list that receives (op, [what each rank puts into the collective]) for every all-reduce, in order."""
    def note(op, parts):
        if trace is not None:
            trace.append((op, [np.array(p) for p in parts]))

    s0 = states[0]
    ch, nbr = s0.channels, s0.nbricks
    free_apart = bool(ch & CH_TSDF)
    if free_apart:
        note("sum", [[s.max_weight()] for s in states])
        if sum(s.max_weight() for s in states) > MAX_WEIGHT:
            raise HeadroomError
        note("sum", [s.free for s in states])
        total = sum(s.free.astype(np.int64) for s in states)
        for s in states:
            s.free[:] = (total & 0xffffffff).astype(np.uint32)
    for channel in (CH_TSDF, CH_CENTROID):
        if not ch & channel:
            continue
        apart = free_apart and channel == CH_TSDF
        ids = None
        if sparse:
            maps = [s.touched(np.zeros(8 * nbr, np.uint8), channel, free_apart=apart, sub=True) for s in states]
            note("max", maps)
            m = np.maximum.reduce(maps)
            ids = np.nonzero(m)[0]
            if 2 * len(ids) >= 8 * nbr and not s0.sparse:
                ids = None
        if ids is None and s0.sparse:
            ids = np.arange(8 * nbr)
        if ids is None:
            if apart:
                for s in states[1:]:
                    s.free[:] = 0
            for s in states:
                s.fold()
            note("sum", [s.rec[channel] for s in states])
            total = sum_rows(channel, [s.rec[channel] for s in states])
            for s in states:
                s.rec[channel][:] = total
            continue
        blocks = [s.pack(channel, ids, free_apart=apart, sub=True) for s in states]
        note("sum", blocks)
        block = sum_rows(channel, blocks)
        for s in states:
            s.unpack(channel, ids, block, free_apart=apart, sub=True)


# ---- crafted inputs (reachable states only: a record has non-zero sums only where its weight / count is non-zero) ------------
def probe_bricks(nbricks, first=0):
    """brick `first`, a brick with index = 3 (mod 4) -- the fourth wave of a workgroup of the one-wave-per-brick kernels -- and the last"""
    mid = first + 7
    assert mid % 4 == 3 and first < mid < nbricks - 1
    return (first, mid, nbricks - 1)


def probe(channel, nvox, record):
    """all zero but ONE record, which holds nothing but what marks it: a TSDF weight (a measured tsdf of exactly 0), a centroid
    count (one black point at the voxel's corner)"""
    a = np.zeros((nvox, WORDS[channel]), DTYPE[channel])
    a[record, 1] = 1 if channel == CH_TSDF else 1 << 32
    return a


def random_records(channel, n, rng):
    """full-width bit patterns with a non-zero weight / count: for the pure copies (pack, unpack, upload, download)"""
    bits = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    if channel == CH_TSDF:
        a = (bits[:, :2] & M32).astype(np.uint32).view(np.int32).copy()
        a[a[:, 1] == 0, 1] = 1
        return a
    bits[(bits[:, 1] >> S32) == np.uint64(0), 1] |= np.uint64(1 << 32)
    return bits


def copy_image(channel, state_or_nvox, bricks, seed, sub_bricks=None):
    """random records in the listed bricks (sub_bricks: {brick: sub-bricks that hold anything}, default all eight), zeros elsewhere"""
    nvox = state_or_nvox if isinstance(state_or_nvox, int) else state_or_nvox.nvox
    rng = np.random.default_rng(seed)
    a = np.zeros((nvox, WORDS[channel]), DTYPE[channel])
    for b in bricks:
        for s in (sub_bricks or {}).get(b, range(8)):
            lo = 512 * b + 64 * s
            a[lo:lo + 64] = random_records(channel, 64, rng)
    if channel == CH_TSDF and len(bricks):
        b = bricks[0]
        a[512 * b + 1] = (-Q * 65536, 65536)            # -2147418112: the int32 extremes of a voxel at the weight limit
        a[512 * b + 510] = (Q * 65536, 65536)
    return a


# (a, b) sums of two TSDF records of weight 1 (|sum| <= 32767).  a < 0 < b with |a| > b stays negative; the other pairs reach or
# pass zero or add two negative sums: as unsigned 32-bit halves those carry, which a 64-bit lane would add to the weight.
TSDF_PAIRS_NO_CARRY = ((-30000, 20000), (-32767, 1), (-2, 1))
TSDF_PAIRS_CARRY = ((-20000, 30000), (-1, 1), (-1, 32767), (-7, -9), (-32767, -32767))
TSDF_W_A, TSDF_W_B = 40000, 25536                       # weights that add up to MAX_WEIGHT exactly


def _u64(*words):
    return np.array(words, dtype=np.uint64)


def add_images(channel, nvox, bricks_a, bricks_b):
    """(A, B): the grid and the image added to it.  Crafted records sit at the probe positions of every brick both hold; the bricks
    only one of them holds (a sparse grid: a brick that draws its slot on receipt / a brick that receives zeros) get a few too."""
    a = np.zeros((nvox, WORDS[channel]), DTYPE[channel])
    b = np.zeros_like(a)
    both = [x for x in bricks_a if x in bricks_b]
    assert both
    if channel == CH_TSDF:
        pairs = TSDF_PAIRS_NO_CARRY + TSDF_PAIRS_CARRY
        for n, br in enumerate(both):
            for k, pos in enumerate(PROBE_POSITIONS):
                pa, pb = pairs[(n + k) % len(pairs)]
                a[512 * br + pos] = (pa, 1)
                b[512 * br + pos] = (pb, 1)
            # the int32 extremes: -32767 w and +32767 w with the weights at the limit, in either half of a 16-byte pair
            a[512 * br + 200], b[512 * br + 200] = (-Q * TSDF_W_A, TSDF_W_A), (-Q * TSDF_W_B, TSDF_W_B)
            a[512 * br + 201], b[512 * br + 201] = (Q * TSDF_W_A, TSDF_W_A), (Q * TSDF_W_B, TSDF_W_B)
            a[512 * br + 300], b[512 * br + 300] = (-Q * TSDF_W_A, TSDF_W_A), (Q * TSDF_W_B, TSDF_W_B)
        for img, only in ((a, [x for x in bricks_a if x not in bricks_b]), (b, [x for x in bricks_b if x not in bricks_a])):
            for br in only:
                img[512 * br + 77] = (-12345, 3)
                img[512 * br + 511] = (Q * 9, 9)
    else:
        for n, br in enumerate(both):
            for k, pos in enumerate(PROBE_POSITIONS):
                lo_a, lo_b = 0xfffffff0 - k, 0x20 + n + k                  # low halves that sum past 2^32
                a[512 * br + pos] = _u64(lo_a | 5 << 32, lo_a | ((1 << 20) - 1 - k) << 32, lo_a | 0xfffffffe << 32, lo_a)
                b[512 * br + pos] = _u64(lo_b | 7 << 32, lo_b | (1 + k) << 32, lo_b | 3 << 32, lo_b)  # counts sum to 2^20; word 2 wraps mod 2^64
        for img, only in ((a, [x for x in bricks_a if x not in bricks_b]), (b, [x for x in bricks_b if x not in bricks_a])):
            for br in only:
                img[512 * br + 77] = _u64(0x80000001 | 0xc0000003 << 32, 17 | 2 << 32, 400 | 300 << 32, 200)
                img[512 * br + 511] = _u64(1, 1 << 32, 0, 0)
    return a, b


# ---- three ranks with partly disjoint bricks (16 bricks) ---------------------------------------------------------------------
# records: brick 1 on every rank, 2 / 5 / 15 on exactly one, 7 and 9 on two, 3 on none (and no count: nothing at all)
RANK_TSDF_BRICKS = ((1, 2, 7), (1, 5, 9), (1, 7, 9, 15))
RANK_CENTROID_BRICKS = ((1, 6, 7), (1, 9, 10), (0, 1, 9, 15))
# pending counts: 12 / 13 / 14 count-only on one rank each, 4 count-only on all, 1 and 9 next to records, 5 count-only on rank 0
# where rank 1 holds records (a sparse rank 0 draws the slot when the merged rows arrive and folds its count into them later)
RANK_COUNTS = ({12: 3, 4: 1, 1: 2, 5: 7}, {13: 65, 4: 10}, {14: 1, 4: 100, 9: 4})
RANK_POOLS = (12, 12)                                   # sparse layout: every brick any rank holds fits (no refusal in the merge)


def rank_inputs(r):
    """(TSDF image, centroid image, counts) of rank r: what its frames would have left, before anything is folded"""
    rng = np.random.default_rng(100 + r)
    nvox, nbricks = DIMS[0] * DIMS[1] * DIMS[2], DIMS[0] * DIMS[1] * DIMS[2] // 512
    t = np.zeros((nvox, 2), np.int32)
    c = np.zeros((nvox, 4), np.uint64)
    for b in RANK_TSDF_BRICKS[r]:
        for sb in sorted(rng.choice(8, size=1 + (b + r) % 4, replace=False)):             # a surface crosses a few sub-bricks
            lo = 512 * b + 64 * int(sb)
            w = rng.integers(1, 50, 64) * (rng.random(64) < 0.7)                            # some records of the sub-brick stay empty
            w[int(sb)] = 1 + int(sb)                                                        # (but never all)
            t[lo:lo + 64, 1] = w
            t[lo:lo + 64, 0] = rng.integers(-Q, Q + 1, 64) * w
    for b in RANK_CENTROID_BRICKS[r]:
        for sb in sorted(rng.choice(8, size=1 + (b + 2 * r) % 3, replace=False)):
            lo = 512 * b + 64 * int(sb)
            n = rng.integers(1, 100, 64).astype(np.uint64) * (rng.random(64) < 0.6)
            n[int(sb)] = 1 + int(sb)
            words = rng.integers(0, 1 << 64, size=(64, 4), dtype=np.uint64)               # full-width halves: the sums carry
            words[:, 1] = (words[:, 1] & M32) | (n << S32)
            words[n == 0] = 0
            c[lo:lo + 64] = words
    counts = np.zeros(nbricks, np.uint32)
    for b, n in RANK_COUNTS[r].items():
        counts[b] = n
    return t, c, counts


def rank_states(sparse):
    """three RankStates (fresh ones on every call), loaded the way the GPU test loads its contexts: records uploaded, counts set"""
    out = []
    for r in range(3):
        s = RankState(DIMS, pool_tsdf=RANK_POOLS[0] if sparse else 0, pool_centroid=RANK_POOLS[1] if sparse else 0)
        t, c, counts = rank_inputs(r)
        s.load(CH_TSDF, t)
        s.load(CH_CENTROID, c)
        s.free[:] = counts
        s.check()
        out.append(s)
    return out


def python_sum_of_folded_images(states):
    """{channel: image}: the elementwise Python-integer sum of the ranks' folded dense images, wrapped to the stored width --
    what a merge must leave on every rank, computed with nothing of the model but RankState.image"""
    out = {}
    for channel in (CH_TSDF, CH_CENTROID):
        imgs = [s.image(channel) for s in states]
        tot = [sum(int(v) for v in vals) for vals in zip(*(i.ravel().tolist() for i in imgs))]
        if channel == CH_TSDF:
            tot = [((v + (1 << 31)) % (1 << 32)) - (1 << 31) for v in tot]
            out[channel] = np.array(tot, np.int64).astype(np.int32).reshape(imgs[0].shape)
        else:
            out[channel] = np.array([v % (1 << 64) for v in tot], np.uint64).reshape(imgs[0].shape)
    return out
