"""The TSDF update on its decision edges: the crafted frames of tsdf_edges_common through the HIP kernels, every grid compared
bit for bit (np.array_equal on the downloaded channel) with the C oracle and, where it applies, with the exact-rational model of
tsdf_edges_reference.  tests/test_tsdf_edges_reference_cpu.py proves on the CPU that the edges are hit and that the references
agree with each other.

What fails here when a comparison of the pair kernel moves by one voxel (tried on scratch builds of kernels_tsdf.hip):
  * `sdf > -trunc` for `sdf >= -trunc` in stage C: 94 of the 117 tests, first test_single_frame[t0] (129 voxels at sdf == -trunc);
    test_32_saturated_observations_in_one_launch[all_behind] loses the whole zc = 1 slice;
  * a window that leaves out uf == -0.5 (`uf > -0.5` beside the unsigned compare): test_single_frame[left] and [u16_left], the
    family sequence, the 33-frame and the degenerate batch; frame top does the same for vf;
  * `trunc_free = g.trunc` for `g.trunc * 1.001f`: NOT detectable through the grid, by any input -- a voxel the tile rule then calls
    free has sdf >= trunc, so sdf * fl(1 / trunc) >= 1 - 2^-23 and rint(32767 (1 - 2^-23)) == 32767, the value a free voxel gets:
    the margin guards nothing the quantisation does not already absorb.  Frames t0 and right hold 40 and 56 voxels strictly
    inside the band all the same, and all 117 tests pass on such a build.
"""
import numpy as np
import pytest

import tl3d
import tsdf_edges_common as ec
import tsdf_edges_reference as er

pytestmark = pytest.mark.gpu

FAMILY = ec.family()
PERMS = ec.permutation_cases()
VARIANTS = ec.variants()
ALL = FAMILY + PERMS + VARIANTS
BY_NAME = {c.name: c for c in ALL}


def _ids(cases):
    return [c.name for c in cases]


_REF = {}


def reference(case):
    """(C oracle's grid of the single frame, rational model's grid or None, where the model applies) -- computed once, never changed"""
    key = (case.name, case.dims)
    if key not in _REF:
        orc = ec.c_oracle_for(case)
        orc.tsdf_integrate(case.depth, case.R, case.t, case.scale)
        model, applies = er.integrate(case) if case.dyadic else (None, None)
        for a in (orc.tsdf, model, applies):
            if a is not None:
                a.setflags(write=False)
        _REF[key] = (orc.tsdf, model, applies)
    return _REF[key]


def reference_sum(cases):
    """the oracle's grid of the frames fused one at a time (integer sums), the model's likewise, where every frame's model applies"""
    total = np.zeros_like(reference(cases[0])[0])
    model, applies = np.zeros_like(total), np.ones(len(total), bool)
    for c in cases:
        g, m, a = reference(c)
        total += g
        if m is None:
            model = None
        elif model is not None:
            model += m
            applies &= a
    return total, model, applies


def context(case, n_slots=1, grid=True):
    c = case.cam
    spec = tl3d.GridSpec(case.dims, case.origin, ec.VOXEL, ec.TRUNC, tl3d.CH_TSDF) if grid else None
    return tl3d.FusionContext(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], min_depth=ec.MIN_DEPTH, max_depth=ec.MAX_DEPTH,
                              n_slots=n_slots, grid=spec)


def upload_all(ctx, cases):
    """every DISTINCT image once; slot of each image"""
    slot_of = {}
    for c in cases:
        if id(c.upload) not in slot_of:
            slot_of[id(c.upload)] = len(slot_of)
            ctx.upload(slot_of[id(c.upload)], c.upload, None)
    return slot_of


def integrate_all(ctx, cases, slot_of, order=None):
    for i in (range(len(cases)) if order is None else order):
        c = cases[i]
        ctx.integrate(slot_of[id(c.upload)], c.pose, c.scale)
    return ctx.download_grid(tl3d.CH_TSDF)


def fuse(ctx, cases, order=None):
    """upload, integrate the frames in `order`; the downloaded TSDF channel"""
    return integrate_all(ctx, cases, upload_all(ctx, cases), order)


def attach_exact_pool(ctx, cases, slot_of):
    """Give the grid-less context a SPARSE grid whose pool holds exactly the bricks this fusion gives records to.  That is the
    library's own count (count_bricks: the fusion's classification without records), not the number of bricks the oracle
    touches: the classification is conservative, so a brick on the image border or beside a hole is listed -- and takes a slot --
    although no voxel of it is updated in the end (kernels_tsdf_prep.hip, brick_cull_kernel), while a brick that is free space in
    every frame is touched by the oracle and keeps a 4-byte count instead of records.  What the oracle's grid does bound: every
    brick holding a record that is not pure free space was listed, so it needs a slot."""
    geom = tl3d.GridSpec(cases[0].dims, cases[0].origin, ec.VOXEL, ec.TRUNC, tl3d.CH_TSDF)
    nt, _ = ctx.count_bricks(geom, [slot_of[id(c.upload)] for c in cases], [c.pose for c in cases], scales=[c.scale for c in cases])
    want = reference_sum(cases)[0].astype(np.int64).reshape(-1, 512, 2)
    needs = int((want[:, :, 0] != 32767 * want[:, :, 1]).any(axis=1).sum())
    nbricks = len(want)
    assert needs <= nt <= nbricks, (needs, nt, nbricks)
    ctx.attach_grid(tl3d.GridSpec(cases[0].dims, cases[0].origin, ec.VOXEL, ec.TRUNC, tl3d.CH_TSDF, pool_tsdf=max(1, nt)))
    return nt


def n_images(cases):
    return len({id(c.upload) for c in cases})


def check(grid, cases, what=""):
    want, model, applies = reference_sum(cases)
    assert np.array_equal(grid, want), (what, int((grid != want).any(axis=1).sum()))
    if model is not None:
        assert np.array_equal(grid[applies], model[applies]), what


# ---- single frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_single_frame(case):
    with context(case) as ctx:
        check(fuse(ctx, [case]), [case], case.name)


# ---- update forms and layouts ------------------------------------------------------------------------------------------------------
def batched_or_not_dense_or_sparse(cases, what):
    """deferred to the batch boundary or one launch per frame; records for every brick or a pool of exactly the bricks the fusion
    gives records to"""
    for sparse in (False, True):
        with context(cases[0], n_slots=n_images(cases), grid=not sparse) as ctx:
            slot_of = upload_all(ctx, cases)
            nt = attach_exact_pool(ctx, cases, slot_of) if sparse else None
            launches = []
            for pairing in (True, False):
                ctx.reset()
                ctx.reset_stats()
                ctx.set_tsdf_pairing(pairing)
                check(integrate_all(ctx, cases, slot_of), cases, (what, sparse, pairing))
                launches.append(ctx.stats()["tsdf_launches"])
                if sparse:
                    st = ctx.stats()
                    assert st["pool_refused"] == 0 and st["pool_slots_tsdf"] == nt, (what, pairing, nt, st["pool_slots_tsdf"], st["pool_refused"])
            assert launches == [1, len(cases)], launches


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_single_frame_batched_or_not_dense_or_sparse(case):
    batched_or_not_dense_or_sparse([case], case.name)


GROUPS = {"family": FAMILY, "permutations": PERMS,
          "ragged": [c for c in VARIANTS if c.name.startswith("ragged")],
          "base_variants": [BY_NAME[n] for n in ("scale2", "scale3", "rot0", "rot1", "no_valid", "last_pixel", "all_free")]}


@pytest.mark.parametrize("group", list(GROUPS))
def test_sequences_batched_or_not_dense_or_sparse(group):
    batched_or_not_dense_or_sparse(GROUPS[group], group)


# ---- f32 against u16 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u16_t0", "u16_left"])
def test_f32_and_u16_frames_of_the_same_millimetres_give_the_same_grid(name):
    case = BY_NAME[name]
    as_f32 = ec.replace(case, mm=None)
    with context(case) as ctx:
        g16 = fuse(ctx, [case])
        ctx.reset()
        g32 = fuse(ctx, [as_f32])
    assert np.array_equal(g16, g32)
    check(g16, [case], name)


# ---- 32 observations of one voxel in one launch -----------------------------------------------------------------------------------------
# The running sum of a voxel over a batch is ONE 32-bit LDS word: 21 bits of sum(q + 32768), 11 bits of weight.  32 free-space
# observations give 32 * 65535 = 2 097 120 of 2^21 = 2 097 152.
BIG = ec.with_grid(ec.base_case(), (40, 16, 24), (-12, 0, 0), "big")


def on_big(case, name, hole=False):
    """`case` fused into the 5 x 2 x 3-brick grid; hole: no valid pixel in tile columns 3-4 of tile rows 1-2"""
    d = case.depth
    if hole:
        d = d.copy()
        d[8:24, 24:40] = 0.0
    return ec.replace(case, name=name, dims=BIG.dims, origin=BIG.origin, depth=d)


def wall(z, name):
    return ec.replace(ec.base_case(name), depth=np.full((ec.CAM["height"], ec.CAM["width"]), z, np.float32))


def mixed_class_sequence():
    """32 frames of one pose.  Brick (1, 0, 2) of the big grid -- x in [-3/8, -1/8], zc in [0.98, 1.23], pixels 6..18 x 2..14 with the
    classifiers' margin: inside the image, clear of the hole -- is FREE under the far wall, MIXED under the patchwork (sub-bricks of
    it FREE, others with voxels the tiles decide and voxels that read their pixel), SKIPPED under the walls at 0.75 and 0.6 (more
    than trunc behind them) and under the frame with no valid pixel.  Frames 0..30 carry the hole, so brick (4, 1, 2) -- pixels
    28..39 x 10..21, all inside the hole -- is skipped by every one of them; frame 31, the whole patchwork, is the only frame that
    lists it: bit 31 of its frame mask, alone."""
    kinds = [on_big(ec.all_free(), "far_hole", True), on_big(ec.base_case(), "patch_hole", True), on_big(wall(0.75, "w075"), "w075_hole", True),
             on_big(wall(0.6, "w06"), "w06_hole", True), on_big(ec.no_valid_pixel(), "none")]
    seq = [kinds[i % 5] for i in range(31)] + [on_big(ec.base_case(), "patch_whole")]
    assert len(seq) == 32
    return seq


def saturated(name):
    return [on_big({"all_free": ec.all_free(), "t0": ec.base_case(), "all_behind": ec.saturating_behind()}[name], name)] * 32


SEQ32 = {"all_free": lambda: saturated("all_free"), "t0": lambda: saturated("t0"), "all_behind": lambda: saturated("all_behind"),
         "mixed_classes": mixed_class_sequence}


@pytest.mark.parametrize("name", list(SEQ32))
def test_32_saturated_observations_in_one_launch(name):
    """all_free: 32 x (32767, 1) by the brick-level counters and, in the bricks on the image border, by the LDS word at its limit;
    t0: the same for the patchwork's free voxels, beside 32 x every other q; all_behind: 32 x q = -32767 (packed: 32 x 1);
    mixed_classes: brick-level counts, sub-brick-level counts and pair increments meet in one record."""
    seq = SEQ32[name]()
    with context(seq[0], n_slots=n_images(seq)) as ctx:
        ctx.set_profile(True, False)
        g = fuse(ctx, seq)
        st = ctx.stats()
        assert st["tsdf_launches"] == 1, st["tsdf_launches"]
        if name in ("all_free", "mixed_classes"):
            assert st["tsdf_bricks_free"] > 0
    check(g, seq, name)
    if name == "all_free":
        assert (g[:, 1] == 32).sum() > 5000 and (g[g[:, 1] == 32, 0] == 32 * 32767).all()
    if name == "all_behind":
        assert ((g[:, 1] == 32) & (g[:, 0] == -32 * 32767)).sum() >= 256


def test_33_frames_take_two_launches_and_bit_31_counts():
    seq = mixed_class_sequence()
    # frame 31 is the only one that can list brick (4, 1, 2): the others have no valid pixel under it
    brick = (2 * 2 + 1) * 5 + 4
    for i, c in enumerate(seq):
        sees = bool((reference(c)[0][brick * 512:(brick + 1) * 512, 1] > 0).any())
        assert sees == (i == 31), i
    seq.append(on_big(ec.base_case("left", (-13 / 32, 0.0, 0.0)), "patch_left"))
    with context(seq[0], n_slots=n_images(seq)) as ctx:
        g = fuse(ctx, seq)
        assert ctx.stats()["tsdf_launches"] == 2
    check(g, seq, "33 frames")


# ---- degenerate frames inside a batch ------------------------------------------------------------------------------------------------
def test_degenerate_frames_in_a_batch_in_either_order():
    seq = [BY_NAME["t0"], BY_NAME["left"], BY_NAME["no_valid"], BY_NAME["right"], BY_NAME["last_pixel"]]
    with context(seq[0], n_slots=n_images(seq)) as ctx:
        fwd = fuse(ctx, seq)
        assert ctx.stats()["tsdf_launches"] == 1
        ctx.reset()
        rev = fuse(ctx, seq, order=range(len(seq) - 1, -1, -1))
    check(fwd, seq, "forward")
    assert np.array_equal(rev, fwd)                                       # integer sums commute


# ---- camera-plane poses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zhalf", "zone", "eps_x", "eps_xy"])
def test_nothing_is_written_on_or_behind_the_camera_plane(name):
    case = BY_NAME[name]
    with context(case) as ctx:
        g = fuse(ctx, [case])
    check(g, [case], name)
    m = ec.intermediates(case)
    rec = ec.sn.record_index(m["I"], m["J"], m["K"], case.dims[0] // 8, case.dims[1] // 8)
    behind = rec[m["zc"] <= 0]
    assert len(behind) >= 256 and not g[behind].any()
    if name == "eps_xy":                                                   # zc = 2^-20, xc = yc = 0: pixel (20, 12), far in front of it
        r = int(ec.sn.record_index(7, 7, 16, 2, 2))
        assert m["zc"][16, 7, 7] == np.float32(2.0 ** -20) and tuple(g[r]) == tuple(reference(case)[0][r]) == (32767, 1)


# ---- every camera axis against every lane and sub-brick axis ------------------------------------------------------------------------------
def test_all_24_axis_permutations_in_one_batch_and_one_at_a_time():
    with context(PERMS[0], n_slots=1) as ctx:
        grids, launches = [], []
        for pairing in (True, False):
            ctx.reset()
            ctx.reset_stats()
            ctx.set_tsdf_pairing(pairing)
            grids.append(fuse(ctx, PERMS))
            launches.append(ctx.stats()["tsdf_launches"])
    assert launches == [1, 24], launches
    check(grids[0], PERMS, "one batch")
    check(grids[1], PERMS, "one at a time")
