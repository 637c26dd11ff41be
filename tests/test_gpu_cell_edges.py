"""GPU: the crafted cases of cell_edges_common through the two kernels that read the TSDF cell (csrc/tsdf_cell.h) -- raycast_kernel
(tl3d_raycast) and track_pass_kernel (tl3d_track_evaluate / tl3d_track_frame) -- against the f32 restatements (raycast_reference,
track_reference), which tests/test_cell_edges_reference_cpu.py holds to an fp64 model of its own on the same cases.

Ray casting: depth, normals and colour byte for byte, per case; device outputs, and the frame-slot path, on one case per family.
Tracking: n_src and n_corr exactly; on the exact cases A, b and e byte for byte too -- their sums are exact (the CPU test adds them
three ways), so no order of addition can change them and a lost or doubled sample cannot hide in a reordering bound; on the others
the bound of test_gpu_track.  Sparse: crafted cases behind brick tables (empty TSDF bricks, an absent centroid brick); both readers on a grid whose pool was too short for the frames, against the restatement over
that grid's own download.  Every test has its own small context."""
import functools

import numpy as np
import pytest

import cell_edges_common as cc
import raycast_reference as rr
import tl3d
import track_reference as tr
from helpers import TINY
from tl3d import synth

pytestmark = pytest.mark.gpu

CASES = cc.cases()
RAY = [c for c in CASES if c.kind == "ray"]
TRACK = [c for c in CASES if c.kind == "track"]
ids = lambda cs: [c.name for c in cs]


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _assert_same(got, want, what):
    for a, b, name in zip(got, want, ("depth", "normals", "bgr")):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(_bytes(a), _bytes(b)), (what, name, int((_bytes(a) != _bytes(b)).sum()), np.argwhere(a != b)[:4].tolist())


def _context(case, n_slots=1):
    channels = tl3d.CH_TSDF | (tl3d.CH_CENTROID if case.cen is not None else 0)
    cam = case.cam
    ctx = tl3d.FusionContext(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], min_depth=case.min_depth, max_depth=case.max_depth,
                             n_slots=n_slots, grid=tl3d.GridSpec(case.dims, case.origin, cc.VOXEL, cc.TRUNC, channels))
    ctx.upload_grid(tl3d.CH_TSDF, case.rec)
    if case.cen is not None:
        ctx.upload_grid(tl3d.CH_CENTROID, case.cen)
    return ctx


@functools.lru_cache(maxsize=None)
def _restated_view(name):
    case = cc.by_name(name)
    zn, zf = case.z_range
    with np.errstate(all="ignore"):
        return rr.raycast(case.rec, case.dims, case.origin, cc.VOXEL, cc.TRUNC, case.cam, case.pose, min_weight=case.min_weight, z_near=zn, z_far=zf,
                          centroid=case.cen)[:3]


def _cast(ctx, case, **kw):
    return ctx.raycast(case.pose, min_weight=case.min_weight, z_near=case.z_near, z_far=case.z_far, **kw)


# ---- ray casting -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RAY, ids=ids(RAY))
def test_raycast_equals_the_restatement(case):
    want = _restated_view(case.name)
    with _context(case) as ctx:
        got = _cast(ctx, case)
        print(case.name, "hits", int((got[0] > 0).sum()), "of", got[0].size, "; restatement", int((want[0] > 0).sum()))
        _assert_same(got, want, case.name)
        _assert_same(_cast(ctx, case), got, case.name + " (again)")


ONE_PER_FAMILY = [cc.by_name(n) for n in ("range_far_at_sample", "box_parallel_outside", "steps_cap_reached_by_the_hit", "zeros_unobserved_column",
                                          "weights_checker_mw2", "colour_last_half_voxel", "shapes_17x33", "generic_tilt_0")]


@pytest.mark.parametrize("case", ONE_PER_FAMILY, ids=ids(ONE_PER_FAMILY))
def test_device_outputs_equal_host_outputs(case):
    import torch
    H, W = case.cam["height"], case.cam["width"]
    want = _restated_view(case.name)
    with _context(case) as ctx:
        dev = (torch.full((H, W), -7.0, dtype=torch.float32, device="cuda"), torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda"),
               torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda"))
        _cast(ctx, case, out=dev)
        _assert_same(tuple(t.cpu().numpy() for t in dev), want, case.name)
        only_depth = np.full((H, W), -7.0, np.float32)
        _cast(ctx, case, out=(only_depth, None, None))
        assert np.array_equal(_bytes(only_depth), _bytes(want[0]))


@pytest.mark.parametrize("name", ["colour_last_half_voxel", "shapes_5x3", "shapes_17x33"])
def test_the_slot_path_with_and_without_a_colour_buffer(name):
    case = cc.by_name(name)
    H, W = case.cam["height"], case.cam["width"]
    want = _restated_view(name)
    with _context(case, n_slots=3) as ctx:
        ctx.upload(0, np.full((H, W), 9.0, np.float32), np.full((H, W, 3), 9, np.uint8))        # a slot with a colour buffer
        ctx.upload(1, np.full((H, W), 9000, np.uint16), None)                                   # one without, holding a 16-bit frame
        for slot in (0, 1, 2):                                                                   # 2: an empty slot
            got = _cast(ctx, case, slot=slot)
            _assert_same(got, want, (name, slot))
            assert np.array_equal(_bytes(ctx.download_depth(slot)), _bytes(want[0])), (name, slot)


def _occupied(arr, words):
    return int((np.asarray(arr).reshape(-1, 512 * words) != 0).any(axis=1).sum())


SPARSE = [cc.by_name(n) for n in ("range_far_at_sample", "box_parallel_outside", "steps_cap_reached_by_the_hit", "zeros_unobserved_column",
                                  "weights_checker_mw2", "shapes_17x33", "colour_last_half_voxel")]


@pytest.mark.parametrize("case", SPARSE, ids=ids(SPARSE))
def test_a_sparse_grid_reads_bricks_without_records_as_nothing(case):
    """the same crafted grids behind brick tables: an upload gives slots to the bricks that hold something only, so the rays cross
    SLOT_EMPTY entries before the bricks with records -- and, in the colour case, hit voxels whose centroid brick is absent"""
    cen = None
    if case.cen is not None:
        cen = case.cen.copy()
        cen[4 * 512:5 * 512] = 0                          # brick (0, 0, 1) of the 2 x 2 x 2: the hits with i, j < 8 land in it
    want = rr.raycast(case.rec, case.dims, case.origin, cc.VOXEL, cc.TRUNC, case.cam, case.pose, min_weight=case.min_weight, z_near=case.z_range[0],
                      z_far=case.z_range[1], centroid=cen)[:3]
    nbricks = case.dims[0] * case.dims[1] * case.dims[2] // 512
    nt, nc = _occupied(case.rec, 2), _occupied(cen, 4) if cen is not None else 0
    assert 0 < nt < nbricks and (cen is None or 0 < nc < nbricks)
    cam = case.cam
    spec = tl3d.GridSpec(case.dims, case.origin, cc.VOXEL, cc.TRUNC, tl3d.CH_TSDF | (tl3d.CH_CENTROID if cen is not None else 0), pool_tsdf=nt,
                         pool_centroid=nc)
    with tl3d.FusionContext(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], min_depth=case.min_depth, max_depth=case.max_depth,
                            n_slots=1, grid=spec) as ctx:
        ctx.upload_grid(tl3d.CH_TSDF, case.rec)
        if cen is not None:
            ctx.upload_grid(tl3d.CH_CENTROID, cen)
        st = ctx.stats()
        print(case.name, "bricks", nbricks, "slots: TSDF", st["pool_slots_tsdf"], "of", nt, "centroid", st["pool_slots_centroid"], "of", nc, "refused", st["pool_refused"])
        assert (st["pool_slots_tsdf"], st["pool_slots_centroid"], st["pool_refused"]) == (nt, nc, 0)
        _assert_same(_cast(ctx, case), want, case.name)
    if cen is not None:
        full = _restated_view(case.name)
        grey, grey_full = (want[2] == 128).all(axis=-1), (full[2] == 128).all(axis=-1)
        assert (grey & ~grey_full).sum() > 5 and (~grey).sum() > 5            # some hits lost their colour with the brick, others kept theirs


# ---- tracking ----------------------------------------------------------------------------------------------------------------------------
def _sums_of(ev):
    return np.concatenate([ev["A"][np.triu_indices(6)], ev["b"], [ev["e"]]])


def _check_pass(ctx, case, rec, depth, what):
    got = ctx.track_evaluate(0, case.pose, stride=case.stride, max_dist=case.max_dist, min_weight=case.min_weight, scale=case.scale)
    want = tr.sums(rec, case.dims, case.origin, cc.VOXEL, cc.TRUNC, case.cam, depth, case.pose, stride=case.stride, max_dist=case.max_dist,
                   min_weight=case.min_weight, min_depth=case.min_depth, max_depth=case.max_depth, scale=case.scale)
    print(what, "n_src", got["n_src"], want["n_src"], "n_corr", got["n_corr"], want["n_corr"])
    assert (got["n_src"], got["n_corr"]) == (want["n_src"], want["n_corr"]), what
    g, w = _sums_of(got), np.concatenate([want["A"], want["b"], [want["e"]]])
    if case.exact:
        assert np.array_equal(_bytes(g + 0.0), _bytes(w + 0.0)), (what, np.nonzero(g != w)[0].tolist(), (g - w)[g != w].tolist())
    else:                                          # n_corr terms in another order: (n_corr - 1) 2^-53 sum|term|, held twice over (test_gpu_track)
        assert np.all(np.abs(g - w) <= want["n_corr"] * 2.0 ** -52 * want["abs"]), what
    again = ctx.track_evaluate(0, case.pose, stride=case.stride, max_dist=case.max_dist, min_weight=case.min_weight, scale=case.scale)
    assert np.array_equal(_bytes(_sums_of(again)), _bytes(g)) and (again["n_src"], again["n_corr"]) == (got["n_src"], got["n_corr"]), what
    return got


@pytest.mark.parametrize("case", TRACK, ids=ids(TRACK))
def test_track_evaluate_equals_the_restatement(case):
    with _context(case) as ctx:
        ctx.upload(0, case.depth, None)
        depth = ctx.download_depth(0)
        assert np.array_equal(_bytes(depth), _bytes(cc.frame_f32(case)))                        # NaN, inf and the 16-bit conversion as they are
        got = _check_pass(ctx, case, case.rec, depth, case.name)
        assert got["n_corr"] > (3 if case.cam["width"] == 9 else 50)


def test_track_frame_of_two_iterations_equals_the_reference():
    case = cc.by_name("track_64x32_s1")
    levels = [dict(iters=2, stride=1, max_dist=case.max_dist, damping=1e-6, eps=1e-12, eig_rel=1e-4)]
    with _context(case) as ctx:
        ctx.upload(0, case.depth, None)
        got = ctx.track(0, case.pose, levels, min_weight=case.min_weight)
        again = ctx.track(0, case.pose, levels, min_weight=case.min_weight)
    want = tr.track(case.rec, case.dims, case.origin, cc.VOXEL, cc.TRUNC, case.cam, cc.frame_f32(case), case.pose, levels, min_weight=case.min_weight,
                    min_depth=case.min_depth, max_depth=case.max_depth)
    diff = float(np.abs(got["T"] - want["T"]).max())
    moved = float(np.abs(got["T"] - tr.pose_matrix(case.pose)).max())
    print("status", got["status"], want["status"], "iters", got["iters_run"], want["iters_run"], "n_corr", got["n_corr"], want["n_corr"], "n_src", got["n_src"],
          want["n_src"], f"|T - T_reference| {diff:.3e}, moved {moved:.3e}, rmse {got['rmse']:.6e} {want['rmse']:.6e}")
    assert (got["status"], got["iters_run"], got["n_corr"], got["n_src"]) == (want["status"], want["iters_run"], want["n_corr"], want["n_src"])
    assert got["iters_run"] == 2 and moved > 1e-4
    # the first pass's sums are exact, so both solvers are given the same 6 x 6 system; a plane leaves three directions free and the
    # damped solves differ in rounding only: 2^-40 of the pose's entries (|t| < 8) is a thousand times the fp64 rounding of two solves
    assert diff <= 8.0 * 2.0 ** -40
    assert np.array_equal(got["T"], again["T"]) and got["rmse"] == again["rmse"]


# ---- a sparse grid whose pool is too short ----------------------------------------------------------------------------------------------
def _brick_state(rec):
    return np.abs(rec.reshape(-1, 512, 2)).sum(axis=(1, 2)) > 0


def _crossings(state_dense, state_sparse, dims, origin, voxel, cam, pose):
    """(rays that cross a refused brick and later one with records, rays that do so in the other order): x(z) sampled every half voxel"""
    R, t = np.asarray(pose[0], np.float64), np.asarray(pose[1], np.float64).reshape(3)
    C = -(R.T @ t)
    vv, uu = np.meshgrid(np.arange(cam["height"]), np.arange(cam["width"]), indexing="ij")
    d = np.stack([(uu - cam["cx"]) / cam["fx"], (vv - cam["cy"]) / cam["fy"], np.ones(uu.shape)], axis=-1) @ R        # R^T (xf, yf, 1)
    z = np.arange(0.05, 1.5, 0.5 * voxel)
    x = ((C + d[..., None, :] * z[:, None]) - np.asarray(origin)) / voxel - 0.5
    inside = np.all((x >= 0) & (x <= np.asarray(dims) - 1), axis=-1)
    b = np.clip(np.floor(x + 0.5).astype(np.int64), 0, np.asarray(dims) - 1) // 8
    brick = (b[..., 2] * (dims[1] // 8) + b[..., 1]) * (dims[0] // 8) + b[..., 0]
    refused = inside & (state_dense & ~state_sparse)[brick]
    kept = inside & state_sparse[brick]
    first = lambda m: np.where(m.any(axis=-1), m.argmax(axis=-1), 10 ** 9)
    last = lambda m: np.where(m.any(axis=-1), m.shape[-1] - 1 - m[..., ::-1].argmax(axis=-1), -1)
    return int((first(refused) < last(kept)).sum()), int((first(kept) < last(refused)).sum())


def test_both_readers_on_a_grid_whose_pool_ran_out():
    dims, origin, voxel = (32, 32, 32), (-0.16, -0.16, -0.16), 0.01
    scene = synth.Scene(spheres=[((0.0, 0.0, 0.0), 0.10), ((0.07, 0.03, 0.0), 0.06)])
    poses = synth.orbit_poses(4, 0.5, 25.0)
    frames = [synth.render(scene, p, **TINY)[0] for p in poses]
    make = lambda grid: tl3d.FusionContext(TINY["width"], TINY["height"], TINY["fx"], TINY["fy"], TINY["cx"], TINY["cy"], n_slots=4, grid=grid)
    geom = tl3d.GridSpec(dims, origin, voxel, 4 * voxel, tl3d.CH_TSDF)
    with make(geom) as dense, make(None) as sp:
        for c in (dense, sp):
            for i, d in enumerate(frames):
                c.upload(i, d, None)
        nt, _ = sp.count_bricks(geom, list(range(4)), poses)
        assert nt > 8
        sp.attach_grid(tl3d.GridSpec(dims, origin, voxel, 4 * voxel, tl3d.CH_TSDF, pool_tsdf=nt // 2))
        for c in (dense, sp):
            for i in range(4):
                c.integrate(i, poses[i])
        rec_d, rec_s = dense.download_grid(tl3d.CH_TSDF), sp.download_grid(tl3d.CH_TSDF)
        st = sp.stats()
        refused, slots = st["pool_refused"], st["pool_slots_tsdf"]
        sd, ss = _brick_state(rec_d), _brick_state(rec_s)
        print("bricks with records: dense", int(sd.sum()), "sparse", int(ss.sum()), "of a pool of", nt // 2, "slots handed out", slots, "; refusals reported", refused)
        assert refused > 0 and ss.sum() <= nt // 2 and 0 < ss.sum() < sd.sum() and not (ss & ~sd).any()
        before = after = 0
        # the pool goes to the bricks the classification reaches first, the low ones: seen from behind, the refused bricks come first
        # (and from the sides and from above, where the surfaces the frames saw are still in view)
        views = list(poses) + synth.orbit_poses(4, 0.5, 35.0, start_deg=-105.0) + synth.orbit_poses(3, 0.45, 40.0, height=0.25, start_deg=-20.0)
        differs = fewer = 0
        for k, pose in enumerate(views):
            a, b = _crossings(sd, ss, dims, origin, voxel, TINY, pose)
            before, after = before + a, after + b
            for mw in (0, 2) if k < len(poses) else (0,):
                got = sp.raycast(pose, min_weight=mw)
                want = rr.raycast(rec_s, dims, origin, voxel, 4 * voxel, TINY, pose, min_weight=mw, z_near=sp.min_depth, z_far=sp.max_depth)[:3]
                full = rr.raycast(rec_d, dims, origin, voxel, 4 * voxel, TINY, pose, min_weight=mw, z_near=sp.min_depth, z_far=sp.max_depth)[:3]
                _assert_same(got, want, ("sparse", k, mw))
                _assert_same(dense.raycast(pose, min_weight=mw), full, ("dense", k, mw))
                differs += int(not np.array_equal(want[0], full[0]))                           # the refused bricks are seen to be missing
                print("view", k, "min_weight", mw, "refused before / after records on", a, "/", b, "rays; hits", int((want[0] > 0).sum()), "dense", int((full[0] > 0).sum()))
                if k >= len(poses):
                    continue                                                                    # (no frame was taken from behind)
                ev = sp.track_evaluate(k, pose, stride=1, max_dist=3 * voxel, min_weight=mw)
                ref = tr.sums(rec_s, dims, origin, voxel, 4 * voxel, TINY, frames[k], pose, stride=1, max_dist=3 * voxel, min_weight=mw,
                              min_depth=sp.min_depth, max_depth=sp.max_depth)
                ref_d = tr.sums(rec_d, dims, origin, voxel, 4 * voxel, TINY, frames[k], pose, stride=1, max_dist=3 * voxel, min_weight=mw,
                                min_depth=sp.min_depth, max_depth=sp.max_depth)
                assert (ev["n_src"], ev["n_corr"]) == (ref["n_src"], ref["n_corr"]) and 0 < ref["n_corr"] <= ref_d["n_corr"], (k, mw)
                fewer += int(ref["n_corr"] < ref_d["n_corr"])
                g, w = _sums_of(ev), np.concatenate([ref["A"], ref["b"], [ref["e"]]])
                assert np.all(np.abs(g - w) <= ref["n_corr"] * 2.0 ** -52 * ref["abs"]), (k, mw)
        print("rays that cross a refused brick before one with records:", before, "; after one:", after)
        assert before > 0 and after > 0 and differs >= len(poses) and fewer > 0


def test_both_readers_add_the_pending_free_space_counts_of_a_sparse_grid():
    """A sparse grid gives no records to a brick that only ever was free space: its count stays in the counter table after the fold and
    the readers add it (tsdf_cell.h: corner_record).  A nearly flat frame 0.45 in front of a wide camera leaves such bricks
    between the camera and the plane: fewer slots are handed out than bricks hold something, the rays march through the counted bricks
    at the free-space step, and the dense grid -- which folds every count into records -- gives the same bytes."""
    dims, origin, voxel = (32, 32, 48), (-0.16, -0.16, -0.40), 0.01
    cam = dict(width=64, height=48, fx=24.0, fy=24.0, cx=31.5, cy=23.5)          # wide: the grid's whole front face is in view from 0.16 away
    pose = (np.eye(3), np.array([0.0, 0.0, 0.56]))
    vv, uu = np.meshgrid(np.arange(cam["height"]), np.arange(cam["width"]), indexing="ij")
    frames = [(0.45 + 0.02 * np.sin(uu / 9.0) * np.cos(vv / 7.0)).astype(np.float32), np.full(uu.shape, 0.452, np.float32)]
    make = lambda pool: tl3d.FusionContext(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], n_slots=2,
                                           grid=tl3d.GridSpec(dims, origin, voxel, 4 * voxel, tl3d.CH_TSDF, pool_tsdf=pool))
    with make(0) as dense, make(72) as sp:                      # 72 of 96 bricks: slots are handed out on first touch
        for c in (dense, sp):
            for i, d in enumerate(frames):
                c.upload(i, d, None)
                c.integrate(i, pose)
        rec_d, rec_s = dense.download_grid(tl3d.CH_TSDF), sp.download_grid(tl3d.CH_TSDF)
        st = sp.stats()
        holding = int(_brick_state(rec_s).sum())
        print("bricks that hold something", holding, "; slots handed out", st["pool_slots_tsdf"], "; refused", st["pool_refused"])
        assert np.array_equal(rec_d, rec_s) and st["pool_refused"] == 0
        assert 0 < st["pool_slots_tsdf"] < holding                                             # the rest are counts without records
        view = (np.eye(3), np.array([0.01, -0.005, 0.56]))
        for mw in (0, 2, 3):                                                                    # 3: two observations are not enough
            got = sp.raycast(view, min_weight=mw)
            want = rr.raycast(rec_s, dims, origin, voxel, 4 * voxel, cam, view, min_weight=mw, z_near=sp.min_depth, z_far=sp.max_depth)[:3]
            _assert_same(got, want, ("sparse", mw))
            _assert_same(dense.raycast(view, min_weight=mw), want, ("dense", mw))
            assert ((want[0] > 0).sum() > 200) == (mw < 3) and ((want[0] > 0).sum() == 0) == (mw == 3)
            ev = sp.track_evaluate(0, view, stride=1, max_dist=3 * voxel, min_weight=mw)
            ref = tr.sums(rec_s, dims, origin, voxel, 4 * voxel, cam, frames[0], view, stride=1, max_dist=3 * voxel, min_weight=mw,
                          min_depth=sp.min_depth, max_depth=sp.max_depth)
            assert (ev["n_src"], ev["n_corr"]) == (ref["n_src"], ref["n_corr"]) and (ref["n_corr"] > 200) == (mw < 3), (mw, ref["n_corr"])
            g, w = _sums_of(ev), np.concatenate([ref["A"], ref["b"], [ref["e"]]])
            assert np.all(np.abs(g - w) <= max(1, ref["n_corr"]) * 2.0 ** -52 * ref["abs"]), mw
