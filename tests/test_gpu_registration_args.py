"""GPU: what the registration calls of the C API accept and what they refuse -- tl3d_icp_enqueue / _collect (a lane),
tl3d_icp_batch_enqueue / _collect, tl3d_icp_evaluate_pairs, tl3d_track_evaluate, tl3d_track_frame -- through the ctypes layer,
return codes only (and a message in tl3d_last_error).  The calls share their checks (csrc/api_register.hip) but do not agree on
everything: a lane and a batch take any positive max_dist, infinity included, and estimate the scale; the evaluation and the tracking
calls refuse max_dist >= 1e18, and tracking refuses estimate_scale.  This file pins both the common part and the differences.

The smallest context: an 8 x 8 camera, three slots -- 0: a frame with a normal map, 1: a frame without one, 2: empty -- and a grid of
one brick for the tracking calls.  Every refusal returns before any launch; every accepted run is collected."""
import ctypes as C
import math

import numpy as np
import pytest

from tl3d import _cabi as abi

pytestmark = pytest.mark.gpu

W = H = 8
SRC, TGT, EMPTY = 1, 0, 2            # slot 1 has no normal map: a source needs none
EYE3 = np.eye(3).reshape(9).copy()
ZERO3 = np.zeros(3)


@pytest.fixture(scope="module")
def ctx():
    lib = abi.load()
    cfg = abi.Config()
    cfg.abi_version = abi.ABI_VERSION
    cfg.width, cfg.height = W, H
    cfg.fx, cfg.fy, cfg.cx, cfg.cy = 8.0, 8.0, 3.5, 3.5
    cfg.min_depth, cfg.max_depth = 0.1, 10.0
    cfg.n_slots = 3
    cfg.channels = abi.CH_TSDF
    cfg.nx, cfg.ny, cfg.nz = 8, 8, 8
    cfg.origin = (C.c_double * 3)(-0.5, -0.5, 0.5)
    cfg.voxel_size, cfg.sdf_trunc = 0.125, 0.5
    h = C.c_void_p()
    abi.check(lib.tl3d_create(C.byref(cfg), 0, C.byref(h)))
    depth = np.ones((H, W), np.float32)
    for slot in (TGT, SRC):
        abi.check(lib.tl3d_upload_frame(h, slot, abi.ptr(depth), abi.DEPTH_F32_M, None))
    abi.check(lib.tl3d_build_normals(h, TGT, 1.0, 0.05))
    yield lib, h
    abi.check(lib.tl3d_destroy(h))


def _prm(**kw):
    return abi.IcpParams(int(kw.get("iters", 1)), int(kw.get("stride", 1)), float(kw.get("max_dist", 0.05)), 1e-6, 1e-9, 1e-4,
                         int(kw.get("estimate_scale", 0)), 0)


def _pairs(lst):
    arr = (abi.IcpPair * max(1, len(lst)))()
    for p, (s, t) in zip(arr, lst):
        p.slot_src, p.slot_tgt, p.scale_src = s, t, 1.0
        p.T_init[:] = np.eye(4).reshape(16).tolist()
    return arr


def _levels(lst):
    return (abi.IcpParams * max(1, len(lst)))(*[_prm(**kw) for kw in lst])


# the five calls; each returns the return code
def lane(c, lane_no=0, src=SRC, tgt=TGT, **kw):
    lib, h = c
    return lib.tl3d_icp_enqueue(h, lane_no, src, 1.0, tgt, None, C.byref(_prm(**kw)))


def lane_collect(c, lane_no=0):
    lib, h = c
    return lib.tl3d_icp_collect(h, lane_no, C.byref(abi.IcpResult()))


def batch(c, pairs=((SRC, TGT),), levels=({},), n_pairs=None, n_levels=None):
    lib, h = c
    return lib.tl3d_icp_batch_enqueue(h, _pairs(pairs), len(pairs) if n_pairs is None else n_pairs, _levels(levels),
                                      len(levels) if n_levels is None else n_levels)


def batch_collect(c, n_out=1):
    lib, h = c
    return lib.tl3d_icp_batch_collect(h, (abi.IcpResult * max(1, n_out))(), n_out)


def evaluate(c, pairs=((SRC, TGT),), stride=1, max_dist=0.05):
    lib, h = c
    return lib.tl3d_icp_evaluate_pairs(h, _pairs(pairs), len(pairs), stride, max_dist, (abi.IcpEval * max(1, len(pairs)))())


def track_evaluate(c, slot=SRC, stride=1, max_dist=0.05):
    lib, h = c
    return lib.tl3d_track_evaluate(h, slot, 1.0, abi.ptr(EYE3), abi.ptr(ZERO3), 1, stride, max_dist, C.byref(abi.IcpEval()))


def track_frame(c, slot=SRC, levels=({},), n_levels=None):
    lib, h = c
    return lib.tl3d_track_frame(h, slot, 1.0, abi.ptr(EYE3), abi.ptr(ZERO3), 1, _levels(levels), len(levels) if n_levels is None else n_levels,
                                C.byref(abi.IcpResult()))


def _is(c, rc, want, what):
    msg = c[0].tl3d_last_error()
    print(f"{what}: rc {rc} (want {want}){'' if rc == abi.OK else ' -- ' + msg.decode(errors='replace')}")
    assert rc == want, (what, rc, want, msg)
    if want != abi.OK:
        assert msg, what                                    # a refusal says why


def _lane_runs(c, what, **kw):
    _is(c, lane(c, **kw), abi.OK, f"lane enqueue, {what}")
    _is(c, lane_collect(c), abi.OK, f"lane collect, {what}")


def _batch_runs(c, what, **kw):
    _is(c, batch(c, levels=(kw,)), abi.OK, f"batch enqueue, {what}")
    _is(c, batch_collect(c), abi.OK, f"batch collect, {what}")


def test_plain_arguments_are_accepted_by_every_call(ctx):
    _lane_runs(ctx, "plain")
    _batch_runs(ctx, "plain")
    _is(ctx, evaluate(ctx), abi.OK, "evaluate, plain")
    _is(ctx, track_evaluate(ctx), abi.OK, "track evaluate, plain")
    _is(ctx, track_frame(ctx), abi.OK, "track frame, plain")
    _is(ctx, track_frame(ctx, levels=({}, dict(stride=2), dict(iters=0), {})), abi.OK, "track frame, TL3D_ICP_MAX_LEVELS levels")
    _is(ctx, batch(ctx, levels=({}, dict(stride=2), dict(iters=0), {})), abi.OK, "batch enqueue, TL3D_ICP_MAX_LEVELS levels")
    _is(ctx, batch_collect(ctx), abi.OK, "batch collect")


@pytest.mark.parametrize("field, value", [("iters", -1), ("iters", 1001), ("stride", 0), ("max_dist", 0.0), ("max_dist", math.nan)])
def test_what_every_call_refuses(ctx, field, value):
    kw = {field: value}
    what = f"{field} {value}"
    _is(ctx, lane(ctx, **kw), abi.E_INVALID, f"lane enqueue, {what}")
    _is(ctx, batch(ctx, levels=(kw,)), abi.E_INVALID, f"batch enqueue, {what}")
    _is(ctx, batch(ctx, levels=({}, kw)), abi.E_INVALID, f"batch enqueue, second level, {what}")
    _is(ctx, track_frame(ctx, levels=(kw,)), abi.E_INVALID, f"track frame, {what}")
    _is(ctx, track_frame(ctx, levels=({}, kw)), abi.E_INVALID, f"track frame, second level, {what}")
    if field != "iters":                                    # the one-pass calls take no iteration count
        _is(ctx, evaluate(ctx, **kw), abi.E_INVALID, f"evaluate, {what}")
        _is(ctx, track_evaluate(ctx, **kw), abi.E_INVALID, f"track evaluate, {what}")
    _is(ctx, lane_collect(ctx), abi.E_STATE, "lane collect: the refused enqueue left nothing in flight")
    _is(ctx, batch_collect(ctx), abi.E_STATE, "batch collect: the refused enqueue left nothing in flight")


@pytest.mark.parametrize("max_dist", [1e18, math.inf])
def test_a_huge_gate_is_taken_by_lane_and_batch_only(ctx, max_dist):
    what = f"max_dist {max_dist}"
    _lane_runs(ctx, what, max_dist=max_dist)
    _batch_runs(ctx, what, max_dist=max_dist)
    _is(ctx, evaluate(ctx, max_dist=max_dist), abi.E_INVALID, f"evaluate, {what}")
    _is(ctx, track_evaluate(ctx, max_dist=max_dist), abi.E_INVALID, f"track evaluate, {what}")
    _is(ctx, track_frame(ctx, levels=(dict(max_dist=max_dist),)), abi.E_INVALID, f"track frame, {what}")


def test_estimate_scale_is_refused_by_tracking_only(ctx):
    _lane_runs(ctx, "estimate_scale 1", estimate_scale=1)
    _batch_runs(ctx, "estimate_scale 1", estimate_scale=1)
    _is(ctx, track_frame(ctx, levels=(dict(estimate_scale=1),)), abi.E_INVALID, "track frame, estimate_scale 1")


def test_the_number_of_levels_and_of_pairs(ctx):
    for n in (0, abi.ICP_MAX_LEVELS + 1):
        levels = ({},) * (abi.ICP_MAX_LEVELS + 1)
        _is(ctx, batch(ctx, levels=levels, n_levels=n), abi.E_INVALID, f"batch enqueue, n_levels {n}")
        _is(ctx, track_frame(ctx, levels=levels, n_levels=n), abi.E_INVALID, f"track frame, n_levels {n}")
    _is(ctx, evaluate(ctx, pairs=()), abi.OK, "evaluate, n_pairs 0")
    _is(ctx, batch(ctx, pairs=()), abi.E_INVALID, "batch enqueue, n_pairs 0")


def test_slots(ctx):
    for bad in (-1, 3):                                     # out of range [0, 3)
        for src, tgt in ((bad, TGT), (SRC, bad)):
            what = f"slots ({src}, {tgt})"
            _is(ctx, lane(ctx, src=src, tgt=tgt), abi.E_INVALID, f"lane enqueue, {what}")
            _is(ctx, batch(ctx, pairs=((SRC, TGT), (src, tgt))), abi.E_INVALID, f"batch enqueue, {what}")
            _is(ctx, evaluate(ctx, pairs=((SRC, TGT), (src, tgt))), abi.E_INVALID, f"evaluate, {what}")
        _is(ctx, track_evaluate(ctx, slot=bad), abi.E_INVALID, f"track evaluate, slot {bad}")
        _is(ctx, track_frame(ctx, slot=bad), abi.E_INVALID, f"track frame, slot {bad}")
    # a slot without a frame, as source and as target; a target without a normal map (slot 1: as a source it needs none)
    for src, tgt in ((EMPTY, TGT), (TGT, EMPTY), (TGT, SRC)):
        what = f"slots ({src}, {tgt})"
        _is(ctx, lane(ctx, src=src, tgt=tgt), abi.E_STATE, f"lane enqueue, {what}")
        _is(ctx, batch(ctx, pairs=((SRC, TGT), (src, tgt))), abi.E_STATE, f"batch enqueue, {what}")
        _is(ctx, evaluate(ctx, pairs=((SRC, TGT), (src, tgt))), abi.E_STATE, f"evaluate, {what}")
    _is(ctx, track_evaluate(ctx, slot=EMPTY), abi.E_STATE, "track evaluate, a slot without a frame")
    _is(ctx, track_frame(ctx, slot=EMPTY), abi.E_STATE, "track frame, a slot without a frame")
    _is(ctx, batch_collect(ctx), abi.E_STATE, "batch collect: nothing in flight")


def test_lanes(ctx):
    for bad in (-1, abi.ICP_LANES):
        _is(ctx, lane(ctx, lane_no=bad), abi.E_INVALID, f"lane enqueue, lane {bad}")
        _is(ctx, lane_collect(ctx, lane_no=bad), abi.E_INVALID, f"lane collect, lane {bad}")
    _is(ctx, lane_collect(ctx, lane_no=1), abi.E_STATE, "collect on a lane never used")
    _is(ctx, lane(ctx, lane_no=1), abi.OK, "lane enqueue")
    _is(ctx, lane(ctx, lane_no=1), abi.E_STATE, "enqueue on a busy lane")
    _is(ctx, lane_collect(ctx, lane_no=1), abi.OK, "lane collect")
    _is(ctx, lane_collect(ctx, lane_no=1), abi.E_STATE, "collect on an idle lane")


def test_a_batch_in_flight(ctx):
    _is(ctx, batch_collect(ctx), abi.E_STATE, "batch collect with no batch in flight")
    _is(ctx, batch(ctx, pairs=((SRC, TGT), (TGT, TGT))), abi.OK, "batch enqueue, two pairs")
    _is(ctx, batch(ctx), abi.E_STATE, "a second batch enqueue")
    _is(ctx, evaluate(ctx), abi.E_STATE, "evaluate while a batch is uncollected")
    _is(ctx, track_evaluate(ctx), abi.E_STATE, "track evaluate while a batch is uncollected")
    _is(ctx, track_frame(ctx), abi.E_STATE, "track frame while a batch is uncollected")
    for n_out in (1, 3):
        _is(ctx, batch_collect(ctx, n_out=n_out), abi.E_INVALID, f"batch collect, n_out {n_out} for two pairs")
    _is(ctx, batch_collect(ctx, n_out=2), abi.OK, "batch collect")
    _is(ctx, batch_collect(ctx, n_out=2), abi.E_STATE, "batch collect, again")
    _is(ctx, evaluate(ctx), abi.OK, "evaluate, after the collect")
