"""Shared by tests/test_gpu_registration_gates.py and its CPU companion: the scenes that sit on the count thresholds of the step
behind a pass of tracking, colour and cloud registration (csrc/kernels_regstep.hip), and the three numpy references' runs on them,
each computed once per process.  Not a test.

Two thresholds.  An ITERATION needs 6 correspondences (tracking: 8; tests/test_gpu_icp_degenerate.py pins that one), else the run
fails: status 2, no update.  A LEVEL that ends with fewer than 8 is the run's last.  The references state both rules
(track_reference.track, rgbd_reference.register, cloud_register_reference.register); a scene here is a handful of pixels or points
chosen so that the reference's count lands on a threshold's either side, which every user of a scene asserts of the reference.

The end-of-level schedule is two levels with the same stride and gate: the first makes ONE update (tracking: none -- its iterations
need the 8 correspondences the level's end asks for, so only a level without updates ends below 8 unfailed), the second up to
LEVEL2_ITERS.  With 6 or 7 correspondences at the end of the first level the second must not run: the result is the one-level run's,
bit for bit.  With 8 it runs: iters_run is the second level's."""
import functools

import numpy as np

import cloud_register_common as cc
import cloud_register_reference as cr
import icp_degenerate_common as dc
import rgbd_common as rc
import rgbd_reference as rref
import track_reference as tr

PARITY = cc.PARITY                                             # the project's ICP parity bar: a run's pose against its reference
LEVEL2_ITERS = 3
COUNTS = (6, 7, 8)


def hole_around_cutoff(M, damping, eig_rel):
    """no eigenvalue of the damped system within a factor 2 of the cutoff: the device and the reference keep the same directions
    (the condition tests/test_icp_degenerate_reference_cpu.py asks of every one-step comparison)"""
    lam, _, _ = dc.spectrum(np.asarray(M), damping, eig_rel)
    cut = eig_rel * lam.max()
    return bool(np.all((lam > 2.0 * cut) | (lam < 0.5 * cut)))


def check_schedule_refs(one, two, n, updates):
    """What a scene of the end-of-level schedule has to be, asserted of the reference's one-level and two-level runs: level one makes
    `updates` updates unfailed and ends with exactly n correspondences; below 8 the second level changes nothing, with 8 it runs to
    its last iteration and moves the pose by more than the parity bar can hide."""
    assert (one["status"], one["iters_run"], one["n_corr"], one["n_src"]) == (0, updates, n, n), (n, one)
    if n < 8:
        assert (two["status"], two["iters_run"], two["n_corr"]) == (0, updates, n) and np.array_equal(two["T"], one["T"]), (n, two)
    else:
        assert (two["status"], two["iters_run"]) == (0, LEVEL2_ITERS) and two["n_corr"] >= 8, (n, two)
        assert np.linalg.norm(two["T"] - one["T"]) > 2.0 * PARITY, n


def same_result(a, b):
    """two results of the device, bit for bit"""
    return np.array_equal(a["T"], b["T"]) and all(a[k] == b[k] for k in ("scale", "rmse", "fitness", "n_corr", "n_src", "iters_run", "status"))


# ---- cloud: N source points on a box of a few hundred target points --------------------------------------------------------------
CLOUD_T0 = cc.pose((3, 1, 2), 2.0, (0.015, -0.01, 0.02))       # the planted motion: 2 degrees and 2.7 cm; the runs start at the identity
CLOUD_LV = dict(stride=1, max_dist=0.2, damping=1e-6, eps=1e-12, eig_rel=1e-4)
CLOUD_KINDS = ("point", "plane", "point_scale")                # point-to-point, point-to-plane, point-to-point with scale


@functools.lru_cache(maxsize=None)
def cloud_case(n, kind):
    """n source points in general position -- moved copies of target points, taken from the six faces in turn --, all inside the
    gate of a 300-point box (of a seed whose first pass has no eigenvalue near the cutoff with 6, 7 or 8 points, point-to-plane
    too, where six or seven rows leave one direction weak: users assert hole_around_cutoff)"""
    tgt, nrm = cc.box_samples(300, 34)
    by_face = [np.nonzero(nrm @ np.array([1.0, 2.0, 3.0]) == k)[0] for k in (1, -2, 3, -1, 2, -3)]
    pick = [by_face[i % 6][i // 6] for i in range(n)]
    return dict(src=cc.unmove(tgt[pick], CLOUD_T0), tgt=tgt, normals=nrm if kind == "plane" else None, estimate_scale=kind == "point_scale")


def cloud_levels(iters):
    return [dict(CLOUD_LV, iters=it) for it in iters]


@functools.lru_cache(maxsize=None)
def cloud_ref(n, kind, iters):
    c = cloud_case(n, kind)
    return cr.register(c["src"], c["tgt"], c["normals"], levels=cloud_levels(iters), estimate_scale=c["estimate_scale"])


def cloud_first_system(n, kind):
    """(M, number of correspondences) of the first pass: for hole_around_cutoff"""
    c = cloud_case(n, kind)
    E = cr.evaluate(c["src"], c["tgt"], c["normals"], stride=1, max_dist=CLOUD_LV["max_dist"], with_scale=c["estimate_scale"])
    k = 7 if c["estimate_scale"] else 6
    return cr.full(E["A"])[:k, :k], E["n_corr"]


# ---- colour: the control pair with N source pixels -------------------------------------------------------------------------------
RGBD_WEIGHTS = (0.0, rc.WEIGHT)
RGBD_LV = dict(stride=2, max_dist=dc.PRM["max_dist"], damping=dc.PRM["damping"], eps=1e-12, eig_rel=dc.PRM["eig_rel"], photo_gate=rc.GATE)


@functools.lru_cache(maxsize=None)
def rgbd_frame(n):
    """(source depth, source colours): the control pair's source zeroed except at the first n of icp_degenerate_common.PIXELS (n = 5
    and 6: its pixels5 / pixels6), with the control pair's colours"""
    f = rc.pairs()["control"]
    src = np.zeros_like(f["src"])
    for u, v in dc.PIXELS[:n]:
        src[v, u] = f["src"][v, u]
    if n in (5, 6):
        assert np.array_equal(src, dc.pixel_frames()[f"pixels{n}"]["src"])
    return src, f["src_bgr"]


def rgbd_levels(iters, weight):
    return [dict(RGBD_LV, iters=it, photo_weight=weight) for it in iters]


@functools.lru_cache(maxsize=None)
def rgbd_maps(n):
    """what rgbd_reference reads of the n-pixel pair (normal smoothing off): source depth, target normals, the two intensity maps"""
    f = rc.pairs()["control"]
    src, bgr = rgbd_frame(n)
    nmap = dc.oracle().normals(f["tgt"])
    return src, nmap, rref.intensity_map(src, bgr, rc.RADIUS, rc.JUMP), rref.intensity_map(f["tgt"], f["tgt_bgr"], rc.RADIUS, rc.JUMP)


def rgbd_T0():
    return rc.pairs()["control"]["T_init"]


@functools.lru_cache(maxsize=None)
def rgbd_ref(n, iters, weight):
    return rref.register(rc.CAM, *rgbd_maps(n), rgbd_T0(), rgbd_levels(iters, weight))


def rgbd_first_system(n, weight):
    s = rref.sums(rc.CAM, *rgbd_maps(n), rgbd_T0(), stride=RGBD_LV["stride"], max_dist=RGBD_LV["max_dist"], photo_gate=rc.GATE)
    return tr.sym6(rref.joint(s, weight)[0]), s


# ---- tracking: the plane's frame with N pixels ------------------------------------------------------------------------------------
TRACK_LV = dict(dc.TRACK_PRM, stride=2, eps=1e-12)


def track_levels(iters):
    return [dict(TRACK_LV, iters=it) for it in iters]


@functools.lru_cache(maxsize=None)
def track_ref(n, iters):
    c = dc.track_cases()["track_plane"]
    return tr.track(c["rec"], *dc.T_SPEC, dc.CAM, dc.track_pixel_depth(n), c["start"], track_levels(iters))
