"""CPU: the numpy restatement of point-to-SDF tracking (tests/track_reference.py) held to account -- its
normal equations against central differences (which fixes the sign convention), convergence on a rendered frame, a degenerate
volume, and the whole tracking stage on an open arc with the C oracle as the integrator."""
import numpy as np
import pytest

import raycast_reference as rr
import track_reference as tr
from track_common import (ARC, CRAFTED_DIMS, CRAFTED_ORIGIN, CRAFTED_TRUNC, CRAFTED_VOXEL, LEVELS, SMALL, arc_frames, centre_errors_mm,
                          crafted_depth, crafted_records, crafted_views, fused_model, novel_pose, offset_pose, pose_delta)
from tl3d import synth

CRAFTED = (CRAFTED_DIMS, CRAFTED_ORIGIN, CRAFTED_VOXEL, CRAFTED_TRUNC)


def _frozen_residuals(det, T, origin, voxel, trunc):
    """fp64 residuals of the correspondences of `det` at pose T: the kernel's function -- its rounded constants taken as exact --
    with every sample kept in the cell it was found in (the cell's trilinear polynomial, extended), so that it is smooth in T"""
    R, t = T[:3, :3], T[:3, 3]
    ivs = float(np.float32(1.0 / voxel))
    org = np.asarray(origin, np.float64).astype(np.float32).astype(np.float64)
    cg = (-(R.T @ t) - org) * ivs - 0.5
    x = cg[None, :] + (det["p"].astype(np.float64) @ R) * ivs             # rows: R^T p_c
    f = x - det["ijk"]
    tc = det["tc"].astype(np.float64)
    lerp = lambda a, b, w: a + w * (b - a)
    c00, c10 = lerp(tc[:, 0], tc[:, 1], f[:, 0]), lerp(tc[:, 2], tc[:, 3], f[:, 0])
    c01, c11 = lerp(tc[:, 4], tc[:, 5], f[:, 0]), lerp(tc[:, 6], tc[:, 7], f[:, 0])
    return float(np.float32(trunc)) * lerp(lerp(c00, c10, f[:, 1]), lerp(c01, c11, f[:, 1]), f[:, 2])


@pytest.mark.parametrize("view", [0, 1])
def test_normal_equations_match_central_differences(view):
    """b is minus the gradient of e / 2 under M <- se3_apply(y) M, and A is J^T J of the central-difference Jacobian dr / dy = -J
    (Gauss-Newton's A leaves out sum r d2r, so it is compared through the Jacobian, not through second differences of e)."""
    rec = crafted_records()
    pose = crafted_views()[view]
    depth = crafted_depth(rec, pose)
    off = offset_pose(pose, 0.5, CRAFTED_VOXEL)                            # 1 voxel, 0.5 degrees off: residuals of some millimetres
    s = tr.sums(rec, *CRAFTED, SMALL, depth, off, stride=1, max_dist=3 * CRAFTED_VOXEL, min_weight=0, detail=True)
    assert s["n_corr"] > 500
    T = tr.pose_matrix(off)
    r0 = _frozen_residuals(s, T, CRAFTED_ORIGIN, CRAFTED_VOXEL, CRAFTED_TRUNC)
    assert np.abs(r0 - s["r"]).max() < 2e-5 * CRAFTED_TRUNC                # the f32 residuals are the fp64 ones to f32 rounding of x
    h = 1e-6
    Jy = np.zeros((s["n_corr"], 6))
    grad = np.zeros(6)
    for a in range(6):
        y = np.zeros(6)
        y[a] = h
        rp = _frozen_residuals(s, tr.se3_apply(y, T), CRAFTED_ORIGIN, CRAFTED_VOXEL, CRAFTED_TRUNC)
        rm = _frozen_residuals(s, tr.se3_apply(-y, T), CRAFTED_ORIGIN, CRAFTED_VOXEL, CRAFTED_TRUNC)
        Jy[:, a] = (rp - rm) / (2 * h)
        grad[a] = 0.5 * (rp @ rp - rm @ rm) / (2 * h)
    A, b = tr.sym6(s["A"]), s["b"]
    eb = np.abs(grad + b).max() / np.abs(b).max()
    eA = np.abs(Jy.T @ Jy - A).max() / np.abs(A).max()
    eJ = np.abs(Jy + s["J"]).max()
    print(f"view {view}: n_corr {s['n_corr']}, |grad(e/2) + b| / |b| = {eb:.2e}, |JyT Jy - A| / |A| = {eA:.2e}, max |dr/dy + J| = {eJ:.2e}")
    assert eb < 1e-5
    assert eA < 1e-5
    assert np.linalg.norm(grad - b) > np.linalg.norm(b)                    # the other sign is far off: b is not near zero here


def test_a_rendered_frame_is_recovered():
    """The bars are the existing frame-to-model test's (0.1 voxel, 0.1 degrees).  The model is the ray-cast tests' recipe (6 frames,
    8 degrees apart) at FINE_VOXEL: point-to-SDF carries a bias of its own, from cells next to a silhouette whose far corners saw the
    background (free space) -- about 0.09 voxel here, 0.15 voxel at 25 mm, whatever the start."""
    scene, poses, orc, spec = fused_model()
    truth = novel_pose()
    depth, _ = synth.render(scene, truth, SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], seed=50)
    start = offset_pose(truth, 0.5, 0.010)
    res = tr.track(orc.tsdf, *spec, SMALL, depth, start, LEVELS)
    d0 = pose_delta(tr.pose_matrix(start), tr.pose_matrix(truth), spec[2])
    d1 = pose_delta(res["T"], tr.pose_matrix(truth), spec[2])
    print(f"start {d0[0]:.3f} voxel / {d0[1]:.3f} deg -> {d1[0]:.4f} voxel / {d1[1]:.4f} deg; fitness {res['fitness']:.3f}, rmse "
          f"{res['rmse'] * 1e3:.3f} mm, {res['iters_run']} iterations, status {res['status']}")
    assert d0[0] > 0.9 and d0[1] > 0.4
    assert res["status"] in (0, 1) and res["n_corr"] > 500
    assert d1[0] < 0.1 and d1[1] < 0.1


def test_a_single_plane_leaves_what_it_does_not_observe_at_the_prior():
    dims, voxel = (64, 64, 64), 0.02
    origin, trunc = tuple(-0.5 * d * voxel for d in dims), 4 * voxel
    nrm = np.array([1.0, 2.0, 8.0]) / np.linalg.norm([1.0, 2.0, 8.0])
    ii, jj, kk = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    p = np.stack([origin[a] + (g + 0.5) * voxel for a, g in enumerate((ii, jj, kk))], axis=-1)
    sdf = -(p @ nrm - 0.1)                                                 # positive towards the camera at z = -2
    rec = rr.records_from_volume(np.rint(np.clip(sdf / trunc, -1.0, 1.0) * 32767.0).astype(np.int64), np.ones(dims, np.int64))
    pose = (np.eye(3), np.array([0.0, 0.0, 2.0]))
    cam = dict(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5)
    depth = rr.raycast(rec, dims, origin, voxel, trunc, cam, pose)[0]
    assert (depth > 0).sum() > 1000
    start = offset_pose(pose, 0.5, 0.010)
    T0 = tr.pose_matrix(start)
    # one step: the update has no component along what a plane does not observe -- the in-plane translations and the rotation
    # about the normal (camera frame: n_c = R n): their eigenvalues are the damping's, far below the cutoff.  The records hold the
    # field to 1 / 32767 of the truncation, i.e. a gradient (0.25 per voxel) to 1.2e-4 of itself per sample: the kept eigenvectors
    # lean into the unobserved directions by less than that
    s = tr.sums(rec, dims, origin, voxel, trunc, cam, depth, start, stride=1, max_dist=0.05, min_weight=1)
    assert s["n_corr"] > 500
    x = tr.solve(s["A"], s["b"], 1e-6, 1e-4)
    nc = T0[:3, :3] @ nrm
    t1 = np.cross(nc, [1.0, 0.0, 0.0]); t1 /= np.linalg.norm(t1)
    t2 = np.cross(nc, t1)
    leak = max(abs(x[:3] @ nc), abs(x[3:] @ t1), abs(x[3:] @ t2))
    print(f"step |x| {np.linalg.norm(x):.3e}, component along unobserved directions {leak:.3e}")
    assert np.linalg.norm(x) > 1e-3 and leak < 1e-4 * np.linalg.norm(x)
    # the whole registration: the plane is found (residual gone), and the pose moved only where the plane pulled it.  The
    # unobserved directions turn with the camera from one iteration to the next, by at most the 0.5 degrees of the start: what
    # leaks into them is second order, below sin(0.5 deg) = 0.9 % of the motion; 2 % is the bar.
    res = tr.track(rec, dims, origin, voxel, trunc, cam, depth, start, [dict(iters=15, stride=1, max_dist=0.05, damping=1e-6, eps=1e-9, eig_rel=1e-4)])
    assert res["status"] in (0, 1) and res["rmse"] < 0.05 * voxel
    D = res["T"] @ np.linalg.inv(T0)
    w = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2.0
    moved = np.linalg.norm(np.concatenate([w, D[:3, 3]]))
    leak = max(abs(w @ nc), abs(D[:3, 3] @ t1), abs(D[:3, 3] @ t2))
    print(f"registration moved {moved:.3e}, along unobserved directions {leak:.3e}, rmse {res['rmse'] * 1e3:.4f} mm")
    assert moved > 1e-3 and leak < 0.02 * moved


def arc_chain_and_tracked(arc=ARC, say=print, min_fitness=0.5):
    """The whole stage on the CPU: chain from the C oracle's ICP (as tests/test_posegraph_cpu.py builds it), then every frame
    registered against the model the oracle fused from the frames before it (numpy reference), then integrated at its pose.
    Returns (truth, chain, tracked) as [n, 4, 4] world->camera poses, frame 0 at its analytic pose."""
    from oracle import c_oracle
    poses, frames = arc_frames(arc)
    dims, voxel, centre = arc["dims"], arc["voxel"], arc["centre"]
    origin = tuple(centre[i] - 0.5 * dims[i] * voxel for i in range(3))
    orc = c_oracle.Oracle(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], 0.1, 50.0, dims=dims, origin=origin,
                          voxel_size=voxel, sdf_trunc=4 * voxel)
    maps = [orc.normals_smooth(d, radius=1) for d, _ in frames]
    truth = np.stack([tr.pose_matrix(p) for p in poses])
    chain, guess = [truth[0]], np.eye(4)
    for k in range(len(frames) - 1):
        T, res = guess, None
        for lv in LEVELS:
            res = orc.icp(maps[k][0], maps[k + 1][1], T_init=T, iters=lv["iters"], stride=lv["stride"], max_dist=lv["max_dist"], damping=1e-6,
                          eps=1e-7, eig_rel=1e-4)
            T = res["T"]
            if res["status"] == 2 or res["n_corr"] < 8:
                break
        assert res["status"] != 2
        guess = res["T"]
        chain.append(res["T"] @ chain[-1])
    chain = np.stack(chain)
    spec = (dims, origin, voxel, 4 * voxel)
    tracked, lost = [chain[0]], 0
    orc.tsdf_integrate(frames[0][0], chain[0][:3, :3], chain[0][:3, 3])
    for k in range(1, len(frames)):
        M0 = (chain[k] @ np.linalg.inv(chain[k - 1])) @ tracked[-1]
        res = tr.track(orc.tsdf, *spec, SMALL, frames[k][0], (M0[:3, :3], M0[:3, 3]), LEVELS)
        ok = res["status"] != 2 and res["fitness"] >= min_fitness
        say(f"  frame {k}: fitness {res['fitness']:.3f}, rmse {res['rmse'] * 1e3:.2f} mm, {res['iters_run']} iterations, status {res['status']}")
        lost += not ok
        M = res["T"] if ok else M0
        tracked.append(M)
        orc.tsdf_integrate(frames[k][0], M[:3, :3], M[:3, 3])
    say(f"arc of {len(frames)} frames: {lost} lost")
    return truth, chain, np.stack(tracked), lost


def test_tracking_an_open_arc_beats_the_chain():
    truth, chain, tracked, lost = arc_chain_and_tracked()
    e_chain, e_track = centre_errors_mm(chain, truth), centre_errors_mm(tracked, truth)
    print(f"mean camera-centre error: chain {e_chain.mean():.4f} mm, tracked {e_track.mean():.4f} mm; last frame: chain {e_chain[-1]:.4f} mm, "
          f"tracked {e_track[-1]:.4f} mm")
    assert lost == 0
    assert e_track.mean() < e_chain.mean()
