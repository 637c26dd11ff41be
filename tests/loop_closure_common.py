"""Shared by the loop-closure tests (CPU and GPU): the closed orbit of the issue's experiment and its error measures.

The orbit: synth.object_scene(True) seen from synth.orbit_poses(N + 1, 1.0, 360 / N) -- frame N repeats frame 0's view --, depth
noise sigma with seeds 100 + i.  Errors are against the analytic poses in the gauge cam0 = I."""
import numpy as np

from tl3d import synth

ORBIT_CAM = dict(width=320, height=240, fx=300.0, fy=300.0, cx=160.0, cy=120.0)
LEVELS = ((10, 4, 0.20), (15, 2, 0.05))               # (iterations, stride, gate): the pipeline's default schedule
GATE, STRIDE = 0.05, 2                                 # where an edge's weight is evaluated: the final level's


def orbit_truth(n_loop):
    """[N + 1, 4, 4] analytic world -> camera poses in the gauge cam0 = I."""
    poses = synth.orbit_poses(n_loop + 1, 1.0, 360.0 / n_loop)
    T = np.tile(np.eye(4), (len(poses), 1, 1))
    for k, (R, t) in enumerate(poses):
        T[k, :3, :3], T[k, :3, 3] = R, np.asarray(t).reshape(3)
    return poses, T @ np.linalg.inv(T[0])


def orbit_frames(n_loop, sigma, cam=ORBIT_CAM, xp=np, device=None):
    poses, truth = orbit_truth(n_loop)
    scene = synth.object_scene(True)
    frames = [synth.render(scene, p, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], xp=xp, device=device,
                           noise_sigma=sigma, seed=100 + i) for i, p in enumerate(poses)]
    return frames, truth


def pose_error(T, T_true):
    """(camera-centre error in mm, rotation error in degrees) of one 4x4 pose."""
    c = -T[:3, :3].T @ T[:3, 3]
    ct = -T_true[:3, :3].T @ T_true[:3, 3]
    cosang = np.clip(0.5 * (np.trace(T[:3, :3] @ T_true[:3, :3].T) - 1.0), -1.0, 1.0)
    # the sine form: arccos loses the angles this test is about (1e-3 degrees) to rounding
    s = 0.5 * np.linalg.norm((T[:3, :3] @ T_true[:3, :3].T) - (T[:3, :3] @ T_true[:3, :3].T).T, ord="fro") / np.sqrt(2.0)
    return float(np.linalg.norm(c - ct)) * 1e3, float(np.degrees(np.arctan2(s, cosang)))


def mean_centre_error(Ts, truth):
    return float(np.mean([pose_error(a, b)[0] for a, b in zip(Ts, truth)]))


def sym6(a21):
    A = np.zeros((6, 6))
    iu = np.triu_indices(6)
    A[iu] = np.asarray(a21)[:21]
    return A + np.triu(A, 1).T


def check_loop_criteria(chain, optimised, direct, truth, say=print):
    """The three criteria of the issue, on [N + 1, 4, 4] chain / optimised poses and the direct registration Z of pair (0, N)
    (the pose of frame N it implies in the gauge cam0 = I is Z itself).  Prints every figure before it asserts."""
    n = len(truth) - 1
    ch_mm, ch_deg = pose_error(chain[n], truth[n])
    di_mm, di_deg = pose_error(direct, truth[n])
    op_mm, op_deg = pose_error(optimised[n], truth[n])
    m_ch, m_op = mean_centre_error(chain, truth), mean_centre_error(optimised, truth)
    say(f"frame {n}: chain {ch_mm:.4f} mm / {ch_deg:.5f} deg, direct pair {di_mm:.4f} mm / {di_deg:.5f} deg, "
        f"optimised {op_mm:.4f} mm / {op_deg:.5f} deg; mean centre error {m_ch:.4f} -> {m_op:.4f} mm")
    # a condition on the input: the loop's two ends registered directly are at least 4x closer to the truth than the chain's end
    assert di_mm * 4.0 <= ch_mm, (di_mm, ch_mm)
    # the optimiser spreads the loop's residual over all edges and cannot beat the edge it is given: margin 2x
    assert op_mm <= 2.0 * di_mm, (op_mm, di_mm)
    assert op_deg <= 2.0 * di_deg, (op_deg, di_deg)
    assert m_op < m_ch, (m_op, m_ch)
    return dict(chain=(ch_mm, ch_deg), direct=(di_mm, di_deg), optimised=(op_mm, op_deg), mean=(m_ch, m_op))
