"""Shared by the tracking tests (CPU and GPU): the crafted volume of the ray-cast tests, the open arc of the whole-stage
experiment, small pose helpers.  Not a test."""
import numpy as np

import raycast_reference as rr
import track_reference as tr
from tl3d import synth

SMALL = dict(width=160, height=120, fx=140.0, fy=140.0, cx=79.5, cy=59.5)
LEVELS = [dict(iters=10, stride=4, max_dist=0.20, damping=1e-6, eps=1e-7, eig_rel=1e-4),
          dict(iters=15, stride=2, max_dist=0.05, damping=1e-6, eps=1e-7, eig_rel=1e-4)]      # the chain's default schedule

# the crafted grid of tests/test_gpu_raycast.py: 40 x 24 x 72 at 20 mm around (0.3, 0.2, 0.7)
CRAFTED_DIMS, CRAFTED_VOXEL, CRAFTED_CENTRE = (40, 24, 72), 0.02, (0.3, 0.2, 0.7)
CRAFTED_ORIGIN = tuple(CRAFTED_CENTRE[i] - 0.5 * CRAFTED_DIMS[i] * CRAFTED_VOXEL for i in range(3))
CRAFTED_TRUNC = 4 * CRAFTED_VOXEL


def crafted_records(dims=CRAFTED_DIMS, voxel=CRAFTED_VOXEL, origin=CRAFTED_ORIGIN):
    """{sum, weight} records: spheres cut by the grid's faces, weights 1..3, an unobserved slab and column, truncated voxels"""
    rng = np.random.default_rng(11)
    ii, jj, kk = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    p = np.stack([origin[a] + (g + 0.5) * voxel for a, g in enumerate((ii, jj, kk))], axis=-1)
    s1 = np.linalg.norm(p - np.array([0.1, 0.05, 0.6]), axis=-1) - 0.17
    s2 = np.linalg.norm(p - np.array([0.45, 0.2, 0.9]), axis=-1) - 0.3         # cut by the upper x and y faces
    s3 = np.linalg.norm(p - np.array([0.2, 0.1, 1.4]), axis=-1) - 0.2          # cut by the upper z face
    sdf = np.minimum(np.minimum(s1, s2), s3)
    t = np.clip(sdf / (3 * voxel), -1.0, 1.0)
    w = rng.integers(1, 4, size=dims)
    s = np.rint(t * 32767.0).astype(np.int64) * w
    far = np.abs(sdf) > 3.5 * voxel
    s[far] = np.sign(sdf[far]).astype(np.int64) * 32767 * w[far]
    w[:, :, 10:13] = 0                                                         # unobserved slab across a brick face
    s[:, :, 10:13] = 0
    w[5:9, 3:7, :] = 0
    s[5:9, 3:7, :] = 0
    return rr.records_from_volume(s, w)


def crafted_views():
    c, s = np.cos(0.3), np.sin(0.3)
    return [(np.eye(3), np.array([-0.3, -0.2, 0.2])),                          # camera at z = -0.2, looking along +z
            (np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]]), np.array([-0.2, -0.2, 0.3])),
            (np.eye(3), np.array([-0.05, -0.1, -1.0]))]                         # inside the volume, in front of the third sphere


def crafted_depth(rec, pose, cam=SMALL):
    """the depth image a camera at `pose` has of the crafted model: its own ray cast (numpy)"""
    return rr.raycast(rec, CRAFTED_DIMS, CRAFTED_ORIGIN, CRAFTED_VOXEL, CRAFTED_TRUNC, cam, pose, min_weight=0, z_near=0.1, z_far=50.0)[0]


def offset_pose(pose, rot_deg, trans, axis=(0.3, -0.5, 0.8), direction=(0.6, -0.3, 0.74)):
    """pose moved by rot_deg about `axis` and by `trans` metres along `direction` (camera frame, se3_apply)"""
    a = np.asarray(axis, np.float64)
    d = np.asarray(direction, np.float64)
    y = np.concatenate([np.radians(rot_deg) * a / np.linalg.norm(a), trans * d / np.linalg.norm(d)])
    T = tr.se3_apply(y, tr.pose_matrix(pose))
    return T[:3, :3].copy(), T[:3, 3].copy()


def pose_delta(T, T_ref, voxel):
    """(translation difference in voxels, rotation difference in degrees) of two 4x4 poses"""
    dR = T[:3, :3] @ T_ref[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(T[:3, 3] - T_ref[:3, 3])) / voxel, float(ang)


# ---- the model of the convergence tests: the ray-cast tests' recipe (6 frames, 8 degrees apart) on a finer grid -----------------
FINE_DIMS, FINE_VOXEL, FINE_CENTRE = (96, 96, 96), 0.01, (0.0, -0.1, 0.0)
FINE_ORIGIN = tuple(FINE_CENTRE[i] - 0.5 * FINE_DIMS[i] * FINE_VOXEL for i in range(3))


def fused_model(n=6, deg=8.0):
    """(scene, poses, C oracle holding the fused TSDF, (dims, origin, voxel, trunc))"""
    from oracle import c_oracle
    scene = synth.object_scene()
    poses = synth.orbit_poses(n, 1.0, deg)
    orc = c_oracle.Oracle(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], dims=FINE_DIMS, origin=FINE_ORIGIN,
                          voxel_size=FINE_VOXEL, sdf_trunc=4 * FINE_VOXEL)
    for i, p in enumerate(poses):
        d, _ = synth.render(scene, p, SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], seed=i)
        orc.tsdf_integrate(d, p[0], p[1])
    return scene, poses, orc, (FINE_DIMS, FINE_ORIGIN, FINE_VOXEL, 4 * FINE_VOXEL)


def novel_pose():
    """a camera that is not in the model: on the orbit at 20 degrees, midway between its frames 2 and 3"""
    return synth.orbit_poses(6, 1.0, 4.0)[5]


# ---- the open arc of the whole-stage experiment (CPU: oracle + numpy reference; GPU: the pipeline) ----------------------------
# The shape at which tracking beats the chain with the numpy reference alone (tests/test_track_reference_cpu.py): 48 frames 1.5
# degrees apart with 20 mm of depth noise.  At the issue's starting shape (24 frames, 3 degrees, 2 mm) it does not: the chain's mean
# centre error is 0.44 mm there, tracking's 10 mm -- a 26 mm grid gives every registration a bias of 0.1-0.15 voxel (DESIGN.md
# section 12), which the model then carries; the chain loses only once its own error, which grows with the noise and the number
# of pairs, is past that.
# the grid holds the whole room of synth.object_scene() (x, z in +-1.2, y in -1.2 .. 0.35) with a voxel to spare: every pixel of a
# frame can find its cell, as in the pipeline, whose tracking grid is bounded from the frames
ARC = dict(n=48, deg=1.5, radius=1.0, noise=0.02, dims=(96, 96, 96), voxel=0.026, centre=(0.0, -0.425, 0.0))


def arc_frames(arc=ARC, cam=SMALL):
    """(analytic poses, [(depth, bgr)]) of the arc: synth.object_scene() from synth.orbit_poses, depth noise with seeds 0, 1, ..."""
    scene = synth.object_scene()
    poses = synth.orbit_poses(arc["n"], arc["radius"], arc["deg"])
    frames = [synth.render(scene, p, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], noise_sigma=arc["noise"], seed=i)
              for i, p in enumerate(poses)]
    return poses, frames


def centre_errors_mm(Ts, truth):
    """camera-centre error (mm) of every pose, both sets brought to the gauge cam0 = I"""
    out = []
    for T, G in zip(np.asarray(Ts) @ np.linalg.inv(Ts[0]), np.asarray(truth) @ np.linalg.inv(truth[0])):
        out.append(1e3 * float(np.linalg.norm(-T[:3, :3].T @ T[:3, 3] + G[:3, :3].T @ G[:3, 3])))
    return np.array(out)
