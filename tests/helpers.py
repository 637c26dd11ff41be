"""Shared builders for the parity tests: small scenes, grids, oracle/GPU context pairs."""
import numpy as np

import tl3d
from tl3d import synth
from oracle import c_oracle

SMALL = dict(width=160, height=120, fx=140.0, fy=140.0, cx=79.5, cy=59.5)


def small_scene_frames(n=3, deg=2.0, radius=1.0, noise=0.0, cam=SMALL, scene=None):
    scene = scene or synth.object_scene()
    poses = synth.orbit_poses(n, radius, deg)
    frames = [synth.render(scene, p, cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                           noise_sigma=noise, seed=i) for i, p in enumerate(poses)]
    return poses, frames


def make_pair(cam=SMALL, dims=(64, 64, 64), voxel=0.02, centre=(0.0, 0.0, 0.0), trunc=None, n_slots=4,
              min_depth=0.1, max_depth=50.0, channels=tl3d.CH_TSDF | tl3d.CH_CENTROID):
    """(GPU FusionContext, C oracle) over the same geometry."""
    origin = tuple(centre[i] - 0.5 * dims[i] * voxel for i in range(3))
    trunc = 4 * voxel if trunc is None else trunc
    spec = tl3d.GridSpec(dims, origin, voxel, trunc, channels)
    ctx = tl3d.FusionContext(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                             min_depth=min_depth, max_depth=max_depth, n_slots=n_slots, grid=spec)
    orc = c_oracle.Oracle(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"],
                          min_depth=min_depth, max_depth=max_depth, dims=dims, origin=origin, voxel_size=voxel,
                          sdf_trunc=trunc)
    return ctx, orc


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


# The smallest scene the staging tests need: a 64 x 48 camera orbiting two spheres inside a 32^3 grid at 1 cm (64 bricks, 16
# extraction chunks of 2048 records).  Sparse: pools of 64 bricks per channel behind brick tables.
TINY = dict(width=64, height=48, fx=60.0, fy=60.0, cx=31.5, cy=23.5)


def tiny_fused(sparse, n=3, fuse=True):
    """An open FusionContext (close it, or use `with`) with n frames of the tiny scene uploaded and, unless fuse=False, fused
    into both channels; its .tiny_poses holds the poses."""
    scene = synth.Scene(spheres=[((0.0, 0.0, 0.0), 0.10), ((0.07, 0.03, 0.0), 0.06)])
    poses = synth.orbit_poses(n, 0.5, 15.0)
    pool = 64 if sparse else 0
    spec = tl3d.GridSpec((32, 32, 32), (-0.16, -0.16, -0.16), 0.01, 0.04, pool_tsdf=pool, pool_centroid=pool)
    ctx = tl3d.FusionContext(TINY["width"], TINY["height"], TINY["fx"], TINY["fy"], TINY["cx"], TINY["cy"], n_slots=n, grid=spec)
    for i, p in enumerate(poses):
        d, c = synth.render(scene, p, **TINY)
        ctx.upload(i, d, c)
    if fuse:
        ctx.fuse_frames(list(range(n)), poses, centroid_subsample=1)
    ctx.tiny_poses = poses
    return ctx
