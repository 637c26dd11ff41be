"""Crafted batches for the trip counts of the TSDF update's pair loop (kernels_tsdf.hip: tsdf_update_pairs_kernel).

A brick with P pairs (frame, MIXED sub-brick) runs P div U whole loop bodies of U steps, then the P mod U steps that remain, then
the drain that belongs to that remainder (U = 6 steps at the shipped depth-gather latency, 2 and 4 at the others), so what can go
wrong depends on P mod U, on P against U and on P against the depth of the pipeline.  The cases make P take every such value on
a grid of 3 x 3 x 3 bricks:

  * two images of 64 x 48 pixels seen from one pose: a tilted plane through the grid and a step edge (near wall left, far wall
    right) -- bricks with 1 to 8 MIXED sub-bricks, bricks whose sub-bricks are FREE or skipped only, free and skipped bricks;
  * the SAME frame and pose fused n = 1 ... 14 times in one batch: a brick with m MIXED sub-bricks has P = n m pairs.

mixed_per_brick() counts m per brick with the prep chain's numpy model (prep_classes_reference.classify_frame); a brick counts
only where every one of the model's perturbations gives the same classes, so that the last bits of the GPU's projection cannot
move it.  tests/test_update_trip_counts_reference_cpu.py proves from these counts that every loop path is taken; the GPU test
fuses the same batches and holds the grid against the C oracle bit for bit.

Every depth value is a whole number of millimetres, so each image has a uint16 twin with the same grid."""
from __future__ import annotations

import functools

import numpy as np

import prep_classes_reference as pr
from prep_classes_reference import FREE, MIXED

W, H = 64, 48
CAM = dict(width=W, height=H, fx=50.0, fy=50.0, cx=31.5, cy=23.5)
VOX, TRUNC = 0.02, 0.04
DIMS, ORIGIN = (24, 24, 24), (-0.24, -0.24, 0.60)
MIND, MAXD = 0.1, 50.0
POSE = (np.eye(3), np.zeros(3))                  # at the origin, looking along +z at the grid's near face
N_MAX = 14
IMAGES = ("plane", "step")
UNROLLS = (6, 4, 2)                              # steps per loop body at depth-gather latencies 2, 3 and 1
PIPE_DEPTH = 3                                   # 1 + the shipped latency: pairs at or below it never fill the pipeline

SETUP = pr.Setup(W=W, H=H, fx=CAM["fx"], fy=CAM["fy"], cx=CAM["cx"], cy=CAM["cy"], mind=MIND, maxd=MAXD, dims=DIMS, origin=ORIGIN,
                 voxel=VOX, trunc=TRUNC)


@functools.lru_cache(maxsize=None)
def image_mm(name):
    """the image in whole millimetres (uint16, read-only)"""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    if name == "plane":                          # tilted about both image axes, through the grid's near half
        mm = 760.0 + 3.0 * (u - CAM["cx"]) + 12.0 * (v - CAM["cy"])
    elif name == "step":                         # a near wall on the left, a tilted far one on the right, a strip of holes on top
        mm = np.where(u < 24.0, 820.0, 900.0 + 3.0 * (u - CAM["cx"]) + 6.0 * (v - CAM["cy"]))
        mm[:3, :] = 0.0
    else:
        raise KeyError(name)
    out = np.clip(np.rint(mm), 0, 65535).astype(np.uint16)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def image_f32(name):
    """the image in metres, as the 16-bit path converts it"""
    out = image_mm(name).astype(np.float32) / np.float32(1000.0)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mixed_per_brick(name):
    """{brick: (MIXED sub-bricks, FREE sub-bricks)} of the bricks the model classes MIXED, robust ones only"""
    s = SETUP
    depth = image_f32(name)
    pyr = pr.pyramid_by_reduction(s, depth)
    out = {}
    for brick, (v, sv) in pr.classify_frame(s, depth, *POSE, pyr=pyr).items():
        if v.cls != MIXED:
            continue
        boxes = [("brick", pr.brick_box(s, *POSE, *brick))]
        boxes += [("sub", pr.subbrick_box(s, *POSE, *pr.subbrick_origin(*brick, sb))) for sb in range(8)]
        if any(len({c[0] for c in pr.robust_classes(s, pyr, box, kind)[1]}) != 1 for kind, box in boxes):
            continue
        out[brick] = (sum(x.cls == MIXED for x in sv), sum(x.cls == FREE for x in sv))
    return out


def pair_counts():
    """{(image, n): sorted pair counts P = n m of the robust MIXED bricks}"""
    return {(name, n): sorted(n * m for m, _ in mixed_per_brick(name).values()) for name in IMAGES for n in range(1, N_MAX + 1)}
