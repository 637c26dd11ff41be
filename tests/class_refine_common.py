"""Crafted frames for the refinement of replayed classification entries (class_refine_kernel): one MIXED brick (the one-brick grid
and camera A of prep_classes_common) whose sub-bricks reach each class of tl3d_class_refine_info.

  far_planted     far wall, ONE pixel at its voxel's own depth: that sub-brick stays open; the sub-bricks the box test leaves MIXED
                  beside it are in free space voxel by voxel -> FREE
  near_planted    near wall (everything behind it), ONE far pixel: its sub-brick stays open, the others -> dropped
  holes_planted   no valid pixel but ONE at its voxel's own depth: open under it, the others -> dropped
  cross_*         far wall, the brick astride the right / bottom border (anchored_pose with the crossing anchors, moved on until
                  voxel centres leave the image): lanes outside the image skip, lanes inside are free -> both kinds of lane
  step_u, step_v  near wall on one half of the image, far wall on the other, the step ON an 8-px tile boundary through a
                  sub-brick's footprint: no tile holds both depths, every lane is decided, some each way -> both kinds

Depths are whole millimetres; class_refine_reference.expected() says what the counters must show and whether the frame is robust
under the model's perturbations (only such frames are compared with the GPU; tests/test_class_refine_reference_cpu.py pins that)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import prep_classes_common as pc
import prep_classes_reference as pr

I3 = np.eye(3)


@dataclass(frozen=True)
class RCase:
    name: str
    s: pr.Setup = field(repr=False, compare=False)
    t: tuple
    mm: np.ndarray = field(repr=False, compare=False)

    @property
    def pose(self):
        return (I3, np.asarray(self.t, float))

    @property
    def depth(self):
        return pc.to_f32(self.mm)

    @property
    def u16(self):
        return pc.to_u16(self.mm)


def _voxel_pixel(s, t, ijk):
    """(u, v, depth in whole mm) of voxel (i, j, k) of the one brick under pose (I, t)"""
    tr = pr.voxel_truth(s, pc.to_f32(pc.mm_image(s, pc.FAR_MM)), I3, np.asarray(t, float))
    i, j, k = ijk
    assert tr["win"][k, j, i]
    return int(tr["u"][k, j, i]), int(tr["v"][k, j, i]), int(round(float(tr["zc"][k, j, i]) * 1000.0))


OWN_OFFSET_MM = 10                             # a planted "own depth" pixel lies this far behind its voxel: every threshold is >= 9 mm away


def _planted(s, t, wall_mm, ijk, value):
    mm = pc.mm_image(s, wall_mm)
    u, v, own = _voxel_pixel(s, t, ijk)
    mm[v, u] = own + OWN_OFFSET_MM if value == "own" else value
    return mm


def _step(s, axis, boundary, near_first):
    """near wall on one side of pixel column / row `boundary` (a multiple of 8: a tile boundary), far wall on the other"""
    assert boundary % 8 == 0
    mm = pc.mm_image(s, pc.FAR_MM)
    sl = slice(None, boundary) if near_first else slice(boundary, None)
    if axis == 0:
        mm[:, sl] = pc.NEAR_MM
    else:
        mm[sl, :] = pc.NEAR_MM
    return mm


# What a search over distances, voxels, tile boundaries and shifts across the border found robust in the model (every box class and
# every lane decision of a pair that is seen the same under all perturbations); kept as data, checked by the CPU test.
PLANTED = (("far", 1.4, (1, 2, 1)), ("far", 1.4, (1, 2, 5)), ("near", 1.4, (1, 2, 1)), ("near", 1.4, (1, 2, 5)),
           ("holes", 1.4, (1, 2, 2)), ("holes", 1.0, (5, 5, 1)), ("holes", 0.8, (1, 5, 1)))
CROSS = ((0.98046875, 0.0, 2.0), (0.0, 0.4765625, 2.0), (0.33251953125, 0.0, 0.800048828125), (0.0, 0.12890625, 0.800048828125))
STEPS = ((1.4, 0, 264, True), (1.4, 0, 264, False), (1.0, 1, 136, True), (1.0, 1, 160, False), (1.0, 0, 288, True))


@functools.lru_cache(maxsize=None)
def cases():
    s = pc.setup("A")
    out = []
    for kind, tz, ijk in PLANTED:
        mid = pc.anchored_pose(s, tz, (0, 0))
        wall, value = {"far": (pc.FAR_MM, "own"), "near": (pc.NEAR_MM, pc.FAR_MM), "holes": (0, "own")}[kind]
        out.append(RCase(f"{kind}_planted_{tz:g}_{ijk[0]}{ijk[1]}{ijk[2]}", s, mid, _planted(s, mid, wall, ijk, value)))
    for t in CROSS:
        out.append(RCase(f"cross_{'u' if t[0] else 'v'}_{t[2]:.1f}", s, t, pc.mm_image(s, pc.FAR_MM)))
    for tz, axis, boundary, near_first in STEPS:
        mid = pc.anchored_pose(s, tz, (0, 0))
        out.append(RCase(f"step_{'uv'[axis]}_{tz:g}_{boundary}_{'near' if near_first else 'far'}_first", s, mid, _step(s, axis, boundary, near_first)))
    return tuple(out)
