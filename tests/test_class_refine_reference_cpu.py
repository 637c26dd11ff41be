"""CPU: the crafted frames of class_refine_common are robust in the model (every box class and every lane decision of a pair the
refinement sees is the same under the model's perturbations), the table of what each must count is pinned, every class of
tl3d_class_refine_info occurs, and the model's per-voxel decisions are sound against the per-voxel truth."""
import numpy as np
import pytest

import class_refine_common as cc
import class_refine_reference as rr
import prep_classes_reference as pr

# name: (seen, open, dropped, free, both kinds)
TABLE = {
    "far_planted_1.4_121": (4, 2, 0, 2, 0),
    "far_planted_1.4_125": (4, 2, 0, 2, 0),
    "near_planted_1.4_121": (4, 2, 2, 0, 0),
    "near_planted_1.4_125": (4, 2, 2, 0, 0),
    "holes_planted_1.4_122": (4, 2, 2, 0, 0),
    "holes_planted_1_551": (5, 2, 3, 0, 0),
    "holes_planted_0.8_151": (4, 1, 3, 0, 0),
    "cross_u_2.0": (2, 0, 0, 0, 2),
    "cross_v_2.0": (2, 0, 0, 0, 2),
    "cross_u_0.8": (2, 0, 0, 0, 2),
    "cross_v_0.8": (2, 0, 0, 0, 2),
    "step_u_1.4_264_near_first": (8, 0, 0, 4, 4),
    "step_u_1.4_264_far_first": (8, 0, 4, 0, 4),
    "step_v_1_136_near_first": (8, 0, 0, 4, 4),
    "step_v_1_160_far_first": (6, 0, 0, 2, 4),
    "step_u_1_288_near_first": (6, 0, 2, 0, 4),
}
CASES = cc.cases()


def test_table_names():
    assert [c.name for c in CASES] == list(TABLE)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_is_robust_and_pinned(case):
    e = rr.expected(case.s, case.depth, *case.pose)
    assert e["robust"], "a box class or a lane decision changes under a perturbation"
    assert tuple(e[k] for k in ("seen", "open", "dropped", "free", "both")) == TABLE[case.name]
    assert e["seen"] == e["open"] + e["dropped"] + e["free"] + e["both"]
    # depths are whole millimetres (the 16-bit twin holds the same image)
    assert np.array_equal(case.u16.astype(np.int32), np.where(case.mm < 0, 0, case.mm))


def test_every_class_occurs():
    tot = np.sum([TABLE[c.name] for c in CASES], axis=0)
    assert (tot > 0).all(), tot
    kinds = {c.name.split("_")[0] for c in CASES}
    assert kinds == {"far", "near", "holes", "cross", "step"}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_lane_decisions_are_sound(case):
    """a SKIP lane is a voxel the per-voxel rule leaves alone, a FREE lane one it gives exactly (32767, 1)"""
    s = case.s
    dec = rr.lane_decisions(s, case.depth, *case.pose)
    truth = pr.voxel_truth(s, case.depth, *case.pose)
    assert not truth["upd"][dec == rr.SKIP_LANE].any()
    free = dec == rr.FREE_LANE
    assert truth["upd"][free].all() and (truth["q"][free] == 32767).all()
