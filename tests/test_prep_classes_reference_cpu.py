"""The model of the TSDF prep's classes (prep_classes_reference) and the crafted frames (prep_classes_common) on the CPU:
the two pyramid formulations agree, the model never answers skip / free where the per-voxel truth forbids it (on every case and on
seeded random frames), every case is decisive and robust, the table of what the cases reach is pinned, and every seeded fault of
the model is caught by a named case.  tests/test_gpu_prep_classes.py runs the same frames through the HIP kernels."""
import numpy as np
import pytest

import prep_classes_common as pc
import prep_classes_reference as pr
from prep_classes_reference import FREE, MIXED, SKIP

COVER = pc.cases()
BORDER = pc.border_cases()
CELL = pc.cell_cases()
ALL = pc.all_cases()
BY_NAME = {c.name: c for c in ALL}


def _ids(cases):
    return [c.name for c in cases]


# ---- what the cases reach -----------------------------------------------------------------------------------------------------------
# (camera group, classifier, rule, pyramid level) -> cases.  AB: the 552 x 296 and 542 x 287 cameras (and the anamorphic pair), D: 14 x 11
# (two levels), T: 8 x 7 (one level).  Level 5 (256-px tiles): the brick classifier needs a footprint that crosses five 128-px
# tiles -- with FREE still possible only where the image is flat enough to hold it (the anamorphic camera), else by the skip rule,
# which does not ask for "inside"; the sub-brick classifier (more than 8 tiles of 128 px) gets there from 0.2 m by every rule.
LEVELS = {
    ('AB', 'brick', 'free_invalid', 0): 5, ('AB', 'brick', 'free_invalid', 1): 1, ('AB', 'brick', 'free_invalid', 2): 1,
    ('AB', 'brick', 'free_invalid', 3): 4, ('AB', 'brick', 'free_invalid', 4): 3, ('AB', 'brick', 'free_invalid', 5): 2,
    ('AB', 'brick', 'free_low', 0): 1, ('AB', 'brick', 'free_low', 1): 1, ('AB', 'brick', 'free_low', 2): 1,
    ('AB', 'brick', 'free_low', 3): 1, ('AB', 'brick', 'free_low', 4): 1, ('AB', 'brick', 'free_low', 5): 1,
    ('AB', 'brick', 'skip_far', 0): 8, ('AB', 'brick', 'skip_far', 1): 1, ('AB', 'brick', 'skip_far', 2): 1,
    ('AB', 'brick', 'skip_far', 3): 4, ('AB', 'brick', 'skip_far', 4): 3, ('AB', 'brick', 'skip_far', 5): 3,
    ('AB', 'sub', 'free_invalid', 0): 2, ('AB', 'sub', 'free_invalid', 1): 4, ('AB', 'sub', 'free_invalid', 2): 1,
    ('AB', 'sub', 'free_invalid', 3): 4, ('AB', 'sub', 'free_invalid', 4): 3, ('AB', 'sub', 'free_invalid', 5): 3,
    ('AB', 'sub', 'free_low', 0): 1, ('AB', 'sub', 'free_low', 1): 1, ('AB', 'sub', 'free_low', 2): 1,
    ('AB', 'sub', 'free_low', 3): 1, ('AB', 'sub', 'free_low', 4): 1, ('AB', 'sub', 'free_low', 5): 1,
    ('AB', 'sub', 'skip_far', 0): 5, ('AB', 'sub', 'skip_far', 1): 2, ('AB', 'sub', 'skip_far', 2): 2,
    ('AB', 'sub', 'skip_far', 3): 5, ('AB', 'sub', 'skip_far', 4): 3, ('AB', 'sub', 'skip_far', 5): 3,
    ('D', 'brick', 'free_invalid', 0): 1, ('D', 'brick', 'free_low', 0): 1, ('D', 'brick', 'skip_far', 0): 1,
    ('D', 'sub', 'free_invalid', 0): 1, ('D', 'sub', 'free_low', 0): 1, ('D', 'sub', 'skip_far', 0): 1,
    ('T', 'brick', 'free_invalid', 0): 1, ('T', 'brick', 'free_low', 0): 1, ('T', 'brick', 'skip_far', 0): 1,
}
# (classifier, free | skip, position of the decisive pixel's tile) -> cases.  ragged_x@L: the tile of level L - 1 that holds the
# pixel has no right (col) / lower (row) / neither (corner) sibling under its parent of level L; l0_last_*: the last pixel column /
# row of a partial 8-px tile (a box that reaches it has left the image, so only the skip rule gets there); win_*: first / last tile
# of a full 4-tile axis of the brick classifier's window; walk8_AxB: the 8th tile of the sub-brick walk over an A x B box;
# image_near / image_none: the skip image is a near wall / holds no valid pixel.
TAGS = {
    ('brick', 'free', 'distractor'): 2, ('brick', 'free', 'ragged_col@3'): 1, ('brick', 'free', 'ragged_col@4'): 1,
    ('brick', 'free', 'ragged_corner@3'): 1, ('brick', 'free', 'ragged_corner@4'): 1, ('brick', 'free', 'ragged_row@3'): 1,
    ('brick', 'free', 'ragged_row@4'): 3, ('brick', 'free', 'ragged_row@5'): 1, ('brick', 'free', 'win_u_first'): 1,
    ('brick', 'free', 'win_u_last'): 3, ('brick', 'free', 'win_v_first'): 1, ('brick', 'free', 'win_v_last'): 1,
    ('brick', 'skip', 'distractor'): 2, ('brick', 'skip', 'image_near'): 21, ('brick', 'skip', 'image_none'): 1,
    ('brick', 'skip', 'l0_last_col'): 1, ('brick', 'skip', 'l0_last_row'): 1, ('brick', 'skip', 'ragged_col@3'): 1,
    ('brick', 'skip', 'ragged_col@4'): 2, ('brick', 'skip', 'ragged_col@5'): 1, ('brick', 'skip', 'ragged_corner@3'): 1,
    ('brick', 'skip', 'ragged_corner@4'): 2, ('brick', 'skip', 'ragged_corner@5'): 1, ('brick', 'skip', 'ragged_row@3'): 1,
    ('brick', 'skip', 'ragged_row@4'): 2, ('brick', 'skip', 'ragged_row@5'): 1, ('brick', 'skip', 'win_u_first'): 2,
    ('brick', 'skip', 'win_u_last'): 4, ('brick', 'skip', 'win_v_first'): 1, ('brick', 'skip', 'win_v_last'): 1,
    ('sub', 'free', 'distractor'): 5, ('sub', 'free', 'ragged_col@3'): 1, ('sub', 'free', 'ragged_col@4'): 4,
    ('sub', 'free', 'ragged_col@5'): 2, ('sub', 'free', 'ragged_corner@3'): 1, ('sub', 'free', 'ragged_corner@4'): 2,
    ('sub', 'free', 'ragged_corner@5'): 1, ('sub', 'free', 'ragged_row@3'): 1, ('sub', 'free', 'ragged_row@4'): 2,
    ('sub', 'free', 'ragged_row@5'): 1, ('sub', 'free', 'walk8_1x8'): 1, ('sub', 'free', 'walk8_2x4'): 1,
    ('sub', 'free', 'walk8_4x2'): 1, ('sub', 'free', 'walk8_8x1'): 1, ('sub', 'skip', 'distractor'): 3,
    ('sub', 'skip', 'image_near'): 19, ('sub', 'skip', 'image_none'): 2, ('sub', 'skip', 'l0_last_col'): 1,
    ('sub', 'skip', 'l0_last_row'): 1, ('sub', 'skip', 'ragged_col@3'): 1, ('sub', 'skip', 'ragged_col@4'): 2,
    ('sub', 'skip', 'ragged_col@5'): 1, ('sub', 'skip', 'ragged_corner@3'): 1, ('sub', 'skip', 'ragged_corner@4'): 2,
    ('sub', 'skip', 'ragged_corner@5'): 1, ('sub', 'skip', 'ragged_row@3'): 1, ('sub', 'skip', 'ragged_row@4'): 2,
    ('sub', 'skip', 'ragged_row@5'): 1, ('sub', 'skip', 'walk8_1x8'): 1, ('sub', 'skip', 'walk8_2x4'): 1,
    ('sub', 'skip', 'walk8_4x2'): 1, ('sub', 'skip', 'walk8_8x1'): 1,
}
N_COVER, N_BORDER, N_CELL = 94, 9, 4


def test_the_search_still_finds_exactly_the_pinned_cases():
    """prep_classes_cases.RECIPES is what cover() gives: an edit to the model, the cameras or the search that changes, drops or adds
    a case shows here (and the tables below say what it covered)"""
    import prep_classes_cases
    assert pc.cover() == prep_classes_cases.RECIPES


def test_the_case_count_and_the_table_of_what_the_cases_reach_are_pinned():
    assert (len(COVER), len(BORDER), len(CELL)) == (N_COVER, N_BORDER, N_CELL)
    assert len(set(_ids(ALL))) == len(ALL)
    levels, tags = pc.table(COVER)
    assert levels == LEVELS, sorted(set(levels.items()) ^ set(LEVELS.items()))
    assert tags == TAGS, sorted(set(tags.items()) ^ set(TAGS.items()))
    # every classifier at every level it can reach by each rule group, every invalid value, both kinds of skip image, both loads
    for kind in ("brick", "sub"):
        assert {k[3] for k in levels if k[1] == kind and k[2] == "skip_far"} >= set(range(6))
        assert {k[3] for k in levels if k[1] == kind and k[2] != "skip_far"} >= set(range(6))
    planted = {int(c.mm[c.pixel[1], c.pixel[0]]) for c in COVER if c.rule == "free_invalid"}
    assert planted == {0, -1, 50, 16000}, planted
    assert {bool((c.mm_base == pc.NEAR_MM).any()) for c in COVER if c.rule == "skip_far"} == {True, False}      # near wall / no valid pixel
    assert {c.cam for c in COVER} == set(pc.CAMERAS) and pc.CAMERAS["B"]["W"] & 3
    assert [len(pr.level_shapes(pc.CAMERAS[k]["W"], pc.CAMERAS[k]["H"])) for k in "ABDT"] == [8, 8, 2, 1]


# ---- the pyramid, twice -------------------------------------------------------------------------------------------------------------------
def _same_pyramid(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for la, lb in zip(a, b) for x, y in zip(la, lb))


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_reduction_pyramid_equals_brute_force_pyramid(case):
    for d in (case.depth, case.base):
        red, brute = pr.pyramid_by_reduction(case.s, d), pr.pyramid_brute_force(case.s, d)
        assert [l[0].shape[::-1] for l in red] == list(pr.level_shapes(case.s.W, case.s.H))
        assert _same_pyramid(red, brute)
        if case.mm is case.mm_base:
            break


def test_the_pyramid_faults_change_the_pyramid():
    """(the comparison above can fail: each reduction fault differs from the brute-force tables on some case image)"""
    for fault in pr.PYRAMID_FAULTS:
        assert any(not _same_pyramid(pr.pyramid_by_reduction(c.s, c.depth, 1.0, fault), pc.pyramid_of(c.s, c.mm)) for c in ALL), fault


# ---- decisive, robust, sound -------------------------------------------------------------------------------------------------------------------
DECISIVE = tuple(c for c in COVER + CELL if c.pixel is not None)


@pytest.mark.parametrize("case", DECISIVE, ids=_ids(DECISIVE))
def test_case_is_decisive_and_robust_and_so_is_its_u16_twin(case):
    assert pc.is_decisive(case)
    assert pc.is_decisive(case, mm=case.u16.astype(np.int32), mm_base=case.u16_base.astype(np.int32))
    if case.distractor is not None:                     # under no voxel: the per-voxel truth does not know it is there
        truth = pr.voxel_truth(case.s, case.depth, *case.pose)
        assert not (truth["win"] & (truth["u"] == case.distractor[0]) & (truth["v"] == case.distractor[1])).any()
        assert case.mm[case.distractor[1], case.distractor[0]] != case.mm[0, 1]


@pytest.mark.parametrize("case", BORDER, ids=_ids(BORDER))
def test_border_case_is_robust(case):
    _, _, cls, why = pc.BORDER[case.rule]
    v, seen = pr.robust_classes(case.s, pc.pyramid_of(case.s, case.mm), pr.brick_box(case.s, case.R, np.asarray(case.t), 0, 0, 0), "brick")
    assert (v.cls, v.why) == (cls, why) and len(seen) == 1
    skip_ok, free_ok = pc.target_permits(case, case.mm)
    # inside_margin: every voxel is still in the window (the margin is what says no); inside_out: some are not
    assert free_ok == (cls != SKIP and case.rule != "inside_out") and skip_ok == (cls == SKIP)


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_model_is_sound_on_the_whole_frame_of_every_case(case):
    for d in (case.depth, case.base):
        truth = pr.voxel_truth(case.s, d, *case.pose)
        assert pr.unsound(case.s, pr.classify_frame(case.s, d, *case.pose), truth) == []


def test_cell_list_cases_see_the_ragged_cells_by_their_only_layer():
    assert _ids(CELL) == ["A_cell_corner_free_invalid_b440_u466v223", "A_cell_corner_skip_far_b440_u466v223",
                          "A_cell_edge_skip_far_b443_u6v294", "A_cell_edge_far"]
    for case in CELL:
        s = case.s
        assert s.nb == (5, 5, 5) and case.brick[0] == 4
        classes = pr.classify_frame(s, pc.to_f32(pc.mm_image(s, pc.FAR_MM)), *case.pose, subs=False)
        truth = pr.voxel_truth(s, case.base, *case.pose)
        u, v = truth["u"][truth["win"]], truth["v"][truth["win"]]
        why = {}
        for v_, _ in classes.values():
            why[v_.why] = why.get(v_.why, 0) + 1
        if "corner" in case.name:                        # every brick passes both sphere tests; the grid's far faces at the borders
            assert why == {"box": 125} and u.max() >= s.W - 12 and v.max() >= s.H - 12
        else:                                            # only the layer bx = 4 survives, at the left border; most fall to their sphere
            assert why == {"sphere": 110, "pixel box": 5, "box": 10}, why
            assert {k[0] for k, (v_, _) in classes.items() if v_.cls != SKIP} == {4} and u.min() == 0 and u.max() < 64
            assert {v_.cls for v_, _ in classes.values()} == {SKIP, MIXED}


# ---- random frames ---------------------------------------------------------------------------------------------------------------------------
RANDOM = pr.Setup(W=130, H=93, fx=100.0, fy=100.0, cx=64.5, cy=46.0, mind=0.05, maxd=16.0, dims=(16, 16, 24), origin=(-0.25, -0.25, -0.375),
                  voxel=1.0 / 32, trunc=0.125)
N_RANDOM = 240


def _random_frame(rng, i):
    """camera outside the grid looking at it, inside it, grazing it (the grid at the edge of the view) or very close to it; a wall
    near the grid, far behind it or in front of it, tilted, with scattered holes, a block of holes and a foreground occluder"""
    how = ("outside", "inside", "grazing", "close")[i % 4]
    dist = {"outside": rng.uniform(0.8, 3.0), "inside": rng.uniform(0.0, 0.3), "grazing": rng.uniform(0.6, 2.0), "close": rng.uniform(0.3, 0.6)}[how]
    d = rng.normal(size=3)
    pos = dist * d / np.linalg.norm(d)
    look = -pos if how != "inside" else rng.normal(size=3)
    look = look / np.linalg.norm(look) + (rng.normal(size=3) * (0.6 if how == "grazing" else 0.1))
    z = look / np.linalg.norm(look)
    x = np.cross(rng.normal(size=3), z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    t = -R @ pos
    s = RANDOM
    wall = (dist + rng.uniform(-0.4, 0.4), 12.0, 0.1, dist + 1.0)[(i // 4) % 4]
    vv, uu = np.mgrid[0:s.H, 0:s.W]
    img = max(wall, 0.06) + (rng.uniform(-0.3, 0.3) * (uu - s.cx) / s.fx + rng.uniform(-0.3, 0.3) * (vv - s.cy) / s.fy) * (i % 3 == 0)
    img = img.astype(np.float32)
    img[rng.random(img.shape) < 0.003] = 0.0
    if i % 2:
        u0, v0 = rng.integers(0, s.W - 20), rng.integers(0, s.H - 20)
        img[v0:v0 + rng.integers(1, 40), u0:u0 + rng.integers(1, 40)] = rng.choice([0.0, np.nan, 0.05, 16.0, 0.08, 12.0])
    if i % 5 == 0:
        u0, v0 = rng.integers(0, s.W - 10), rng.integers(0, s.H - 10)
        img[v0:v0 + 30, u0:u0 + 50] = rng.uniform(0.06, max(0.07, dist - 0.3))
    return img, R, t


def test_model_is_sound_on_random_frames():
    rng = np.random.default_rng(20260)
    seen = {("brick", c): 0 for c in (SKIP, MIXED, FREE)}
    seen.update({("sub", c): 0 for c in (SKIP, MIXED, FREE)})
    levels = set()
    for i in range(N_RANDOM):
        img, R, t = _random_frame(rng, i)
        classes = pr.classify_frame(RANDOM, img, R, t)
        truth = pr.voxel_truth(RANDOM, img, R, t)
        assert pr.unsound(RANDOM, classes, truth) == [], i
        for v, sv in classes.values():
            seen[("brick", v.cls)] += 1
            levels.add(("brick", v.level))
            for w in sv or ():
                seen[("sub", w.cls)] += 1
                levels.add(("sub", w.level))
    print(seen, sorted(levels))
    assert all(n >= 20 for n in seen.values()), seen
    assert {l for k, l in levels if k == "brick"} >= set(range(4)) and {l for k, l in levels if k == "sub"} >= set(range(4))


# ---- seeded faults ---------------------------------------------------------------------------------------------------------------------------
# fault of the model -> (the case that catches it, how).  A GPU classifier with the same fault would write a grid that differs from
# the oracle's at the voxel over the decisive pixel ("unsound"), or break the count bounds of test_gpu_prep_classes ("loose").
CAUGHT_BY = {
    "drop_last_col": ("A_sub1_free_invalid_L4_z0.64_a10_u529v62", "unsound"),
    "drop_last_row": ("A_brick_free_invalid_L4_z0.5_a00_u167v256", "unsound"),
    "allvalid_lost_above_0": ("A_brick_free_invalid_L1_z5.5_a00_u265v137", "unsound"),
    "allvalid_lost_above_1": ("A_brick_free_invalid_L2_z2.8_a01_u256v248", "unsound"),
    "allvalid_lost_above_2": ("A_brick_free_invalid_L3_z1.4_a01_u236v205", "unsound"),
    "swap_min_max_in_skip": ("A_brick_skip_far_L0_z8_a00_u269v141", "unsound"),
    "window_3x3": ("A_brick_free_invalid_L0_z8_a10_u544v141", "unsound"),
    "walk_first_row_only": ("A_sub6_free_invalid_L0_z8_a01_u269v288", "unsound"),
    "level_one_too_fine": ("A_brick_free_invalid_L4_z0.5_a00_u167v256", "unsound"),
    "partial_tile_invalid": ("B_brick_free_invalid_L3_z1_a01_u215v257", "loose"),
    "ignore_inside": ("B_inside_out", "unsound"),
}


@pytest.mark.parametrize("fault", pr.FAULTS)
def test_seeded_fault_is_caught_by_a_named_case(fault):
    name, how = CAUGHT_BY[fault]
    case = BY_NAME[name]
    assert pc.fault_effect(case, None) is None
    assert pc.fault_effect(case, fault) == how


def test_every_fault_has_its_case():
    assert set(CAUGHT_BY) == set(pr.FAULTS)
