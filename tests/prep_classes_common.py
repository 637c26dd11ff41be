"""Crafted frames for the TSDF prep's brick and sub-brick classes: a uniform image that decides a box of voxels whole, and ONE
decisive pixel, under one chosen voxel centre, that takes the decision back.

  rules        free_invalid  far wall, the pixel is 0 / NaN / min_depth / max_depth   (the all-valid flag)
               free_low      far wall, the pixel lies at the voxel's own depth        (the min channel)
               skip_far      near wall (> trunc in front) or no valid pixel at all, the pixel is far   (the max channel)
  classifiers  brick (one 8^3-voxel grid, the brick would be FREE / skipped whole) and sub (the brick is MIXED through an
               auxiliary odd pixel under another sub-brick; the target sub-brick would be FREE / skipped)
  levels       the camera stands 8 m ... 0.15 m from the brick (voxel 1/32, fx = fy = 512): footprints of ~20 px to far more than
               the image; two anamorphic cameras give flat and tall footprints
  positions    the footprint in the middle of the image and against each border and corner, so that the decisive pixel can sit in a
               tile without right / lower sibling (levels >= 3), in the last column / row of a partial 8-px tile, and in the
               first / last tile of the 4x4 window or the 8th tile of the sub-brick walk

The cases are CHOSEN by cover(): it walks the poses, boxes and voxels in a fixed order and keeps a candidate when it adds a
combination nobody covers yet AND the model (prep_classes_reference) finds it decisive and robust:
  decisive  without the pixel the target's class is FREE (skip), with it MIXED, and the per-voxel truth forbids FREE (skip);
  robust    level, window, inside and class are the same under all 125 perturbations of the projected box.
What it finds is kept as data in prep_classes_cases.py (cases() builds the frames from it without searching); the CPU test
tests/test_prep_classes_reference_cpu.py runs the search, holds the two equal, and pins the number of cases and the table of what
they cover.  border_cases() and cell_cases() add frames without a decisive pixel at the image border and a 125-brick grid.

Every depth value is a whole number of millimetres (NaN apart), so each case has a uint16 twin with the same grid.
"""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

import prep_classes_reference as pr
from prep_classes_reference import FREE, MIXED, SKIP, F32

MIND, MAXD = 0.05, 16.0
VOXEL, TRUNC = 1.0 / 32, 0.125
FAR_MM, NEAR_MM = 12000, 100
CAMERAS = {
    "A": dict(W=552, H=296, fx=512.0, fy=512.0, cx=275.5, cy=147.5),     # ntx 69 35 18 9 5 3 2 1, nty 37 19 10 5 3 2 1 1
    "B": dict(W=542, H=287, fx=512.0, fy=512.0, cx=270.5, cy=143.0),     # W & 3 != 0; ntx 68 34 17 9 5 3 2 1, nty 36 18 9 5 3 2 1 1
    "D": dict(W=14, H=11, fx=12.0, fy=12.0, cx=6.5, cy=5.0),             # two levels
    "T": dict(W=8, H=7, fx=8.0, fy=8.0, cx=3.5, cy=3.0),                 # one level (brick cases only: a pixel holds many voxels)
    "E": dict(W=552, H=296, fx=512.0, fy=40.0, cx=275.5, cy=147.5),      # anamorphic: wide, flat footprints (8x1 and 4x2 tile boxes)
    "F": dict(W=552, H=296, fx=40.0, fy=512.0, cx=275.5, cy=147.5),      # ... and narrow, tall ones (1x8, 2x4)
}
SMALL = ("D", "T")
ONE_BRICK = dict(dims=(8, 8, 8), origin=(-0.125, -0.125, 0.0))
DISTANCES = (8.0, 5.5, 4.0, 2.8, 2.0, 1.4, 1.0, 0.8, 0.64, 0.5, 0.42, 0.36, 0.3, 0.26, 0.2, 0.15)
ANCHORS = tuple(itertools.product((0, 1, -1), repeat=2))
FINE_ANCHORS = tuple(a for a in itertools.product((0, 1, -1, 0.5, -0.5), repeat=2) if a not in ANCHORS)   # (for the close poses)
CROSSING = ((2, 0), (0, 2), (2, 2))                # the footprint 4 px over the right / bottom border (skip rule only)
RULES = ("free_invalid", "free_low", "skip_far")
INVALID_MM = (0, "nan", 50, 16000)                 # hole, NaN, min_depth and max_depth themselves
I3 = np.eye(3)


def setup(cam, dims=ONE_BRICK["dims"], origin=ONE_BRICK["origin"]):
    return pr.Setup(mind=MIND, maxd=MAXD, dims=tuple(dims), origin=tuple(origin), voxel=VOXEL, trunc=TRUNC, **CAMERAS[cam])


def mm_image(s, mm):
    return np.full((s.H, s.W), mm, np.int32)


def to_f32(mm):
    """millimetres -> metres as a 16-bit upload is converted; -1 stands for NaN"""
    d = (mm.astype(F32) / F32(1000.0)).astype(F32)
    d[mm < 0] = np.nan
    return d


def to_u16(mm):
    return np.where(mm < 0, 0, mm).astype(np.uint16)


@dataclass(frozen=True)
class PCase:
    name: str
    cam: str
    s: pr.Setup = field(repr=False, compare=False)
    t: Tuple[float, float, float]
    kind: str                                      # "brick" | "sub"
    rule: str
    brick: Tuple[int, int, int]
    sub: Optional[int]
    pixel: Tuple[int, int]                         # (u, v) of the decisive pixel
    level: int
    window: Tuple[int, int]
    tags: Tuple[str, ...]
    mm: np.ndarray = field(repr=False, compare=False)          # millimetre image WITH the decisive pixel (-1 = NaN)
    mm_base: np.ndarray = field(repr=False, compare=False)     # ... without it
    R: np.ndarray = field(default_factory=lambda: I3, repr=False, compare=False)
    distractor: Optional[Tuple[int, int]] = None

    @property
    def pose(self):
        return (self.R, np.asarray(self.t, float))

    @property
    def depth(self):
        return _f32_of(self, True)

    @property
    def base(self):
        return _f32_of(self, False)

    @property
    def u16(self):
        return to_u16(self.mm)

    @property
    def u16_base(self):
        return to_u16(self.mm_base)


_F32 = {}


def _f32_of(case, planted):
    key = (case.name, planted)
    if key not in _F32:
        d = to_f32(case.mm if planted else case.mm_base)
        d.setflags(write=False)
        _F32[key] = d
    return _F32[key]


# ---- the target's class under an image ---------------------------------------------------------------------------------------------------
def target_box(s, R, t, brick, sub):
    if sub is None:
        return pr.brick_box(s, R, t, *brick)
    return pr.subbrick_box(s, R, t, *pr.subbrick_origin(*brick, sub))


_PYR = {}


def pyramid_of(s, mm):
    """the model's pyramid of a millimetre image; the last few are kept (by the array's identity, which the entry keeps alive)"""
    key = (id(mm), s.W, s.H)
    if key not in _PYR:
        while len(_PYR) >= 16:
            _PYR.pop(next(iter(_PYR)))
        _PYR[key] = (mm, pr.pyramid_by_reduction(s, to_f32(mm)))
    return _PYR[key][1]


def robust_target(s, mm, R, t, brick, sub):
    """(verdict, robust?) of the target under the image; for a sub-brick target the brick must be MIXED under every perturbation"""
    pyr = pyramid_of(s, mm)
    v, seen = pr.robust_classes(s, pyr, target_box(s, R, t, brick, sub), "brick" if sub is None else "sub")
    ok = len(seen) == 1
    if sub is not None:
        _, bseen = pr.robust_classes(s, pyr, pr.brick_box(s, R, t, *brick), "brick")
        ok = ok and {c[0] for c in bseen} == {MIXED}
    return v, ok


def is_decisive(case: PCase, mm=None, mm_base=None):
    """the model's account of a case: robustly FREE / skip without the pixel, robustly MIXED with it (same level and window), and the
    per-voxel truth of the planted image forbids the former class; exactly one voxel of the target lies over the pixel"""
    mm = case.mm if mm is None else mm
    mm_base = case.mm_base if mm_base is None else mm_base
    s, R, t = case.s, case.R, np.asarray(case.t)
    want = SKIP if case.rule == "skip_far" else FREE
    kind, box = case.kind, target_box(s, R, t, case.brick, case.sub)
    if pr.box_class(s, pyramid_of(s, mm), box, kind).cls != MIXED:       # (the cheap test first)
        return False
    v0, r0 = robust_target(s, mm_base, R, t, case.brick, case.sub)
    v1, r1 = robust_target(s, mm, R, t, case.brick, case.sub)
    if not (r0 and r1 and v0.cls == want and v1.cls == MIXED and v0.level == v1.level == case.level and v0.tiles == v1.tiles):
        return False
    truth = pr.voxel_truth(s, to_f32(mm), R, t)
    cell = 8 if case.sub is None else 4
    i0, j0, k0 = (8 * b for b in case.brick) if case.sub is None else pr.subbrick_origin(*case.brick, case.sub)
    skip_ok, free_ok = pr.permitted(truth, cell)
    allowed = (skip_ok if want == SKIP else free_ok)[k0 // cell, j0 // cell, i0 // cell]
    sl = (slice(k0, k0 + cell), slice(j0, j0 + cell), slice(i0, i0 + cell))
    over = truth["win"][sl] & (truth["u"][sl] == case.pixel[0]) & (truth["v"][sl] == case.pixel[1])
    return (not allowed) and (int(over.sum()) == 1 or (case.sub is None and over.any()))


# ---- tags of a pixel -------------------------------------------------------------------------------------------------------------------
def pixel_tags(s, kind, verdict, u, v):
    shapes = pr.level_shapes(s.W, s.H)
    L = verdict.level
    tile = (u >> (3 + L), v >> (3 + L))
    nu, nv = verdict.window
    tags = []
    if kind == "brick":
        tu0, tv0 = verdict.tiles[0]
        if nu == 4:
            tags += ["win_u_first"] if tile[0] == tu0 else ["win_u_last"] if tile[0] == tu0 + 3 else []
        if nv == 4:
            tags += ["win_v_first"] if tile[1] == tv0 else ["win_v_last"] if tile[1] == tv0 + 3 else []
    elif nu * nv == 8 and tile == verdict.tiles[-1]:
        tags.append(f"walk8_{nu}x{nv}")
    for lv in range(3, L + 1):
        ntx, nty = shapes[lv - 1]
        col = ntx & 1 and (u >> (3 + lv - 1)) == ntx - 1
        row = nty & 1 and (v >> (3 + lv - 1)) == nty - 1
        if col or row:
            tags.append(("ragged_corner" if col and row else "ragged_col" if col else "ragged_row") + f"@{lv}")
    if s.W & 7 and u == s.W - 1:
        tags.append("l0_last_col")
    if s.H & 7 and v == s.H - 1:
        tags.append("l0_last_row")
    return tuple(tags)


def distractor_for(s, tags, u, v):
    """for a case in a ragged last COLUMN: the top-left pixel of the FIRST tile of the NEXT tile row at level lv - 1 -- what a
    reduction that read past the end of the row in place of the missing right child would find.  It gets an odd value of the
    case's own kind (a hole under the far wall, a far value in the skip image); cover() keeps it only if the case stays decisive
    with it, the CPU test checks that it lies under no voxel.  (Below a ragged last ROW there is no tile to put one in.)"""
    for tag in tags:
        if tag.startswith(("ragged_col", "ragged_corner")):
            lv = int(tag.split("@")[1])
            ty = (v >> (3 + lv - 1)) + 1
            if ty < pr.level_shapes(s.W, s.H)[lv - 1][1]:
                return (0, ty << (3 + lv - 1))
    return None


# ---- poses --------------------------------------------------------------------------------------------------------------------------------
def anchored_pose(s, tz, anchor):
    """t = (tx, ty, tz), R = I, per axis: the brick's widened footprint in the middle of the image (0), 2 px inside its left / top
    border (-1) or its right / bottom border (+1), half way between (+-0.5), or 4 px across the right / bottom border (2);
    rounded to multiples of 1/4096"""
    t = np.array([0.0, 0.0, tz])
    for _ in range(4):
        b = pr.brick_box(s, I3, t, 0, 0, 0)
        if b.early is not None:
            return None
        for ax, (lo, hi, n, f) in enumerate(((b.umin, b.umax, s.W, s.fx), (b.vmin, b.vmax, s.H, s.fy))):
            mid, left, right = 0.5 * (n - 1) - 0.5 * (lo + hi), 2.0 - lo, (n - 1 - 2.0) - hi
            want = {0: mid, -1: left, 1: right, 2: right + 6.0, 0.5: 0.5 * (mid + right), -0.5: 0.5 * (mid + left)}[anchor[ax]]
            t[ax] += want * (tz + 0.125) / f
    return tuple(float(np.round(x * 4096) / 4096) for x in t)


# ---- the cover ------------------------------------------------------------------------------------------------------------------------------
def _plant(mm, pixel, value):
    out = mm.copy()
    out[pixel[1], pixel[0]] = -1 if value == "nan" else value
    return out


_CAND = {}


def _candidates(s, kind, verdict, truth, brick, sub):
    """one voxel of the target per distinct tag set: (tags, (u, v), zc)"""
    key = (id(truth), sub, verdict.level, verdict.window, verdict.tiles)
    if key not in _CAND:
        _CAND[key] = (truth, _candidates_of(s, kind, verdict, truth, brick, sub))
    return _CAND[key][1]


def _candidates_of(s, kind, verdict, truth, brick, sub):
    cell = 8 if sub is None else 4
    i0, j0, k0 = (8 * b for b in brick) if sub is None else pr.subbrick_origin(*brick, sub)
    sl = (slice(k0, k0 + cell), slice(j0, j0 + cell), slice(i0, i0 + cell))
    win, uu, vv, zc = (truth[k][sl].ravel() for k in ("win", "u", "v", "zc"))
    first = {}
    for w, u, v, z in zip(win.tolist(), uu.tolist(), vv.tolist(), zc.tolist()):
        if w:
            first.setdefault((u, v), []).append(z)
    seen = {}
    for p, zs in first.items():
        if len(zs) == 1 or sub is None:
            seen.setdefault(pixel_tags(s, kind, verdict, *p), (p, zs[0]))
    return [(tags, p, z) for tags, (p, z) in sorted(seen.items(), key=lambda kv: (-len(kv[0]), kv[0]))]


def _aux_choices(s, truth, brick, sub):
    """pixels under a corner voxel of each OTHER sub-brick, the opposite one first"""
    out = []
    for other in sorted((o for o in range(8) if o != sub), key=lambda o: -bin(o ^ sub).count("1")):
        i0, j0, k0 = pr.subbrick_origin(*brick, other)
        i, j, k = i0 + 3 * (other & 1), j0 + 3 * ((other >> 1) & 1), k0 + 3 * (other >> 2)
        if truth["win"][k, j, i]:
            out.append((int(truth["u"][k, j, i]), int(truth["v"][k, j, i])))
    return out


def from_recipe(r) -> PCase:
    """a case from its recipe: (name, camera, t, sub-brick or None, rule, image "free" | "near" | "none", decisive pixel, its value
    in millimetres or "nan", auxiliary pixel or None, distractor pixel or None, level, window, tags)"""
    name, cam, t, sub, rule, image, pixel, value, aux, dis, level, window, tags = r
    s = setup(cam)
    odd = 0 if rule != "skip_far" else FAR_MM
    b = mm_image(s, {"free": FAR_MM, "near": NEAR_MM, "none": 0}[image])
    for p in (aux, dis):
        if p is not None:
            b = _plant(b, p, odd)
    return PCase(name, cam, s, tuple(t), "brick" if sub is None else "sub", rule, (0, 0, 0), sub, tuple(pixel), level, tuple(window),
                 tuple(tags), _plant(b, pixel, value), b, distractor=dis)


@functools.lru_cache(maxsize=None)
def cases():
    """the crafted one-brick cases: the recipes cover() found, kept in prep_classes_cases.py so that importing a test module does
    not repeat the search (tests/test_prep_classes_reference_cpu.py runs it once and holds the two equal)"""
    import prep_classes_cases
    return tuple(from_recipe(r) for r in prep_classes_cases.RECIPES)


@functools.lru_cache(maxsize=None)
def cover():
    """the search: the recipes of the cases, in a fixed order (deterministic)"""
    recipes, covered = [], set()
    n_invalid = 0
    for cam in CAMERAS:
        s = setup(cam)
        small = cam in SMALL
        if small:
            poses = [(tz, (0, 0)) for tz in (1.0, 0.5)]
        else:
            poses = list(itertools.product(DISTANCES, ANCHORS + CROSSING)) + list(itertools.product(DISTANCES[-8:], FINE_ANCHORS))
        bases = {"free": mm_image(s, FAR_MM), "near": mm_image(s, NEAR_MM), "none": mm_image(s, 0)}
        pyrs = {k: pr.pyramid_by_reduction(s, to_f32(v)) for k, v in bases.items()}
        for tz, anchor in poses:
            t = anchored_pose(s, tz, anchor)
            if t is None:
                continue
            truth = pr.voxel_truth(s, to_f32(bases["free"]), I3, np.asarray(t))
            for sub in ((None,) if cam == "T" else (None,) + tuple(range(8))):
                kind = "brick" if sub is None else "sub"
                box = target_box(s, I3, np.asarray(t), (0, 0, 0), sub)
                if box.early is not None:
                    continue
                for rule in (RULES[2:] if anchor in CROSSING else RULES):
                    # skip: a near wall where one fits between min_depth and the box (> trunc in front), else -- and for the
                    # footprints on the left border -- an image without any valid pixel
                    base_name = "free" if rule != "skip_far" else ("near" if (box.zmin - TRUNC > 0.11 and anchor[0] != -1) else "none")
                    v0 = pr.box_class(s, pyrs[base_name], box, kind)
                    if v0.cls != (SKIP if rule == "skip_far" else FREE) or v0.why != "box":
                        continue
                    for tags, pixel, zc in _candidates(s, kind, v0, truth, (0, 0, 0), sub):
                        if rule == "skip_far":
                            tags = tags + ("image_" + base_name,)
                        feats = {(cam if small else "AB", kind, rule, v0.level)} | {(kind, rule[:4], tg) for tg in tags}
                        if feats <= covered:
                            continue
                        if rule == "free_invalid":
                            value = INVALID_MM[n_invalid % 4]
                        elif rule == "free_low":
                            value = int(round(zc * 1000.0))
                        else:
                            value = FAR_MM
                        dis = distractor_for(s, tags, *pixel)
                        tries = [None] if sub is None else _aux_choices(s, truth, (0, 0, 0), sub)
                        for aux, with_dis in itertools.product(tries, (True, False) if dis else (False,)):
                            name = f"{cam}_{kind}{'' if sub is None else sub}_{rule}_L{v0.level}_z{tz:g}_a{anchor[0]}{anchor[1]}_u{pixel[0]}v{pixel[1]}"
                            recipe = (name, cam, t, sub, rule, base_name, pixel, value, aux, dis if with_dis else None, v0.level,
                                      v0.window, tags)
                            if is_decisive(from_recipe(recipe)):
                                recipes.append(recipe)
                                covered |= feats
                                if with_dis:
                                    covered.add((kind, rule[:4], "distractor"))
                                n_invalid += rule == "free_invalid"
                                break
    _CAND.clear()
    return tuple(recipes)


def table(which=None):
    """what the cases cover: {(camera group, classifier, rule, level): n} and {(classifier, free|skip, tag): n}"""
    levels, tags = {}, {}
    for c in cases() if which is None else which:
        k = (c.cam if c.cam in SMALL else "AB", c.kind, c.rule, c.level)
        levels[k] = levels.get(k, 0) + 1
        for tg in c.tags + (("distractor",) if c.distractor else ()):
            k = (c.kind, c.rule[:4], tg)
            tags[k] = tags.get(k, 0) + 1
    return levels, tags


# ---- cases without a decisive pixel: the image border ---------------------------------------------------------------------------------------
def placed_pose(s, tz, spec_u, spec_v):
    """t (R = I) that puts the one brick's widened footprint where the specs say, per axis: ("mid",), ("hi", x): its upper bound at
    pixel coordinate x, ("lo", x): its lower bound"""
    t = np.array([0.0, 0.0, tz])
    for _ in range(5):
        b = pr.brick_box(s, I3, t, 0, 0, 0)
        for ax, (spec, lo, hi, n, f) in enumerate(((spec_u, b.umin, b.umax, s.W, s.fx), (spec_v, b.vmin, b.vmax, s.H, s.fy))):
            want = 0.5 * (n - 1) - 0.5 * (lo + hi) if spec[0] == "mid" else spec[1] - (hi if spec[0] == "hi" else lo)
            t[ax] += want * (tz + 0.125) / f
    return tuple(float(x) for x in t)


# name -> (u spec, v spec, the model's class, why); a spec is ("mid",) or (bound, border, offset): the footprint's "hi" / "lo" bound
# at `offset` pixels from the image's first (0) or last (1) pixel column / row
MID = ("mid",)
BORDER = {
    "inside_in": (("hi", 1, -0.6), MID, FREE, "box"),                  # the widened footprint ends 0.6 px inside the last pixel column
    "inside_margin": (("hi", 1, 0.75), MID, MIXED, "box"),             # ... 0.75 px outside: every corner is still in the image
    "inside_out": (("hi", 1, 12.0), MID, MIXED, "box"),                # voxel columns beyond the window: FREE is forbidden
    "inside_in_bottom": (MID, ("hi", 1, -0.6), FREE, "box"),
    "inside_margin_bottom": (MID, ("hi", 1, 0.75), MIXED, "box"),
    "side_left": (("hi", 0, -3.0), MID, SKIP, "pixel box"),            # past the sphere tests, skipped by its pixel box
    "side_right": (("lo", 1, 3.0), MID, SKIP, "pixel box"),
    "side_top": (MID, ("hi", 0, -3.0), SKIP, "pixel box"),
    "side_bottom": (MID, ("lo", 1, 3.0), SKIP, "pixel box"),
}


@functools.lru_cache(maxsize=None)
def border_cases():
    """one brick under the far wall at 2 m, camera B, no decisive pixel: `inside` and the pixel-box skip"""
    s = setup("B")
    far = mm_image(s, FAR_MM)
    out = []
    for name, (su, sv, cls, why) in BORDER.items():
        su, sv = (sp if sp == MID else (sp[0], sp[1] * (n - 1) + sp[2]) for sp, n in ((su, s.W), (sv, s.H)))
        t = placed_pose(s, 2.0, su, sv)
        v = pr.box_class(s, pyramid_of(s, far), pr.brick_box(s, I3, np.asarray(t), 0, 0, 0), "brick")
        out.append(PCase(f"B_{name}", "B", s, t, "brick", name, (0, 0, 0), None, None, v.level, v.window, (name,), far, far))
    return tuple(out)


# ---- the cell list: a ragged second cell at the image border ------------------------------------------------------------------------------------
CELL_DIMS, CELL_ORIGIN = (40, 40, 40), (0.0, 0.0, 0.0)
CELL_POSES = {"corner": (-0.186, -0.686, 2.0), "edge": (-2.0, -0.6, 0.5)}


@functools.lru_cache(maxsize=None)
def cell_cases():
    """A 40^3-voxel grid: 5 bricks per axis, so the second 4x4x4-brick cell of every axis holds ONE brick layer, 12 voxels from the
    centre the cell's bounding sphere is drawn around.  R = I.
    corner: from 2 m, the grid's +x and +y faces at the right and lower image border: every brick is in view.
    edge:   from 0.5 m and 2 m to the side: the left image border cuts the grid along its last brick layer in x -- of the ragged
            cells in x only that layer exists, and nothing else of the grid is in view; the other bricks fall to the sphere tests.
    One decisive pixel under a brick of the layer bx = 4, for the free and for the skip rule (edge: no brick is wholly inside the
    image, so there is no free case)."""
    s = setup("A", CELL_DIMS, CELL_ORIGIN)
    out = []
    for (pose_name, tt), (rule, base_mm) in itertools.product(CELL_POSES.items(), (("free_invalid", FAR_MM), ("skip_far", NEAR_MM))):
        t = np.asarray(tt)
        base = mm_image(s, base_mm)
        truth = pr.voxel_truth(s, to_f32(base), I3, t)
        found = False
        for bz, by in itertools.product(range(5), (4, 3, 2, 1, 0)):
            brick = (4, by, bz)
            v0 = pr.box_class(s, pyramid_of(s, base), pr.brick_box(s, I3, t, *brick), "brick")
            if v0.why != "box" or v0.cls != (FREE if rule == "free_invalid" else SKIP):
                continue
            for tags, pixel, zc in _candidates_of(s, "brick", v0, truth, brick, None)[:4]:
                name = f"A_cell_{pose_name}_{rule}_b{brick[0]}{brick[1]}{brick[2]}_u{pixel[0]}v{pixel[1]}"
                case = PCase(name, "A", s, tt, "brick", rule, brick, None, pixel, v0.level, v0.window, tags + ("cell_list",),
                             _plant(base, pixel, 0 if rule == "free_invalid" else FAR_MM), base)
                if is_decisive(case):
                    out.append(case)
                    found = True
                    break
            if found:
                break
    # the edge pose under the far wall, no decisive pixel: the bricks the border cuts are MIXED, nothing is free
    far = mm_image(s, FAR_MM)
    out.append(PCase("A_cell_edge_far", "A", s, CELL_POSES["edge"], "brick", "edge_far", (4, 4, 3), None, None, 0, (0, 0), ("cell_list",), far, far))
    return tuple(out)


def all_cases():
    return cases() + border_cases() + cell_cases()


# ---- what a seeded fault of the model does to a case --------------------------------------------------------------------------------------------
def target_class(case: PCase, mm, fault=None):
    s, t = case.s, np.asarray(case.t)
    pyr = pr.pyramid_by_reduction(s, to_f32(mm), 1.0, fault) if fault in pr.PYRAMID_FAULTS else pyramid_of(s, mm)
    return pr.box_class(s, pyr, target_box(s, case.R, t, case.brick, case.sub), case.kind, fault).cls


def target_permits(case: PCase, mm):
    """(skip permitted, free permitted) for the case's target by the per-voxel truth of the image"""
    truth = pr.voxel_truth(case.s, to_f32(mm), case.R, np.asarray(case.t))
    cell = 8 if case.sub is None else 4
    i0, j0, k0 = (8 * b for b in case.brick) if case.sub is None else pr.subbrick_origin(*case.brick, case.sub)
    skip_ok, free_ok = pr.permitted(truth, cell)
    return bool(skip_ok[k0 // cell, j0 // cell, i0 // cell]), bool(free_ok[k0 // cell, j0 // cell, i0 // cell])


def fault_effect(case: PCase, fault):
    """"unsound": with the fault the model answers skip / free for the target where the per-voxel truth forbids it;
    "loose": it answers MIXED for the image without the decisive pixel, where the faultless model decides the target whole"""
    for mm in (case.mm, case.mm_base):
        cls = target_class(case, mm, fault)
        skip_ok, free_ok = target_permits(case, mm)
        if (cls == SKIP and not skip_ok) or (cls == FREE and not free_ok):
            return "unsound"
    if target_class(case, case.mm_base) != MIXED and target_class(case, case.mm_base, fault) == MIXED:
        return "loose"
    return None
