"""A plain numpy model of what the refinement of a replayed classification entry (kernels_tsdf.hip: class_refine_kernel) decides:
per voxel, whether the 8x8-pixel tile under its pixel leaves it OPEN, makes it SKIP ("behind everything") or FREE ("in front of
everything": tsdf == 1 exactly); per (frame, MIXED sub-brick) pair, the class that follows from its 64 lanes.  TEST REFERENCE ONLY.

Built on prep_classes_reference: voxel_truth's projection for the lanes, the level-0 tiles of pyramid_by_reduction for the tile
records, robust_classes for which sub-bricks the box test leaves MIXED (the pairs the kernel sees).  Like that model it is not
kept bit-equal with the GPU; a frame is compared with the GPU only if every answer is the same under the model's own
perturbations: the pixel moved by +-0.25 px per axis, the voxel's depth by +-0.5 % of a voxel (27 moves), and the boxes by
prep_classes_reference.perturbations()."""
from __future__ import annotations

import itertools

import numpy as np

from oracle import second_numpy as sn
import prep_classes_reference as pr
from prep_classes_reference import F32, MIXED

OPEN, SKIP_LANE, FREE_LANE = 0, 1, 2
PAIR_CLASSES = ("open", "dropped", "free", "both")


def lane_moves(s: pr.Setup):
    e = 0.005 * s.voxel
    return tuple(itertools.product((0.0, -0.25, 0.25), (0.0, -0.25, 0.25), (0.0, -e, e)))


def tile_records(s: pr.Setup, depth, scale=1.0):
    """(x, y) per level-0 tile [ty, tx] as the update reads them: x = lowest depth if all 64 pixels are valid else -inf,
    y = highest valid depth (-inf if none)"""
    lo, hi, ok = pr.pyramid_by_reduction(s, depth, scale)[0]
    x = np.where(np.asarray(ok, bool), np.asarray(lo, F32), F32(-np.inf)).astype(F32)
    return x, np.asarray(hi, F32)


def lane_decisions(s: pr.Setup, depth, R, t, scale=1.0, move=(0.0, 0.0, 0.0)):
    """per voxel [nz, ny, nx]: OPEN / SKIP_LANE / FREE_LANE by rule (4), the pixel moved by move[:2] and the depth by move[2]"""
    g = s.geometry()
    nx, ny, nz = g.dims
    r, tt = sn._pose32(R, t)
    half = F32(0.5)
    wx = sn.fma32(np.arange(nx, dtype=F32) + half, g.voxel, g.origin[0])
    wy = sn.fma32(np.arange(ny, dtype=F32) + half, g.voxel, g.origin[1])
    wz = sn.fma32(np.arange(nz, dtype=F32) + half, g.voxel, g.origin[2])
    K, J, I = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    xc, yc, zc = sn._transform(r, tt, wx[I], wy[J], wz[K])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = F32(1.0) / zc
        uf = sn.fma32(g.fx * xc, inv, g.cx) + F32(move[0])
        vf = sn.fma32(g.fy * yc, inv, g.cy) + F32(move[1])
        win = (zc > F32(0)) & (uf >= F32(-0.5)) & (uf < F32(g.W) - F32(0.5)) & (vf >= F32(-0.5)) & (vf < F32(g.H) - F32(0.5))
        u = np.clip(np.where(win, np.floor(uf + half), 0), 0, g.W - 1).astype(np.int64)
        v = np.clip(np.where(win, np.floor(vf + half), 0), 0, g.H - 1).astype(np.int64)
        x, y = tile_records(s, depth, scale)
        z = (zc + F32(move[2])).astype(F32)
        fre = win & (x[v >> 3, u >> 3] - z >= F32(g.trunc) * F32(1.001))
        skp = ~win | ~(y[v >> 3, u >> 3] - z >= -F32(g.trunc))
    out = np.full(zc.shape, OPEN, np.int8)
    out[fre] = FREE_LANE
    out[skp] = SKIP_LANE
    return out


def sub_lanes(dec, brick, sb):
    i0, j0, k0 = pr.subbrick_origin(*brick, sb)
    return dec[k0:k0 + 4, j0:j0 + 4, i0:i0 + 4].reshape(-1)


def pair_class(lanes):
    if (lanes == OPEN).any():
        return "open"
    if (lanes == SKIP_LANE).all():
        return "dropped"
    if (lanes == FREE_LANE).all():
        return "free"
    return "both"


def expected(s: pr.Setup, depth, R, t, scale=1.0):
    """What one refinement of this frame must count: dict(seen, open, dropped, free, both, robust, subs) -- subs maps
    (brick, sub-brick) of every pair seen to its class; robust is False if a box class or a lane decision of a pair that is
    seen changes under a perturbation (such a frame is not compared with the GPU)."""
    pyr = pr.pyramid_by_reduction(s, depth, scale)
    decs = [lane_decisions(s, depth, R, t, scale, m) for m in lane_moves(s)]
    robust, subs = True, {}
    for bz, by, bx in itertools.product(*(range(n) for n in s.nb[::-1])):
        brick = (bx, by, bz)
        _, seen = pr.robust_classes(s, pyr, pr.brick_box(s, R, t, *brick), "brick")
        classes = {c[0] for c in seen}
        robust = robust and len(classes) == 1
        if MIXED not in classes:
            continue
        for sb in range(8):
            _, seen = pr.robust_classes(s, pyr, pr.subbrick_box(s, R, t, *pr.subbrick_origin(*brick, sb)), "sub")
            classes = {c[0] for c in seen}
            robust = robust and len(classes) == 1
            if MIXED not in classes:
                continue
            lanes = sub_lanes(decs[0], brick, sb)
            robust = robust and all(np.array_equal(sub_lanes(d, brick, sb), lanes) for d in decs[1:])
            subs[(brick, sb)] = pair_class(lanes)
    out = {k: sum(1 for c in subs.values() if c == k) for k in PAIR_CLASSES}
    out.update(seen=len(subs), robust=robust, subs=subs)
    return out
