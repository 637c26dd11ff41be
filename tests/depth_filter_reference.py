"""Two independent numpy formulations of the depth-frame filter (include/tl3d.h: tl3d_filter_depth).

  filter_shifted   shifted-array numpy for the supports and the joins, scipy.sparse.csgraph.connected_components for the regions
  filter_loops     a plain per-pixel loop for the supports, breadth-first search for the regions

Both take one image (float32, or uint16 millimetres) and return (filtered image of the same dtype, int64 [4] counts = valid in,
removed by A, regions after A, removed by B).  All arithmetic is numpy.float32 on the pixel itself (a uint16 value converted
exactly): one rounded difference, one rounded product, one compare.  The filter only writes zeros, and only over valid pixels."""
from collections import deque

import numpy as np

F32 = np.float32


def as_f32(img):
    img = np.asarray(img)
    assert img.ndim == 2 and img.dtype in (np.float32, np.uint16), (img.shape, img.dtype)
    return img.astype(F32)                      # exact for uint16


def valid_mask(d):
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def check_params(jump_rel, radius, min_support, min_region):
    assert np.isfinite(jump_rel) and jump_rel > 0
    assert 1 <= radius <= 3 and 0 <= min_support <= (2 * radius + 1) ** 2 - 1 and min_region >= 0


# ---- formulation 1: shifted arrays + scipy ----------------------------------------------------------------------------------
def _linked_arrays(dp, dq, vp, vq, jump):
    """element-wise linked(p, q) of two equally shaped f32 arrays with their validity"""
    with np.errstate(invalid="ignore", over="ignore"):
        return vp & vq & (np.abs(dq - dp) <= jump * np.minimum(dp, dq))


def filter_shifted(img, jump_rel=0.05, radius=1, min_support=4, min_region=0):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    check_params(jump_rel, radius, min_support, min_region)
    d = as_f32(img)
    h, w = d.shape
    jump = F32(jump_rel)
    v = valid_mask(d)
    r = int(radius)
    pad_d = np.zeros((h + 2 * r, w + 2 * r), F32)
    pad_v = np.zeros((h + 2 * r, w + 2 * r), bool)
    pad_d[r:r + h, r:r + w] = np.where(v, d, F32(0))
    pad_v[r:r + h, r:r + w] = v
    s = np.zeros((h, w), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            dq = pad_d[r + dy:r + dy + h, r + dx:r + dx + w]
            vq = pad_v[r + dy:r + dy + h, r + dx:r + dx + w]
            s += _linked_arrays(pad_d[r:r + h, r:r + w], dq, v, vq, jump)
    keep = v & (s >= int(min_support))
    counts = np.zeros(4, np.int64)
    counts[0], counts[1] = int(v.sum()), int((v & ~keep).sum())
    if min_region > 1:
        idx = np.arange(h * w).reshape(h, w)
        dz = np.where(v, d, F32(0))
        right = _linked_arrays(dz[:, :-1], dz[:, 1:], keep[:, :-1], keep[:, 1:], jump)
        down = _linked_arrays(dz[:-1, :], dz[1:, :], keep[:-1, :], keep[1:, :], jump)
        a = np.concatenate([idx[:, :-1][right], idx[:-1, :][down]])
        b = np.concatenate([idx[:, 1:][right], idx[1:, :][down]])
        graph = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(h * w, h * w))
        _, label = connected_components(graph, directed=False)
        label = label.reshape(h, w)
        sizes = np.bincount(label[keep], minlength=h * w)
        counts[2] = int((sizes > 0).sum())
        small = keep & (sizes[label] < int(min_region))
        counts[3] = int(small.sum())
        keep = keep & ~small
    out = np.array(img, copy=True)
    out[v & ~keep] = 0
    return out, counts


# ---- formulation 2: loops + BFS -----------------------------------------------------------------------------------------------
def _valid1(x):
    return bool(np.isfinite(x)) and bool(x > 0)


def _linked1(a, b, jump):
    """linked(p, q) of two VALID f32 scalars"""
    lo = a if a < b else b
    with np.errstate(over="ignore"):
        return bool(np.abs(F32(b - a)) <= F32(jump * lo))


def filter_loops(img, jump_rel=0.05, radius=1, min_support=4, min_region=0):
    check_params(jump_rel, radius, min_support, min_region)
    d = as_f32(img)
    h, w = d.shape
    jump = F32(jump_rel)
    r = int(radius)
    v = [[_valid1(d[y, x]) for x in range(w)] for y in range(h)]
    keep = [[False] * w for _ in range(h)]
    n_valid = n_a = 0
    for y in range(h):
        for x in range(w):
            if not v[y][x]:
                continue
            n_valid += 1
            s = 0
            for yy in range(max(0, y - r), min(h, y + r + 1)):
                for xx in range(max(0, x - r), min(w, x + r + 1)):
                    if (yy != y or xx != x) and v[yy][xx] and _linked1(d[y, x], d[yy, xx], jump):
                        s += 1
            keep[y][x] = s >= min_support
            n_a += 0 if keep[y][x] else 1
    n_regions = n_b = 0
    drop = [[v[y][x] and not keep[y][x] for x in range(w)] for y in range(h)]
    if min_region > 1:
        seen = [[False] * w for _ in range(h)]
        for y0 in range(h):
            for x0 in range(w):
                if not keep[y0][x0] or seen[y0][x0]:
                    continue
                n_regions += 1
                seen[y0][x0] = True
                members, todo = [], deque([(y0, x0)])
                while todo:
                    y, x = todo.popleft()
                    members.append((y, x))
                    for yy, xx in ((y, x + 1), (y, x - 1), (y + 1, x), (y - 1, x)):
                        if 0 <= yy < h and 0 <= xx < w and keep[yy][xx] and not seen[yy][xx] and _linked1(d[y, x], d[yy, xx], jump):
                            seen[yy][xx] = True
                            todo.append((yy, xx))
                if len(members) < min_region:
                    n_b += len(members)
                    for y, x in members:
                        drop[y][x] = True
    out = np.array(img, copy=True)
    out[np.array(drop, bool).reshape(h, w)] = 0
    return out, np.array([n_valid, n_a, n_regions, n_b], np.int64)


def bits(a):
    """the raw bits of an image, for equality that tells -0.0 from 0.0 and one NaN from another"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)
