"""Crafted images for the depth-frame filter, shared by the CPU reference tests and the GPU tests.

A case is (name, image, params): image float32 or uint16 [H, W], params the keyword arguments of the filter (jump_rel, radius,
min_support, min_region).  The support pass works on 64 x 16 pixel tiles: x = 64, 128, ... are tile seams, y = 16, 32, ... block-row
seams; a thread takes rows 4 apart.  Nothing here is random but the `noise` images, which come from a fixed seed."""
import numpy as np

F32 = np.float32
TILE_W, TILE_H = 64, 16
DEFAULTS = dict(jump_rel=0.05, radius=1, min_support=4, min_region=0)


def prm(**kw):
    out = dict(DEFAULTS)
    out.update(kw)
    return out


def ulp_up(x):
    return np.nextafter(F32(x), F32(np.inf))


def ulp_down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def blank(h, w, dtype=np.float32):
    return np.zeros((h, w), dtype)


# ---- the smallest cases, with their answers written by hand -------------------------------------------------------------------
def hand_cases():
    """[(name, image, params, expected image, expected counts)]"""
    out = []
    # a 3x3 plateau: the centre has 8 supports, an edge 5, a corner 3.  min_support 4 drops the corners, 6 leaves the centre, 3 keeps all.
    p = np.full((3, 3), 2.0, F32)
    e4 = p.copy(); e4[[0, 0, 2, 2], [0, 2, 0, 2]] = 0
    e6 = np.zeros((3, 3), F32); e6[1, 1] = 2.0
    out.append(("plateau3_s4", p, prm(min_support=4), e4, [9, 4, 0, 0]))
    out.append(("plateau3_s6", p, prm(min_support=6), e6, [9, 8, 0, 0]))
    out.append(("plateau3_s3", p, prm(min_support=3), p.copy(), [9, 0, 0, 0]))
    out.append(("plateau3_s8", p, prm(min_support=8), e6, [9, 8, 0, 0]))
    # one pixel alone: 0 supports; kept only by min_support 0, and then a region of one
    one = np.full((1, 1), 5.0, F32)
    out.append(("one_s0", one, prm(min_support=0), one.copy(), [1, 0, 0, 0]))
    out.append(("one_s1", one, prm(min_support=1), np.zeros((1, 1), F32), [1, 1, 0, 0]))
    out.append(("one_s0_region2", one, prm(min_support=0, min_region=2), np.zeros((1, 1), F32), [1, 0, 1, 1]))
    out.append(("one_s0_region1", one, prm(min_support=0, min_region=1), one.copy(), [1, 0, 0, 0]))
    # a row 1.00 1.04 1.08 1.12 at jump 0.05: neighbours are linked, 1.00 and 1.08 are not: a non-transitive chain, ONE region of 4
    row = np.array([[1.0, 1.04, 1.08, 1.12]], F32)
    out.append(("chain_region4", row, prm(min_support=1, min_region=4), row.copy(), [4, 0, 1, 0]))
    out.append(("chain_region5", row, prm(min_support=1, min_region=5), np.zeros((1, 4), F32), [4, 0, 1, 4]))
    # two pixels across a jump: no support for either
    jump = np.array([[1.0, 2.0]], F32)
    out.append(("jump_pair", jump, prm(min_support=1), np.zeros((1, 2), F32), [2, 2, 0, 0]))
    # the diagonal: with radius 1 the two support each other (stage A is 8-connected), stage B (4-connected) sees two regions of one
    dia = np.array([[1.0, 0.0], [0.0, 1.0]], F32)
    out.append(("diagonal_a", dia, prm(min_support=1), dia.copy(), [2, 0, 0, 0]))
    out.append(("diagonal_b", dia, prm(min_support=1, min_region=2), np.zeros((2, 2), F32), [2, 0, 2, 2]))
    # invalid pixels keep their bits and support nobody
    bad = np.array([[np.nan, -1.0, 3.0, 3.0, -0.0, np.inf]], F32)
    out.append(("invalid_kept", bad, prm(min_support=1), bad.copy(), [2, 0, 0, 0]))
    out.append(("invalid_kept_s2", bad, prm(min_support=2), np.array([[np.nan, -1.0, 0.0, 0.0, -0.0, np.inf]], F32), [2, 2, 0, 0]))
    # u16: 1000 and 1050 are linked at 0.05 (50 <= 50), 1000 and 1051 are not
    out.append(("u16_linked", np.array([[1000, 1050]], np.uint16), prm(min_support=1), np.array([[1000, 1050]], np.uint16), [2, 0, 0, 0]))
    out.append(("u16_apart", np.array([[1000, 1051]], np.uint16), prm(min_support=1), np.array([[0, 0]], np.uint16), [2, 2, 0, 0]))
    return out


# ---- builders ---------------------------------------------------------------------------------------------------------------
def noise_image(h, w, seed, dtype=np.float32, invalid=0.08, fliers=0.04):
    """a slanted plane with a step, some invalid pixels of every kind and some isolated fliers"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = 1.5 + 0.004 * xx + 0.003 * yy + np.where(xx + yy > (h + w) // 2, 0.6, 0.0)
    d = d * (1.0 + 0.01 * rng.standard_normal((h, w)))
    fl = rng.random((h, w)) < fliers
    d[fl] = d[fl] * rng.uniform(0.5, 1.6, int(fl.sum()))
    if dtype == np.uint16:
        img = np.clip(np.rint(d * 1000.0), 1, 65535).astype(np.uint16)
        img[rng.random((h, w)) < invalid] = 0
        return img
    img = d.astype(F32)
    bad = rng.random((h, w)) < invalid
    kinds = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -2.5], F32)
    img[bad] = kinds[rng.integers(0, len(kinds), int(bad.sum()))]
    return img


def seam_pairs(h, w, radius, dtype=np.float32):
    """isolated little groups whose supporter and supported pixel lie on opposite sides of a tile seam, of a block-row seam, and in
    the image's corners and on its borders; `radius` apart, so that only a window of that radius sees them"""
    img = blank(h, w, dtype)
    val = 1200 if dtype == np.uint16 else 1.2
    r = radius
    spots = []
    for sx in range(TILE_W, w, TILE_W):            # across every tile seam, at several rows
        for y in (0, 3, TILE_H - 1, TILE_H, h - 1):
            if y < h and sx - 1 >= 0 and sx - 1 + r < w:
                spots.append(((y, sx - 1), (y, sx - 1 + r)))
    for sy in range(TILE_H, h, TILE_H):            # across every block-row seam
        for x in (0, 5, TILE_W - 1, TILE_W, w - 1):
            if x < w and sy - 1 + r < h:
                spots.append(((sy - 1, x), (sy - 1 + r, x)))
    for (y, x) in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):          # corners: a diagonal partner r away
        yy, xx = (y + r if y == 0 else y - r), (x + r if x == 0 else x - r)
        if 0 <= yy < h and 0 <= xx < w:
            spots.append(((y, x), (yy, xx)))
    taken = np.zeros((h, w), bool)
    for a, b in spots:                             # keep groups 2r + 1 apart so that they do not support each other
        y0, y1 = min(a[0], b[0]) - 2 * r - 1, max(a[0], b[0]) + 2 * r + 2
        x0, x1 = min(a[1], b[1]) - 2 * r - 1, max(a[1], b[1]) + 2 * r + 2
        if taken[max(0, y0):y1, max(0, x0):x1].any():
            continue
        img[a], img[b] = val, val
        taken[a], taken[b] = True, True
    return img


def support_ladder(radius, dtype=np.float32):
    """per group: a centre with exactly k supporters in its window, k = 0 .. (2r+1)^2 - 1, groups far apart; laid out over tiles"""
    r = radius
    win = 2 * r + 1
    n = win * win
    pitch = 2 * win + 1
    cols = 6
    rows = -(-n // cols)
    h, w = rows * pitch + 2, cols * pitch + 3
    img = blank(h, w, dtype)
    val = 900 if dtype == np.uint16 else 0.9
    far = 3000 if dtype == np.uint16 else 3.0           # fills the rest of the window with valid but unlinked pixels
    for k in range(n):
        cy, cx = (k // cols) * pitch + win, (k % cols) * pitch + win
        cells = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]
        for j, (dy, dx) in enumerate(cells):
            img[cy + dy, cx + dx] = val if j < k else (far if j % 2 else 0)
        img[cy, cx] = val
    return img


def link_boundary_cases():
    """pairs whose |d_q - d_p| equals the rounded product exactly, and sits one f32 ulp to either side; both orders"""
    out = []
    for jump, lo in ((0.0625, 1.0), (0.25, 3.0), (0.05, 1.0), (0.05, 2.7182817), (0.3, 0.001)):
        lo = F32(lo)
        prod = F32(F32(jump) * lo)
        hi = F32(lo + prod)
        for tag, h in (("at", hi), ("below", ulp_down(hi)), ("above", ulp_up(hi)), ("above2", ulp_up(ulp_up(hi)))):
            for order in ("lo_hi", "hi_lo"):
                pair = np.array([[lo, h] if order == "lo_hi" else [h, lo]], F32)
                col = np.ascontiguousarray(pair.T)
                name = f"link_j{jump}_lo{float(lo):g}_{tag}_{order}"
                out.append((name + "_a", pair, prm(jump_rel=jump, min_support=1)))
                out.append((name + "_b", pair, prm(jump_rel=jump, min_support=0, min_region=2)))
                out.append((name + "_col_b", col, prm(jump_rel=jump, min_support=0, min_region=2)))
    for a, b in ((1000, 1050), (1000, 1051), (1000, 1049), (1050, 1000), (1051, 1000), (1, 1), (1, 2), (2, 1), (0, 1), (65535, 65535),
                 (65535, 62415), (62415, 65535), (65535, 62414), (62414, 65535), (65535, 0), (20, 21), (21, 20), (19, 20), (40, 42), (40, 43)):
        pair = np.array([[a, b]], np.uint16)
        out.append((f"link_u16_{a}_{b}_a", pair, prm(min_support=1)))
        out.append((f"link_u16_{a}_{b}_b", pair, prm(min_support=0, min_region=2)))
    return out


def region_blobs(min_region, dtype=np.float32):
    """blobs of exactly min_region and min_region - 1 pixels (rows that wrap), well apart, some across seams"""
    h, w = 40, 70
    img = blank(h, w, dtype)
    val = 2000 if dtype == np.uint16 else 2.0
    for i, (y0, x0, n) in enumerate(((1, 1, min_region), (1, 28, min_region - 1), (6, 50, min_region), (20, 28, min_region - 1),
                                     (30, 2, min_region), (14, 60, min_region - 1))):
        width = 6
        for k in range(n):
            img[y0 + k // width, x0 + k % width] = val
    return img


def checkerboard(h, w, dtype=np.float32):
    img = blank(h, w, dtype)
    yy, xx = np.mgrid[0:h, 0:w]
    img[(yy + xx) % 2 == 0] = 1500 if dtype == np.uint16 else 1.5
    return img


def spiral(h, w, dtype=np.float32):
    """a one-pixel-wide rectangular spiral with one-pixel gaps: one long 4-connected path over many tiles"""
    img = blank(h, w, dtype)
    val = 1000 if dtype == np.uint16 else 1.0
    top, left, bottom, right = 0, 0, h - 1, w - 1
    img[0, 0:w] = val
    while bottom - top >= 2 and right - left >= 2:
        img[top:bottom + 1, right] = val                     # down the right side
        img[bottom, left:right + 1] = val                    # along the bottom
        img[top + 2:bottom + 1, left] = val                  # up the left side, stopping two below the top row
        top += 2
        img[top, left:right - 1] = val                       # along the next top row, stopping two before the right side
        left += 2
        bottom -= 2
        right -= 2
    return img


def comb(h, w, dtype=np.float32):
    """vertical teeth on every other column that join only in the last row"""
    img = blank(h, w, dtype)
    val = 1000 if dtype == np.uint16 else 1.0
    img[:, ::2] = val
    img[h - 1, :] = val
    return img


def slope_comb(h, w):
    """the comb with depth growing along the path, so that pixels far apart in the region are far apart in depth too"""
    img = comb(h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = (1.0 + 0.01 * xx + 0.002 * (h - 1 - yy)).astype(F32)
    return np.where(img > 0, ramp, F32(0)).astype(F32)


def stage_a_cuts(dtype=np.float32):
    """two 3 x 6 blocks joined by a one-pixel-wide neck of three pixels: 39 pixels, one region.  With min_support 3 the middle neck
    pixel (2 supports) goes in stage A and cuts the shape into halves of 19 pixels, which min_region 30 then removes; with
    min_support 0 the whole shape is one region of 39 and stays"""
    img = blank(12, 40, dtype)
    val = 1000 if dtype == np.uint16 else 1.0
    img[4:7, 2:8] = val            # 18 pixels
    img[5, 8:11] = val             # neck: each neck pixel has at most 2 linked neighbours but the ends
    img[4:7, 11:17] = val          # 18 pixels
    return img


# ---- the list ---------------------------------------------------------------------------------------------------------------
def crafted_cases():
    """[(name, image, params)], every image at most about 200 x 150"""
    cases = [(n, i, p) for n, i, p, _e, _c in hand_cases()]
    cases += link_boundary_cases()
    for dt, tag in ((np.float32, "f32"), (np.uint16, "u16")):
        # shapes: 1x1, 1xN, Nx1, narrower than a halo, no multiple of the tile in either axis
        for (h, w) in ((1, 1), (1, 45), (45, 1), (2, 5), (5, 2), (13, 37), (33, 129), (16, 64), (17, 65)):
            for r in (1, 2, 3):
                full = np.full((h, w), 1000 if dt == np.uint16 else 1.0, dt)
                cases.append((f"full_{tag}_{h}x{w}_r{r}", full, prm(radius=r, min_support=min(4, (2 * r + 1) ** 2 - 1), min_region=6)))
                cases.append((f"noise_{tag}_{h}x{w}_r{r}", noise_image(h, w, 100 * h + w + r, dt), prm(radius=r, min_support=r + 1, min_region=3)))
        for r in (1, 2, 3):
            cases.append((f"seams_{tag}_r{r}", seam_pairs(41, 150, r, dt), prm(radius=r, min_support=1)))
            cases.append((f"seams_{tag}_r{r}_s2", seam_pairs(41, 150, r, dt), prm(radius=r, min_support=2)))
            n = (2 * r + 1) ** 2
            for ms in sorted({0, 1, 4, n // 2, n - 2, n - 1}):
                cases.append((f"ladder_{tag}_r{r}_s{ms}", support_ladder(r, dt), prm(radius=r, min_support=ms)))
        for mr in (2, 7, 20):
            cases.append((f"blobs_{tag}_{mr}", region_blobs(mr, dt), prm(min_support=0, min_region=mr)))
            cases.append((f"blobs_{tag}_{mr}_s1", region_blobs(mr, dt), prm(min_support=1, min_region=mr)))
        cases.append((f"checker_{tag}_a", checkerboard(21, 70, dt), prm(min_support=4)))
        cases.append((f"checker_{tag}_b", checkerboard(21, 70, dt), prm(min_support=2, min_region=2)))
        cases.append((f"spiral_{tag}_keep", spiral(61, 131, dt), prm(min_support=1, min_region=500)))
        cases.append((f"spiral_{tag}_drop", spiral(61, 131, dt), prm(min_support=1, min_region=100000)))
        cases.append((f"comb_{tag}_keep", comb(50, 150, dt), prm(min_support=1, min_region=3000)))
        cases.append((f"comb_{tag}_drop", comb(50, 150, dt), prm(min_support=1, min_region=5000)))
        cases.append((f"cut_{tag}_no_a", stage_a_cuts(dt), prm(min_support=0, min_region=30)))
        cases.append((f"cut_{tag}_a", stage_a_cuts(dt), prm(min_support=3, min_region=30)))
        cases.append((f"all_valid_{tag}", np.full((30, 50), 700 if dt == np.uint16 else 0.7, dt), prm(min_region=10)))
        cases.append((f"all_invalid_{tag}", blank(30, 50, dt), prm(min_region=10)))
        cases.append((f"noise_{tag}_big", noise_image(150, 200, 7, dt), prm(min_region=12)))
        cases.append((f"noise_{tag}_big_r3", noise_image(150, 200, 8, dt), prm(radius=3, min_support=20, min_region=40)))
    cases.append(("slope_comb_keep", slope_comb(50, 150), prm(min_support=1, min_region=3000)))
    cases.append(("all_nan", np.full((9, 40), np.nan, F32), prm(min_region=5)))
    cases.append(("mixed_invalid", np.tile(np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1.0, 1.0], F32), (11, 9)), prm(min_support=2, min_region=4)))
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def by_shape(cases):
    """{(h, w): [case]} in first-seen order: the GPU tests make one context per shape"""
    out = {}
    for c in cases:
        out.setdefault(tuple(c[1].shape), []).append(c)
    return out
