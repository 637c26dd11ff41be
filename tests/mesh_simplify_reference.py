"""numpy restatement of the vertex-clustering rules: what tl3d_mesh_simplify_clusters must give, bit
for bit.  No reference code exists (the reference has no mesh); the rules are the project's own."""
import numpy as np

Q = 16777216.0          # 2^24 steps per cell
RANGE = 1 << 20         # cell indices lie in [-2^20, 2^20)


def cells(xyz, cell, origin=None):
    """(i int64 [V,3], q int64 [V,3]) per axis: d = (double)x - o, i = floor(d / cell), r = d - i * cell, q = rint(r / cell * 2^24);
    ValueError for a vertex that is not finite or lies 2^20 cells or more away"""
    o = np.zeros(3) if origin is None else np.asarray(origin, np.float64)
    cell = np.float64(cell)
    if not (np.isfinite(cell) and cell > 0 and np.isfinite(o).all()):
        raise ValueError("cell / origin")
    with np.errstate(all="ignore"):
        d = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64) - o
        fi = np.floor(d / cell)
        if not ((fi >= -RANGE) & (fi < RANGE)).all():
            raise ValueError("a vertex is not finite or out of range")
        r = d - fi * cell
        q = np.rint((r / cell) * Q).astype(np.int64)
    return fi.astype(np.int64), q


def simplify(xyz, rgb, tris, cell, origin=None):
    """(xyz f32 [K,3], rgb u8 [K,3] or None, tris u32 [T',3], info) with info = clusters, vertices_in, triangles_in,
    degenerate_dropped, duplicates_dropped, vert_map (u32 [V])"""
    o = np.zeros(3) if origin is None else np.asarray(origin, np.float64)
    tris = np.asarray(tris, np.uint32).reshape(-1, 3)
    i, q = cells(xyz, cell, o)
    if len(tris) and tris.max() >= len(i):
        raise ValueError("index out of range")
    key = ((i[:, 0] + RANGE) << 42) | ((i[:, 1] + RANGE) << 21) | (i[:, 2] + RANGE)
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                   # clusters in the order of their smallest member
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    vmap = rank[inv.reshape(-1)]
    k = len(order)
    n = np.bincount(vmap, minlength=k).astype(np.int64)
    s = np.zeros((k, 3), np.int64)
    np.add.at(s, vmap, q)
    ic = i[first[order]].astype(np.float64).reshape(k, 3)
    pos = (o + (ic + s.astype(np.float64) / (n[:, None].astype(np.float64) * Q)) * np.float64(cell)).astype(np.float32)
    col = None
    if rgb is not None:
        c = np.zeros((k, 3), np.int64)
        np.add.at(c, vmap, np.asarray(rgb, np.uint8).reshape(-1, 3).astype(np.int64))
        col = ((2 * c + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    m = vmap[tris.astype(np.int64)].reshape(-1, 3)
    deg = (m[:, 0] == m[:, 1]) | (m[:, 1] == m[:, 2]) | (m[:, 0] == m[:, 2])
    idx = np.flatnonzero(~deg)
    mm = m[idx]
    rot = (np.argmin(mm, axis=1)[:, None] + np.arange(3)[None, :]) % 3
    canon = np.take_along_axis(mm, rot, axis=1)                # smallest index first, winding kept
    firsts = np.unique(canon, axis=0, return_index=True)[1] if len(canon) else np.zeros(0, np.int64)
    keep = np.sort(idx[firsts])
    info = dict(clusters=k, vertices_in=len(i), triangles_in=len(tris), degenerate_dropped=int(deg.sum()),
                duplicates_dropped=int(len(idx) - len(keep)), vert_map=vmap.astype(np.uint32))
    return pos, col, m[keep].astype(np.uint32).reshape(-1, 3), info
