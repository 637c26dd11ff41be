"""Crafted parts for the mesh weld (tl3d_mesh_weld_keyed, FusionContext.weld_meshes, lattice.weld_meshes) whose welded mesh is known BY
CONSTRUCTION: a case starts from the welded mesh's own vertices (distinct keys, each owned by the one box that holds its owner voxel)
and triangles, and cuts it into parts; no weld code takes part in the expected result.

A part lists, in an order of its own, the vertices its core owns and copies of vertices other cores own (halo copies: the ones its
triangles name, plus some no triangle names).  A halo copy carries a position and a colour that differ from the owner's, so a weld
that took either from the wrong copy shows.  The expected result: the owned vertices in part order, then in the part's own order; all
triangles in part order, each corner the output index of the vertex's one owned copy.

Each case is built once per process (functools.lru_cache) and must not be modified by a test: copy what you change."""
import ctypes as C
import functools

import numpy as np

import keytab_common as kt


def key_of(i, j, k, axis, L):
    return 3 * ((int(k) * int(L[1]) + int(j)) * int(L[0]) + int(i)) + int(axis)


def owner_part(keys, L, boxes):
    """the index of the box that holds each key's owner voxel, -1 where none does"""
    idx = np.asarray(keys, np.int64) // 3
    lx, ly = int(L[0]), int(L[1])
    x, y, z = idx % lx, (idx // lx) % ly, idx // (lx * ly)
    part = np.full(len(idx), -1, np.int64)
    for p, (lo, hi) in enumerate(boxes):
        m = (x >= lo[0]) & (x < hi[0]) & (y >= lo[1]) & (y < hi[1]) & (z >= lo[2]) & (z < hi[2])
        assert np.all(part[m] == -1), "the boxes overlap"
        part[m] = p
    return part


def assemble(L, boxes, keys, xyz, rgb, lists, tris):
    """The parts and the welded mesh of a construction.  keys / xyz / rgb [G]: the welded mesh's vertices (every key in one box);
    lists[p]: the global vertex ids part p lists, in its order; tris[p]: [n, 3] global ids, all of them in lists[p].
    Returns (parts, want, info): parts as lattice.weld_meshes takes them, want = (xyz, rgb, tris, keys), info: per part the owner
    part of every triangle corner (`corner_owner`), and the global ids in output order (`order`)."""
    part = owner_part(keys, L, boxes)
    G = len(keys)
    out_index = np.full(G, -1, np.int64)
    base, parts, corner_owner, order, want_tris = 0, [], [], [], []
    for p, (lo, hi) in enumerate(boxes):
        lst = np.asarray(lists[p], np.int64)
        own = part[lst] == p
        assert len(np.unique(lst[own])) == int(own.sum()), "a part lists an owned vertex twice"
        out_index[lst[own]] = base + np.arange(int(own.sum()))
        base += int(own.sum())
        order.append(lst[own])
    assert np.all(out_index >= 0), "a vertex no part lists as owned"
    for p, (lo, hi) in enumerate(boxes):
        lst = np.asarray(lists[p], np.int64)
        own = part[lst] == p
        tp = np.asarray(tris[p], np.int64).reshape(-1, 3)
        pos = np.full(G, -1, np.int64)
        pos[lst] = np.arange(len(lst))                    # (a vertex listed twice: the later position; cases here list each once)
        assert np.all(pos[tp] >= 0), "a triangle names a vertex its part does not list"
        pxyz, prgb = xyz[lst].copy(), rgb[lst].copy()
        pxyz[~own] += np.float32(1000.0)                  # a halo copy is recognisably not the owner's
        prgb[~own] ^= np.uint8(0xFF)
        parts.append((pxyz, prgb, pos[tp].astype(np.uint32), keys[lst].copy(), tuple(int(v) for v in lo), tuple(int(v) for v in hi)))
        want_tris.append(out_index[tp].astype(np.uint32))
        corner_owner.append(part[tp])
    order = np.concatenate(order) if order else np.zeros(0, np.int64)
    want = (xyz[order], rgb[order], np.concatenate(want_tris) if want_tris else np.zeros((0, 3), np.uint32), keys[order])
    return parts, want, dict(corner_owner=corner_owner, order=order, part=part)


def _distinct_keys(rng, n, end):
    keys = np.unique(rng.integers(0, end, size=n, dtype=np.int64))
    while len(keys) < n:
        keys = np.unique(np.concatenate([keys, rng.integers(0, end, size=n - len(keys), dtype=np.int64)]))
    rng.shuffle(keys)
    return keys


def _vertices(rng, n):
    return rng.standard_normal((n, 3)).astype(np.float32), rng.integers(0, 256, (n, 3), dtype=np.uint8)


def soup_parts(L, boxes, G, T, seed):
    """G distinct random keys in the lattice with random xyz and rgb; T triangles, half of them with all corners in the first corner's
    part, the other half with corners anywhere; a triangle belongs to the part that owns its first corner.  A part lists its owned
    vertices, the halo vertices its triangles name and 10 % extra halo copies no triangle names, shuffled.  The boxes tile L."""
    rng = np.random.default_rng(seed)
    nvox = int(L[0]) * int(L[1]) * int(L[2])
    keys = _distinct_keys(rng, G, 3 * nvox)
    xyz, rgb = _vertices(rng, G)
    part = owner_part(keys, L, boxes)
    assert np.all(part >= 0), "the boxes do not cover the lattice"
    tri = rng.integers(0, G, (T, 3))
    tpart = part[tri[:, 0]]
    local = np.arange(T) < T // 2
    members = [np.flatnonzero(part == p) for p in range(len(boxes))]
    for p, mem in enumerate(members):
        sel = np.flatnonzero(local & (tpart == p))
        tri[sel, 1:] = mem[rng.integers(0, len(mem), (len(sel), 2))]
    lists, tris = [], []
    for p, mem in enumerate(members):
        tp = tri[tpart == p]
        named = np.unique(tp)
        halo = named[part[named] != p]
        spare = np.setdiff1d(np.flatnonzero(part != p), halo)
        extra = rng.choice(spare, size=min(len(spare), (len(mem) + len(halo)) // 10), replace=False)
        lst = np.concatenate([mem, halo, extra])
        rng.shuffle(lst)
        lists.append(lst)
        tris.append(tp)
    return assemble(L, boxes, keys, xyz, rgb, lists, tris)


SIZED_L = (96, 16, 16)
SIZED = [(2047, 5, 2048), (2048, 0, 2047), (2049, 2048, 0), (0, 300, 2049), (1, 0, 1), (4097, 1, 4097)]     # (owned, halo, triangles)


def sized_parts(seed=5):
    """Six 16^3 cores along x, (owned, halo, triangles) per part as SIZED: both sides of the chunk of 2048, a part that owns nothing
    (its triangles resolve through the table only), a part with halo copies and no triangles, a part of one vertex with the
    triangle (0, 0, 0)."""
    rng = np.random.default_rng(seed)
    L = SIZED_L
    boxes = [((16 * p, 0, 0), (16 * p + 16, 16, 16)) for p in range(len(SIZED))]
    per_core = 3 * 16 ** 3
    keys, start = [], [0]
    for p, (own, _h, _t) in enumerate(SIZED):
        loc = rng.choice(per_core, size=own, replace=False)           # (voxel in the core, axis)
        v, axis = loc // 3, loc % 3
        keys.append(np.array([key_of(16 * p + int(a % 16), int((a // 16) % 16), int(a // 256), int(ax), L) for a, ax in zip(v, axis)], np.int64))
        start.append(start[-1] + own)
    keys = np.concatenate(keys)
    G = len(keys)
    xyz, rgb = _vertices(rng, G)
    lists, tris = [], []
    for p, (own, halo, nt) in enumerate(SIZED):
        mine = np.arange(start[p], start[p + 1])
        others = np.concatenate([np.arange(0, start[p]), np.arange(start[p + 1], G)])
        h = rng.choice(others, size=halo, replace=False)
        lst = np.concatenate([mine, h])
        if own > 1:
            rng.shuffle(lst)
        t = lst[rng.integers(0, len(lst), (nt, 3))] if nt else np.zeros((0, 3), np.int64)
        if nt and halo:                                               # every halo copy a part with triangles lists is named at least once
            t[rng.permutation(nt)[:min(nt, halo)], 1] = h[:min(nt, halo)]
        lists.append(lst)
        tris.append(t)
    return assemble(L, boxes, keys, xyz, rgb, lists, tris)


WRAP_L = (1 << 21, 1 << 20, (1 << 20) - 8)                # (the lattice of soup_wide)
WRAP_KEPT = 512                                           # half of the smallest key table


def wrap_parts(seed=17):
    """The key table at its smallest capacity, filled to exactly half, every probe sequence running into the end of the array:
    WRAP_KEPT keys of the lower x half of WRAP_L whose sequences start in the last 8 of 1024 slots (keytab_common.wrapping).
    Part 0 (core: the lower x half) owns them all and has some triangles of its own; part 1 (core: the upper half) owns nothing,
    lists a halo copy of every one, and its triangles name each of them at least once, so every lookup walks a wrapped chain."""
    rng = np.random.default_rng(seed)
    L = WRAP_L

    def draw(rng, count):
        v = np.stack([rng.integers(0, L[0] // 2, count), rng.integers(0, L[1], count), rng.integers(0, L[2], count), rng.integers(0, 3, count)],
                     axis=1)
        return (3 * ((v[:, 2] * L[1] + v[:, 1]) * L[0] + v[:, 0]) + v[:, 3]).astype(np.uint64), v
    v = kt.wrapping(rng, WRAP_KEPT, draw)
    keys = np.array([key_of(i, j, k, axis, L) for i, j, k, axis in v], np.int64)
    G = len(keys)
    xyz, rgb = _vertices(rng, G)
    t1 = rng.integers(0, G, (G + 88, 3))
    t1[:G, 0] = rng.permutation(G)                        # every halo copy is named
    lists = [rng.permutation(G), rng.permutation(G)]
    tris = [rng.integers(0, G, (100, 3)), t1]
    return assemble(L, _halves(L, (0,)), keys, xyz, rgb, lists, tris)


def seam_case():
    """two blocks along x, six kept vertices (one of them unreferenced), one seam vertex (the case of tests/test_blocks_host.py)"""
    L = (16, 8, 8)
    ka = np.array([key_of(7, 0, 0, 0, L), key_of(8, 0, 0, 1, L), key_of(7, 1, 0, 1, L), key_of(3, 3, 3, 2, L), key_of(9, 2, 2, 0, L)], np.int64)
    xa = np.arange(15, dtype=np.float32).reshape(5, 3)
    ra = np.arange(15, dtype=np.uint8).reshape(5, 3)
    ta = np.array([[0, 1, 2]], np.uint32)
    kb = np.array([key_of(8, 0, 0, 1, L), key_of(9, 2, 2, 0, L), key_of(12, 4, 4, 2, L)], np.int64)
    xb = np.array([[3, 4, 5], [12, 13, 14], [100, 100, 100]], np.float32)
    rb = np.array([[3, 4, 5], [12, 13, 14], [9, 9, 9]], np.uint8)
    tb = np.array([[0, 1, 2]], np.uint32)
    parts = [(xa, ra, ta, ka, (0, 0, 0), (8, 8, 8)), (xb, rb, tb, kb, (8, 0, 0), (16, 8, 8))]
    want = (np.concatenate([xa[[0, 2, 3]], xb]), np.concatenate([ra[[0, 2, 3]], rb]), np.array([[0, 3, 1], [3, 4, 5]], np.uint32),
            np.concatenate([ka[[0, 2, 3]], kb]))
    return L, parts, want


def coincident_case():
    """two vertices at one position with different keys stay apart; the second part is empty"""
    L = (16, 8, 8)
    k = np.array([key_of(7, 3, 3, 0, L), key_of(7, 3, 3, 1, L), key_of(6, 3, 3, 2, L)], np.int64)
    x = np.array([[1, 1, 1], [1, 1, 1], [2, 2, 2]], np.float32)
    r = np.zeros((3, 3), np.uint8)
    t = np.array([[0, 1, 2]], np.uint32)
    parts = [(x, r, t, k, (0, 0, 0), (8, 8, 8)), (x[:0], r[:0], t[:0], k[:0], (8, 0, 0), (16, 8, 8))]
    return L, parts, (x, r, t, k)


def _halves(L, axes):
    """the boxes of a lattice halved along each of `axes`"""
    cuts = [[0, int(L[a]) // 2, int(L[a])] if a in axes else [0, int(L[a])] for a in range(3)]
    return [((cuts[0][i], cuts[1][j], cuts[2][k]), (cuts[0][i + 1], cuts[1][j + 1], cuts[2][k + 1]))
            for k in range(len(cuts[2]) - 1) for j in range(len(cuts[1]) - 1) for i in range(len(cuts[0]) - 1)]


def _block_boxes(dims, max_voxels):
    from tl3d import pipeline as pl
    from tl3d.fusion import GridSpec
    lat = GridSpec(tuple(dims), (0.0, 0.0, 0.0), 0.01, 0.04)
    out = []
    for b in pl.plan_blocks(lat, max_voxels):
        off = np.asarray(b.grid.voxel_offset, np.int64)
        out.append((tuple(int(v) for v in off + np.asarray(b.lo)), tuple(int(v) for v in off + np.asarray(b.hi))))
    return out


SOUPS = ("soup_small", "soup_blocks", "soup_wide")
CASES = SOUPS + ("sized", "wrap", "seam", "coincident")


@functools.lru_cache(maxsize=None)
def case(name):
    """(L, parts, want, info) of a named case; info is None for the hand-made ones"""
    if name == "soup_small":            # eight boxes that are no multiples of 8
        L = (64, 48, 40)
        return (L,) + soup_parts(L, _halves(L, (0, 1, 2)), 5000, 9000, 11)
    if name == "soup_blocks":           # the 8 blocks of plan_blocks: long probe chains in both tables
        L = (256, 256, 256)
        boxes = _block_boxes(L, 136 ** 3)
        assert len(boxes) == 8
        return (L,) + soup_parts(L, boxes, 1 << 18, 1 << 19, 12)
    if name == "soup_wide":             # keys up to 3 * 2^61: beyond fp64 and 32-bit arithmetic
        L = (1 << 21, 1 << 20, (1 << 20) - 8)
        return (L,) + soup_parts(L, _halves(L, (0, 1)), 1 << 16, 1 << 17, 13)
    if name == "sized":
        return (SIZED_L,) + sized_parts()
    if name == "wrap":                  # the smallest key table, half full, every chain wrapping round its end
        return (WRAP_L,) + wrap_parts()
    if name == "seam":
        return seam_case() + (None,)
    if name == "coincident":
        return coincident_case() + (None,)
    raise KeyError(name)


def same_bytes(got, want):
    """all four arrays of a welded mesh equal another's in shape, type and bytes"""
    for g, w, dtype in zip(got, want, (np.float32, np.uint8, np.uint32, np.int64)):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype != dtype or w.dtype != dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            return False
    return True


def raw_call(ctx, parts, L, vert_cap=None, tri_cap=None, outs=None, n_parts=None, counts=True, fix=None):
    """tl3d_mesh_weld_keyed itself, on host arrays, with the context handle ctx (None: a NULL ctx).  Capacities default to the sums
    of the parts' sizes, outs to fresh arrays (xyz, rgb, key, tri; an entry may be None); fix(arr) edits the MeshPart array before
    the call; counts=False passes one NULL count.  Returns (code, message, [n_vert, n_tri, n_twice, n_unowned], outs); a count the
    call did not store reads -7."""
    from tl3d import _cabi as abi
    lib = abi.load()
    arr = (abi.MeshPart * max(1, len(parts)))()
    hold = []
    for m, (x, r, t, k, lo, hi) in zip(arr, parts):
        x, t, k = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(t, np.uint32), np.ascontiguousarray(k, np.int64)
        r = None if r is None else np.ascontiguousarray(r, np.uint8)
        hold.append((x, r, t, k))
        m.xyz_hd, m.key_hd, m.tri_hd = x.ctypes.data, k.ctypes.data, t.ctypes.data
        m.rgb_hd = None if r is None else r.ctypes.data
        m.n_vert, m.n_tri = len(x), len(t)
        for a in range(3):
            m.core_lo[a], m.core_hi[a] = int(lo[a]), int(hi[a])
    if fix:
        fix(arr)
    nv, nt = sum(len(h[0]) for h in hold), sum(len(h[2]) for h in hold)
    outs = outs or (np.empty((nv, 3), np.float32), np.empty((nv, 3), np.uint8), np.empty(nv, np.int64), np.empty((nt, 3), np.uint32))
    c = [C.c_int64(-7) for _ in range(4)]
    refs = [C.byref(v) for v in c] if counts else [C.byref(c[0]), None, C.byref(c[2]), C.byref(c[3])]
    dims = None if L is None else (C.c_int64 * 3)(*[int(d) for d in L])
    rc = lib.tl3d_mesh_weld_keyed(ctx, arr, len(parts) if n_parts is None else n_parts, dims, abi.ptr(outs[0]), abi.ptr(outs[1]),
                                  abi.ptr(outs[2]), nv if vert_cap is None else vert_cap, abi.ptr(outs[3]),
                                  nt if tri_cap is None else tri_cap, *refs)
    return rc, lib.tl3d_last_error().decode(), [v.value for v in c], outs
