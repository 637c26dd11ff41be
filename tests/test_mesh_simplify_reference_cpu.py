"""CPU: the numpy restatement of the vertex-clustering rules (tests/mesh_simplify_reference.py) against a
dictionary-and-loops restatement on random meshes, on hand-worked cases and against pinned figures on the crafted mesh and the
GPU tests' topologies; the C-ABI call is exported, bound and refuses bad arguments without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import keytab_common as kt
import mesh_simplify_reference as msr
from mesh_simplify_common import CRAFTED, CRAFTED_ORIGIN, FIGURES, TOPOLOGIES, WRAPPED, WRAPPED_VERTS, cell_keys, crafted_mesh, reference
from tl3d import _cabi as abi


def _loops(xyz, rgb, tris, cell, origin=None):
    """the rules of DESIGN.md section 4.2.2 one vertex and one triangle at a time, in Python floats (fp64) and ints"""
    o = [0.0, 0.0, 0.0] if origin is None else [float(v) for v in origin]
    cell = float(cell)
    clusters, vmap = {}, []
    for v, p in enumerate(xyz):
        key, qs = [], []
        for a in range(3):
            d = float(p[a]) - o[a]
            i = math.floor(d / cell)
            r = d - float(i) * cell
            qs.append(int(np.rint((r / cell) * 16777216.0)))
            key.append(i)
        rec = clusters.setdefault(tuple(key), dict(id=len(clusters), n=0, s=[0, 0, 0], c=[0, 0, 0]))       # dicts keep insertion order
        rec["n"] += 1
        for a in range(3):
            rec["s"][a] += qs[a]
            if rgb is not None:
                rec["c"][a] += int(rgb[v][a])
        vmap.append(rec["id"])
    pos, col = [], []
    for key, rec in clusters.items():
        pos.append([np.float32(o[a] + (float(key[a]) + float(rec["s"][a]) / (float(rec["n"]) * 16777216.0)) * cell) for a in range(3)])
        col.append([(2 * rec["c"][a] + rec["n"]) // (2 * rec["n"]) for a in range(3)])
    seen, out, deg, dup = set(), [], 0, 0
    for t in tris:
        m = [vmap[int(t[0])], vmap[int(t[1])], vmap[int(t[2])]]
        if m[0] == m[1] or m[1] == m[2] or m[0] == m[2]:
            deg += 1
            continue
        k = m.index(min(m))
        canon = (m[k], m[(k + 1) % 3], m[(k + 2) % 3])
        if canon in seen:
            dup += 1
            continue
        seen.add(canon)
        out.append(m)
    return (np.array(pos, np.float32).reshape(-1, 3), np.array(col, np.uint8).reshape(-1, 3) if rgb is not None else None,
            np.array(out, np.uint32).reshape(-1, 3), dict(clusters=len(clusters), vertices_in=len(xyz), triangles_in=len(tris),
                                                          degenerate_dropped=deg, duplicates_dropped=dup, vert_map=np.array(vmap, np.uint32)))


def _assert_same(got, want, what=""):
    for a, b, name in zip(got[:3], want[:3], ("xyz", "rgb", "tris")):
        if a is None or b is None:
            assert a is None and b is None, f"{what} {name}"
        else:
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what} {name}"
    for k in ("clusters", "vertices_in", "triangles_in", "degenerate_dropped", "duplicates_dropped"):
        assert got[3][k] == want[3][k], (what, k, got[3][k], want[3][k])
    assert got[3]["vert_map"].dtype == np.uint32 and np.array_equal(got[3]["vert_map"], want[3]["vert_map"]), what + " vert_map"


@pytest.mark.parametrize("seed", range(6))
def test_reference_equals_loops_on_random_meshes(seed):
    rng = np.random.default_rng(100 + seed)
    nv, nt = int(rng.integers(1, 2001)), int(rng.integers(0, 4000))
    xyz = rng.normal(0.0, 0.3, size=(nv, 3)).astype(np.float32)
    face = rng.random(nv) < 0.2
    xyz[face] = np.round(xyz[face] * 8) / 8                         # some on cell faces
    rgb = rng.integers(0, 256, size=(nv, 3), dtype=np.uint8) if seed % 3 else None
    near = np.clip(rng.integers(0, nv, size=(nt, 1)) + rng.integers(-6, 7, size=(nt, 3)), 0, nv - 1)
    tris = np.concatenate([near, near[: nt // 4, [2, 0, 1]], near[: nt // 8, ::-1]]).astype(np.uint32)
    cell = (0.125, 0.05, 0.31, 1.0, 0.0078125, 0.2)[seed]
    origin = None if seed % 2 else (0.01 * seed, -0.37, 1.0 / 3.0)
    got = msr.simplify(xyz, rgb, tris, cell, origin)
    _assert_same(got, _loops(xyz, rgb, tris, cell, origin), f"seed {seed}")
    assert got[0].dtype == np.float32 and got[2].dtype == np.uint32 and (rgb is None or got[1].dtype == np.uint8)


def test_two_triangles_sharing_an_edge_that_collapses():
    # b and c share a cell: the edge (b, c) collapses, both triangles become degenerate; a third one far away survives
    xyz = np.array([(0.1, 0.1, 0.1), (1.1, 0.1, 0.1), (1.2, 0.2, 0.1), (2.1, 0.1, 0.1), (0.1, 3.1, 0.1), (5.5, 0.5, 0.5)], np.float32)
    tris = np.array([(0, 1, 2), (2, 1, 3), (0, 3, 4), (0, 1, 4)], np.uint32)
    x, c, t, info = msr.simplify(xyz, None, tris, 1.0)
    assert c is None and info["clusters"] == 5 and np.array_equal(info["vert_map"], [0, 1, 1, 2, 3, 4])
    assert np.array_equal(t, [(0, 2, 3), (0, 1, 3)]) and info["degenerate_dropped"] == 2 and info["duplicates_dropped"] == 0
    # the merged vertex is the mean of its members, the others stay where they were up to 2^-24 of a cell; the cluster no
    # triangle names (vertex 5) is an output vertex all the same
    q = np.rint((np.array([0.1, 0.2], np.float32).astype(np.float64)) * 16777216.0)
    assert x[1, 1] == np.float32(0.0 + (0.0 + q.sum() / (2.0 * 16777216.0)) * 1.0)
    assert np.abs(x[[0, 2, 3, 4]] - xyz[[0, 3, 4, 5]]).max() <= 2.0 ** -24 and len(x) == 5


def test_rotations_are_duplicates_and_the_reversed_triangle_is_not():
    xyz = np.array([(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, 1.5, 0.5)], np.float32)
    tris = np.array([(2, 0, 1), (0, 1, 2), (1, 2, 0), (1, 0, 2), (2, 1, 0)], np.uint32)       # three rotations, two reversed
    x, _, t, info = msr.simplify(xyz, None, tris, 1.0)
    assert np.array_equal(t, [(2, 0, 1), (1, 0, 2)])                # the first of each winding, as listed: mapped, not rotated
    assert info["duplicates_dropped"] == 3 and info["degenerate_dropped"] == 0
    assert np.array_equal(x, xyz)


def test_colour_mean_rounds_halves_up():
    xyz = np.full((4, 3), 0.5, np.float32)
    rgb = np.array([(0, 10, 255), (1, 10, 255), (0, 11, 254), (0, 11, 255)], np.uint8)       # means 0.25, 10.5, 254.75
    assert np.array_equal(msr.simplify(xyz, rgb, np.zeros((0, 3), np.uint32), 1.0)[1], [(0, 11, 255)])
    assert np.array_equal(msr.simplify(xyz[:2], rgb[:2], np.zeros((0, 3), np.uint32), 1.0)[1], [(1, 10, 255)])      # 0.5 -> 1
    assert np.array_equal(msr.simplify(xyz[:3], rgb[:3], np.zeros((0, 3), np.uint32), 1.0)[1], [(0, 10, 255)])      # 1/3, 31/3, 764/3


@pytest.mark.parametrize("origin", [None, (0.75, -0.25, 8.0)])
def test_a_vertex_on_a_cell_face_belongs_to_the_cell_above(origin):
    o = np.zeros(3) if origin is None else np.array(origin)
    ks = np.array([-5, -2, 0, 3, 7])
    cell = 0.25                                                     # k * cell and o + k * cell are exact in f32 here
    xyz = np.stack([o[0] + ks * cell, np.full(5, o[1] + 0.1), np.full(5, o[2] + 0.1)], axis=1).astype(np.float32)
    i, q = msr.cells(xyz, cell, origin)
    assert np.array_equal(i[:, 0], ks) and not q[:, 0].any()
    below = xyz.copy()
    below[:, 0] = np.nextafter(xyz[:, 0], np.float32(-np.inf))
    i, q = msr.cells(below, cell, origin)
    assert np.array_equal(i[:, 0], ks - 1) and (q[:, 0] > 16777216 - 64).all() and (q[:, 0] <= 16777216).all()
    x, _, _, info = msr.simplify(np.concatenate([xyz, below]), None, np.zeros((0, 3), np.uint32), cell, origin)
    assert info["clusters"] == 10 and np.array_equal(x[:5, 0], xyz[:, 0])


def test_vertices_out_of_range_are_refused():
    ok = np.array([(0.5, 0.5, 0.5)], np.float32)
    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (1048576.0, 0, 0), (0, -1048577.0, 0)):
        with pytest.raises(ValueError):
            msr.simplify(np.concatenate([ok, np.array([bad], np.float32)]), None, np.zeros((0, 3), np.uint32), 1.0)
    assert msr.simplify(np.array([(1048575.5, -1048576.0, 0)], np.float32), None, np.zeros((0, 3), np.uint32), 1.0)[3]["clusters"] == 1
    for cell, origin in ((0.0, None), (-1.0, None), (np.nan, None), (1.0, (0, np.nan, 0))):
        with pytest.raises(ValueError):
            msr.simplify(ok, None, np.zeros((0, 3), np.uint32), cell, origin)
    with pytest.raises(ValueError):
        msr.simplify(ok, None, np.array([(0, 0, 1)], np.uint32), 1.0)


def _assert_box_property(inp, want):
    """every output vertex lies in the closed box of its cell, up to the f32 rounding of the result"""
    xyz, rgb, tris, cell, origin = inp
    o = np.zeros(3) if origin is None else np.asarray(origin, np.float64)
    i, _ = msr.cells(xyz, cell, origin)
    ic = np.zeros((want[3]["clusters"], 3), np.int64)
    ic[want[3]["vert_map"]] = i
    lo, hi = (o + ic * float(cell)).astype(np.float32), (o + (ic + 1) * float(cell)).astype(np.float32)
    assert (want[0] >= np.nextafter(lo, np.float32(-np.inf))).all() and (want[0] <= np.nextafter(hi, np.float32(np.inf))).all()


@pytest.mark.parametrize("cell", sorted(CRAFTED))
def test_crafted_mesh_figures(cell):
    xyz, rgb, tris = crafted_mesh(0)
    assert (len(xyz), len(tris)) == (5135, 9188)
    want = msr.simplify(xyz, rgb, tris, cell)
    x, c, t, info = want
    assert (len(x), len(t), info["duplicates_dropped"]) == CRAFTED[cell]
    assert info["clusters"] == len(x) == len(c) and info["degenerate_dropped"] + info["duplicates_dropped"] + len(t) == 9188
    _assert_same(want, _loops(xyz, rgb, tris, cell), f"cell {cell}")
    _assert_box_property((xyz, rgb, tris, cell, None), want)
    shifted = msr.simplify(xyz, rgb, tris, cell, CRAFTED_ORIGIN)
    _assert_same(shifted, _loops(xyz, rgb, tris, cell, CRAFTED_ORIGIN), f"cell {cell}, shifted")
    _assert_box_property((xyz, rgb, tris, cell, CRAFTED_ORIGIN), shifted)
    # winding: a surviving triangle is its input triangle, mapped
    m = info["vert_map"][tris.astype(np.int64)]
    rows = {tuple(r) for r in m.tolist()}
    assert all(tuple(r) in rows for r in t.tolist())


@pytest.mark.parametrize("name", TOPOLOGIES)
def test_topology_figures(name):
    inp, want = reference(name)
    assert (len(want[0]), len(want[2]), want[3]["degenerate_dropped"], want[3]["duplicates_dropped"]) == FIGURES[name]
    _assert_box_property(inp, want)
    if name == "cell finer than the spacing":                       # nothing merges: the triangle list comes back unchanged
        assert np.array_equal(want[2], inp[2]) and np.array_equal(want[3]["vert_map"], np.arange(len(inp[0])))
    if name.startswith("axis lines") or name == "doubled sheet":
        _assert_same(want, _loops(*inp), name)


@pytest.mark.parametrize("name", WRAPPED)
def test_wrapped_chains_fill_the_smallest_table_with_chains_that_wrap(name):
    """the two conditions that keep the cases from going hollow, by the Python copy of the mixer and of the sizing rule; and their
    pinned figures"""
    inp, want = reference(name)
    xyz, rgb, tris, cell, origin = inp
    i, _ = msr.cells(xyz, cell, origin)
    assert np.abs(i).max() < 1 << 20 and np.array_equal(cell_keys(i) >> np.uint64(42), (i[:, 0] + (1 << 20)).astype(np.uint64))
    keys = cell_keys(i)
    assert len(xyz) == WRAPPED_VERTS == 512 and kt.kt_slots(len(xyz)) == 1024 and kt.kt_slots(len(xyz) + 1) == 2048
    assert kt.start_slot(keys, 1024).min() >= 1016                  # more keys than slots to the end: every chain wraps
    distinct = len(np.unique(keys))
    if name.endswith("shared"):                                     # the second half lies in cells of the first half
        assert distinct == len(np.unique(keys[:256])) == 256 and np.isin(keys[256:], keys[:256]).all()
        assert not (xyz[256:] == xyz[want[3]["vert_map"][256:]]).all(axis=1).any()       # ... and nowhere on their leaders
    else:
        assert distinct == 512                                      # exactly half of the table
    assert (len(want[0]), len(want[2]), want[3]["degenerate_dropped"], want[3]["duplicates_dropped"]) == FIGURES[name]
    assert want[3]["clusters"] == distinct and 300 <= len(tris) <= 500
    _assert_box_property(inp, want)
    _assert_same(want, _loops(*inp), name)


# ---- the C-ABI without a GPU --------------------------------------------------------------------------------------------------
def test_call_is_exported_and_bound():
    lib = abi.load()
    assert "tl3d_mesh_simplify_clusters" in abi.SYMBOLS and hasattr(lib, "tl3d_mesh_simplify_clusters")
    assert len(lib.tl3d_mesh_simplify_clusters.argtypes) == 18 and lib.tl3d_mesh_simplify_clusters.restype is C.c_int


def test_argument_validation_needs_no_gpu():
    """Every check but the two scans is decided before the first device call: made here with a null context, which is refused too,
    but last, so the message tells which check answered."""
    lib = abi.load()
    tris = np.array([[0, 1, 2], [2, 3, 4]], np.uint32)
    xyz, rgb = np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8)
    oxyz, orgb, otri, vmap = np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8), np.zeros((2, 3), np.uint32), np.zeros(5, np.uint32)
    counts = [C.c_int64(-7) for _ in range(4)]

    def call(**kw):
        a = dict(xyz=xyz, rgb=rgb, n_vert=5, tri=tris, n_tri=2, cell=0.5, origin=None, oxyz=oxyz, orgb=orgb, vcap=5, otri=otri, tcap=2,
                 vmap=vmap)
        a.update(kw)
        o = None if a["origin"] is None else (C.c_double * 3)(*a["origin"])
        rc = lib.tl3d_mesh_simplify_clusters(None, abi.ptr(a["xyz"]), abi.ptr(a["rgb"]), a["n_vert"], abi.ptr(a["tri"]), a["n_tri"],
                                             a["cell"], o, abi.ptr(a["oxyz"]), abi.ptr(a["orgb"]), a["vcap"], abi.ptr(a["otri"]), a["tcap"],
                                             abi.ptr(a["vmap"]), *[C.byref(c) for c in counts])
        return rc, lib.tl3d_last_error()
    for kw, msg in ((dict(n_tri=-2), b"negative size"), (dict(n_vert=-1), b"negative size"), (dict(n_vert=1 << 31), b"2^31"),
                    (dict(n_tri=1 << 32), b"2^32"), (dict(vcap=-1), b"negative capacity"), (dict(tcap=-1), b"negative capacity"),
                    (dict(cell=0.0), b"cell size"), (dict(cell=-0.5), b"cell size"), (dict(cell=float("nan")), b"cell size"),
                    (dict(cell=float("inf")), b"cell size"), (dict(origin=(0.0, float("nan"), 0.0)), b"origin"),
                    (dict(origin=(float("inf"), 0.0, 0.0)), b"origin"), (dict(xyz=None), b"null vertex list"),
                    (dict(tri=None), b"null triangle list"), (dict(oxyz=None), b"null output"), (dict(orgb=None), b"null output"),
                    (dict(otri=None), b"null output"), (dict(oxyz=xyz), b"aliases"), (dict(orgb=rgb), b"aliases"),
                    (dict(otri=tris), b"aliases"), (dict(vmap=tris.reshape(-1)[1:]), b"aliases"),
                    (dict(oxyz=tris.view(np.float32)), b"aliases"), (dict(), b"null ctx"), (dict(rgb=None, orgb=None), b"null ctx"),
                    (dict(vmap=None, origin=(1.0, 2.0, 3.0)), b"null ctx")):
        rc, err = call(**kw)
        assert rc == abi.E_INVALID and msg in err, (kw.keys(), err)
    assert [c.value for c in counts] == [-7] * 4 and not oxyz.any() and not otri.any() and not vmap.any()       # nothing written
