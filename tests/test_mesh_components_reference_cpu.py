"""CPU: the scipy restatement of the mesh component rules (tests/mesh_components_reference.py) against a pure-Python union-find
on hand-made meshes and against pinned figures on the crafted grid of test_gpu_mesh.py; the two C-ABI calls are exported, bound
and refuse bad arguments without a GPU."""
import ctypes as C

import numpy as np
import pytest

import mesh_components_reference as mcr
from mesh_components_common import KEPT, crafted_mesh, speck_scene
from tl3d import _cabi as abi


def _union_find(tris, n_vert):
    parent = list(range(n_vert))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for a, b, c in tris:
        for u, v in ((a, b), (b, c)):
            ru, rv = find(int(u)), find(int(v))
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    labels = [find(v) for v in range(n_vert)]
    counts = [0] * n_vert
    for a, _, _ in tris:
        counts[labels[int(a)]] += 1
    return np.array(labels, np.uint32), np.array(counts, np.uint32), len(set(labels))


TET = [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)]
HAND_MADE = {
    "two tetrahedra": (np.array(TET + [tuple(v + 4 for v in t) for t in TET]), 8),
    "a shared vertex": (np.array(TET + [(3, 4, 5), (6, 7, 8)]), 9),
    "degenerate triangles": (np.array([(5, 5, 2), (7, 7, 7), (1, 0, 0), (2, 9, 9), (8, 8, 8)]), 11),
    "isolated vertices": (np.array([(9, 4, 6), (6, 2, 9)]), 12),
    "descending chain": (np.array([(i + 2, i + 1, i) for i in range(20)][::-1]), 22),
    "an empty mesh": (np.zeros((0, 3), np.int64), 0),
    "vertices without triangles": (np.zeros((0, 3), np.int64), 5),
}


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_reference_equals_union_find_on_hand_made_meshes(name):
    tris, n_vert = HAND_MADE[name]
    got, want = mcr.components(tris, n_vert), _union_find(tris, n_vert)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert int(got[1].sum()) == len(tris)
    assert np.array_equal(got[0][got[0]], got[0]) and (got[0] <= np.arange(n_vert)).all()


def test_reference_filter_on_hand_made_meshes():
    tris, n_vert = HAND_MADE["a shared vertex"]                   # components: {0..5} with 5 triangles, {6, 7, 8} with 1
    xyz = np.arange(3 * n_vert, dtype=np.float32).reshape(-1, 3)
    rgb = np.arange(3 * n_vert, dtype=np.uint8).reshape(-1, 3)
    x, c, t, info = mcr.filter_mesh(xyz, rgb, tris, 0)
    assert np.array_equal(x, xyz) and np.array_equal(c, rgb) and np.array_equal(t, tris) and info["components_kept"] == 2
    x, c, t, info = mcr.filter_mesh(xyz, rgb, tris, 2)
    assert np.array_equal(x, xyz[:6]) and np.array_equal(c, rgb[:6]) and np.array_equal(t, tris[:5])
    assert (info["components"], info["components_kept"], info["vertices_dropped"], info["triangles_dropped"]) == (2, 1, 3, 1)
    x, c, t, info = mcr.filter_mesh(xyz, rgb, tris[::-1], 6)
    assert len(x) == 0 and len(t) == 0 and info["components_kept"] == 0
    # the kept triangles are re-indexed: dropping the FIRST component shifts the second one's indices down
    tris2 = np.array([(0, 1, 2), (3, 4, 5), (4, 5, 6)])
    x, _, t, info = mcr.filter_mesh(xyz[:8], None, tris2, 2)
    assert np.array_equal(x, xyz[3:7]) and np.array_equal(t, [(0, 1, 2), (1, 2, 3)]) and info["vertices_dropped"] == 4
    # ties of largest_only go to the smaller label; a mesh without triangles keeps nothing
    x, _, t, _ = mcr.filter_mesh(xyz[:6], None, np.array([(3, 4, 5), (0, 1, 2)]), 0, largest_only=True)
    assert np.array_equal(x, xyz[:3]) and np.array_equal(t, [(0, 1, 2)])
    x, _, t, info = mcr.filter_mesh(xyz[:4], None, np.zeros((0, 3), np.uint32), 0, largest_only=True)
    assert len(x) == 0 and info["components"] == 4 and info["components_kept"] == 0
    x, _, t, info = mcr.filter_mesh(xyz[:4], None, np.zeros((0, 3), np.uint32), 0)
    assert len(x) == 4 and info["components_kept"] == 4


# ---- the crafted grid of test_gpu_mesh.py: three spheres, 2 % exact zeros, unobserved slabs ---------------------------------
@pytest.mark.parametrize("min_weight,figures", [(0, (5135, 9188, 119, 39)), (2, (2234, 328, 1802, 1704))])
def test_crafted_grid_component_figures(min_weight, figures):
    xyz, rgb, tris = crafted_mesh(min_weight)
    labels, counts, n = mcr.components(tris, len(xyz))
    isolated = int(((labels == np.arange(len(xyz))) & (counts == 0)).sum())
    assert (len(xyz), len(tris), n, isolated) == figures
    want = _union_find(tris, len(xyz))
    assert np.array_equal(labels, want[0]) and np.array_equal(counts, want[1]) and n == want[2]
    if min_weight == 0:
        assert sorted(counts[counts > 0].tolist())[-3:] == [1564, 1860, 5445]
        small = counts[(labels == np.arange(len(xyz))) & (counts > 0) & (counts < 1564)]
        assert len(small) == 77 and small.min() == 1 and small.max() == 18


@pytest.mark.parametrize("min_triangles", sorted(KEPT))
def test_crafted_grid_filter_figures(min_triangles):
    xyz, rgb, tris = crafted_mesh(0)
    x, c, t, info = mcr.filter_mesh(xyz, rgb, tris, min_triangles)
    assert (len(x), len(t), info["components_kept"]) == KEPT[min_triangles]
    assert info["components"] == 119 and info["vertices_dropped"] == 5135 - len(x) and info["triangles_dropped"] == 9188 - len(t)
    assert len(c) == len(x) and (len(t) == 0 or t.max() == len(x) - 1 or min_triangles == 0)
    # order-preserving: the kept rows are a subsequence of the input, and the triangles name the same positions as before
    assert np.array_equal(x, xyz[info["keep_vert"]])
    assert np.array_equal(x[t.astype(np.int64)], xyz[tris.astype(np.int64)][info["keep_vert"][tris[:, 0]]])
    if min_triangles == 0:
        assert np.array_equal(x, xyz) and np.array_equal(t, tris)


def test_crafted_grid_largest_component():
    xyz, rgb, tris = crafted_mesh(0)
    x, c, t, info = mcr.filter_mesh(xyz, rgb, tris, 0, largest_only=True)
    assert (len(x), len(t), info["components_kept"]) == (2877, 5445, 1)
    same = mcr.filter_mesh(xyz, rgb, tris, 5445)
    assert np.array_equal(x, same[0]) and np.array_equal(t, same[2])
    assert len(mcr.filter_mesh(xyz, rgb, tris, 5446, largest_only=True)[0]) == 0


# ---- the C-ABI without a GPU --------------------------------------------------------------------------------------------------
def test_calls_are_exported_and_bound():
    lib = abi.load()
    for name in ("tl3d_mesh_components", "tl3d_mesh_filter_components"):
        assert name in abi.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    assert len(lib.tl3d_mesh_components.argtypes) == 7 and len(lib.tl3d_mesh_filter_components.argtypes) == 18


def test_argument_validation_needs_no_gpu():
    """Every check but the index scan is decided before the first device call: made here with a null context, which is refused
    too, but last, so the message tells which check answered."""
    lib = abi.load()
    n = C.c_int64(7)
    tris = np.array([[0, 1, 2], [2, 3, 4]], np.uint32)
    lab, cnt = np.zeros(5, np.uint32), np.zeros(5, np.uint32)

    def components(tri, n_tri, n_vert, label, count, ctx=None):
        return lib.tl3d_mesh_components(ctx, abi.ptr(tri), n_tri, n_vert, abi.ptr(label), abi.ptr(count), C.byref(n)), lib.tl3d_last_error()
    for args, msg in (((tris, -1, 5, lab, cnt), b"negative size"), ((tris, 2, -5, lab, cnt), b"negative size"),
                      ((tris, 2, 1 << 31, lab, cnt), b"2^31"), ((tris, 1 << 32, 5, lab, cnt), b"2^32"),
                      ((None, 2, 5, lab, cnt), b"null triangle list"), ((tris, 2, 5, None, cnt), b"null argument"),
                      ((tris, 2, 5, tris.reshape(-1)[1:], cnt), b"aliases"), ((tris, 2, 5, lab, tris.reshape(-1)[:5]), b"aliases"),
                      ((tris, 2, 5, lab, lab), b"aliases"), ((tris, 2, 5, lab, cnt), b"null ctx"), ((tris, 2, 5, lab, None), b"null ctx")):
        rc, err = components(*args)
        assert rc == abi.E_INVALID and msg in err, (msg, err)

    xyz, rgb = np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8)
    oxyz, orgb, otri, keep = np.zeros((5, 3), np.float32), np.zeros((5, 3), np.uint8), np.zeros((2, 3), np.uint32), np.zeros(5, np.uint8)
    counts = [C.c_int64(0) for _ in range(4)]

    def filt(**kw):
        a = dict(xyz=xyz, rgb=rgb, n_vert=5, tri=tris, n_tri=2, min_tri=1, largest=0, oxyz=oxyz, orgb=orgb, vcap=5, otri=otri, tcap=2,
                 keep=keep)
        a.update(kw)
        rc = lib.tl3d_mesh_filter_components(None, abi.ptr(a["xyz"]), abi.ptr(a["rgb"]), a["n_vert"], abi.ptr(a["tri"]), a["n_tri"],
                                             a["min_tri"], a["largest"], abi.ptr(a["oxyz"]), abi.ptr(a["orgb"]), a["vcap"],
                                             abi.ptr(a["otri"]), a["tcap"], abi.ptr(a["keep"]), *[C.byref(c) for c in counts])
        return rc, lib.tl3d_last_error()
    for kw, msg in ((dict(n_tri=-2), b"negative size"), (dict(n_vert=-1), b"negative size"), (dict(n_vert=1 << 31), b"2^31"),
                    (dict(vcap=-1), b"negative capacity"), (dict(tcap=-1), b"negative capacity"), (dict(xyz=None), b"null vertex list"),
                    (dict(tri=None), b"null triangle list"), (dict(oxyz=None), b"null output"), (dict(orgb=None), b"null output"),
                    (dict(otri=None), b"null output"), (dict(oxyz=xyz), b"aliases"), (dict(orgb=rgb), b"aliases"),
                    (dict(otri=tris), b"aliases"), (dict(keep=rgb.reshape(-1)[3:8]), b"aliases"),
                    (dict(oxyz=tris.view(np.float32)), b"aliases"), (dict(), b"null ctx"), (dict(rgb=None, orgb=None), b"null ctx")):
        rc, err = filt(**kw)
        assert rc == abi.E_INVALID and msg in err, (kw.keys(), err)


def test_speck_scene_meets_the_pipeline_tests_conditions_with_the_references_alone():
    """What test_gpu_mesh_components.py asks of the pipeline, shown here for the oracle's TSDF and the two references: the mesh has
    the scene and the speck as separate components, and the filter at SPECK_MIN_TRIANGLES removes the speck and keeps the scene."""
    from mesh_components_common import SPECK_GRID, SPECK_MIN_TRIANGLES
    from oracle import c_oracle
    import mesh_reference as mr
    from helpers import SMALL
    poses, frames, speck = speck_scene()
    dims, voxel, centre = SPECK_GRID["dims"], SPECK_GRID["voxel"], SPECK_GRID["centre"]
    origin = tuple(centre[i] - 0.5 * dims[i] * voxel for i in range(3))
    orc = c_oracle.Oracle(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], min_depth=0.1, max_depth=50.0,
                          dims=dims, origin=origin, voxel_size=voxel, sdf_trunc=4 * voxel)
    for (d, _), p in zip(frames, poses):
        orc.tsdf_integrate(d, p[0], p[1])
    xyz, rgb, tris = mr.extract_mesh(orc.tsdf, dims, origin, voxel, min_weight=0)
    labels, counts, n = mcr.components(tris, len(xyz))
    near = np.linalg.norm(xyz - speck, axis=1) < 0.1
    speck_labels = np.unique(labels[near])
    assert n >= 2 and near.sum() >= 20 and 0 < counts[speck_labels].max() < SPECK_MIN_TRIANGLES < counts.max()
    assert counts[speck_labels].max() == 68 and counts.max() == 6562
    x, c, t, info = mcr.filter_mesh(xyz, rgb, tris, SPECK_MIN_TRIANGLES)
    assert info["components_kept"] == 1 and len(t) == 6562
    assert not (np.linalg.norm(x - speck, axis=1) < 0.1).any()
