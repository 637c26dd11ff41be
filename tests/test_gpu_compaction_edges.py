"""GPU: the two mesh-in / mesh-out calls (tl3d_mesh_filter_components, tl3d_mesh_simplify_clusters) at the element counts where the
bounds of the compaction loop they share (csrc/compact.h) can go wrong: one element, one short of / exactly / one over an iteration
of 256 and a chunk of 2048, and two chunks plus one.  Against the references of the component and simplification tests, byte for
byte, counts included, from host arrays and from device tensors."""
import numpy as np
import pytest

import tl3d
from compaction_edges_common import CELL, FIGURES, MIN_TRIANGLES, SIZES, figures, reference
from helpers import SMALL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    """a context without a grid: the calls need none"""
    with tl3d.FusionContext(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], n_slots=1, grid=None) as c:
        yield c


def _dev(a):
    import torch
    a = np.array(a)                                                 # (a writable copy: the shared inputs are read-only)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _assert_same(got, want, keys, per_vertex, what):
    """the three arrays and the per-vertex array byte for byte, every count equal"""
    for a, b, name in (*zip(got[:3], want[:3], ("xyz", "rgb", "tris")), (got[3][per_vertex], want[3][per_vertex], per_vertex)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, name)
    for k in keys:
        assert got[3][k] == want[3][k], (what, k, got[3][k], want[3][k])


def _from_device(result, per_vertex):
    x, r, t, info = result
    assert x.is_cuda and r.is_cuda and t.is_cuda and info[per_vertex].is_cuda
    return _host(x), _host(r), _host(t), dict(info, **{per_vertex: _host(info[per_vertex])})


@pytest.mark.parametrize("n_tri", SIZES)
def test_filter_components(ctx, n_tri):
    assert figures(n_tri) == FIGURES[n_tri]
    mesh, want, _ = reference(n_tri)
    keys = ("components", "components_kept", "vertices_dropped", "triangles_dropped")
    got = ctx.filter_mesh(*mesh, MIN_TRIANGLES)
    assert (len(got[0]), len(got[2])) == FIGURES[n_tri][1]
    _assert_same(got, want, keys, "keep_vert", f"T {n_tri}, host")
    dev = ctx.filter_mesh(*(_dev(a) for a in mesh), MIN_TRIANGLES)
    _assert_same(_from_device(dev, "keep_vert"), want, keys, "keep_vert", f"T {n_tri}, device")


@pytest.mark.parametrize("n_tri", SIZES)
def test_simplify_clusters(ctx, n_tri):
    assert figures(n_tri) == FIGURES[n_tri]
    mesh, _, want = reference(n_tri)
    keys = ("clusters", "vertices_in", "triangles_in", "degenerate_dropped", "duplicates_dropped")
    got = ctx.simplify_mesh(*mesh, CELL)
    assert (len(got[0]), len(got[2]), got[3]["degenerate_dropped"], got[3]["duplicates_dropped"]) == FIGURES[n_tri][2]
    _assert_same(got, want, keys, "vert_map", f"T {n_tri}, host")
    dev = ctx.simplify_mesh(*(_dev(a) for a in mesh), CELL)
    _assert_same(_from_device(dev, "vert_map"), want, keys, "vert_map", f"T {n_tri}, device")
