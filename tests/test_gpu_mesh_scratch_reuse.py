"""GPU: the mesh calls (csrc/api_mesh.hip) and the cloud calls carve their device scratch from two buffers of the context
(scratch_carve, csrc/api_host.h): whatever a call finds there is what an earlier call of any kind left behind.  One assertion:
every call of a sequence on ONE context returns, bit for bit and dtype for dtype, what the same call returns on a fresh context.

The sequence takes the buffers through what can go wrong: the widest first carve (quadric simplify, which leaves sums and 0xFF
tables behind), small calls of every kind over it, both second-stage arrays (smoothing's neighbour list, the weld's key table) over
each other's remains, both buffers growing in mid-sequence, and the cloud calls on the buffer the mesh calls use.  Two sizes of an
indexed sheet with colours: under one compaction chunk (2048) in vertices and triangles, and several chunks of each.  No reference
here: the mesh tests hold each call to its host reference.  Public API only; once with numpy arrays, once with device tensors."""
import numpy as np
import pytest

import mesh_simplify_common as msc
import mesh_simplify_quadric_common as mqc
import mesh_smooth_common as smc
import mesh_weld_common as mwc
import tl3d

pytestmark = pytest.mark.gpu

SMALL, LARGE = 9, 97                                      # vertices per side: 81 / 128 and 9409 / 18432 vertices / triangles
assert 2 * (SMALL - 1) ** 2 < smc.CHUNK and LARGE ** 2 > 4 * smc.CHUNK and 2 * (LARGE - 1) ** 2 > 8 * smc.CHUNK
CELL = 0.025                                              # 2.5 grid steps: clusters of 4 to 9 vertices


def _fresh():
    return tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1)


def _sheet(n):
    """a noisy n x n height field at a spacing of 1 cm (as mesh_smooth_common.sheet), coloured, with the triangles of all its quads"""
    rng = np.random.default_rng(n)
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 2)
    xyz = np.concatenate([g * 0.01, 0.8 + 0.002 * rng.standard_normal((n * n, 1))], axis=1).astype(np.float32)
    return xyz, msc._colours(rng, n * n), np.ascontiguousarray(mqc._grid_tris(n, n).astype(np.uint32))


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def _flat(out):
    """a call's result as a list of numpy arrays: tuples and info dicts taken apart, device tensors fetched, numbers wrapped"""
    if isinstance(out, dict):
        out = [out[k] for k in sorted(out)]
    if isinstance(out, (tuple, list)):
        return [a for o in out for a in _flat(o)]
    if out is None:
        return []
    return [out.cpu().numpy() if hasattr(out, "data_ptr") else np.asarray(out)]


def _calls(device):
    conv = _dev if device else (lambda a: a)
    (sx, sr, st), (lx, lr, lt) = [tuple(conv(a) for a in _sheet(n)) for n in (SMALL, LARGE)]
    L, parts, _, _ = mwc.case("seam")
    parts = [tuple(conv(a) for a in p[:4]) + tuple(p[4:]) for p in parts]
    pts = _sheet(SMALL)[0]                                                      # (the outlier filter takes numpy only)
    return [
        ("large quadric simplify", lambda c: c.simplify_mesh(lx, lr, lt, CELL, placement="quadric")),
        ("small components", lambda c: c.mesh_components(st, SMALL * SMALL)),
        ("small filter", lambda c: c.filter_mesh(sx, sr, st, min_triangles=1)),
        ("small smooth", lambda c: c.smooth_mesh(sx, st, 2)),
        ("weld", lambda c: c.weld_meshes(parts, L)),
        ("large smooth", lambda c: c.smooth_mesh(lx, lt, 2)),
        ("small mean simplify", lambda c: c.simplify_mesh(sx, sr, st, CELL)),
        ("small normals", lambda c: c.mesh_normals(sx, st)),
        ("weld again", lambda c: c.weld_meshes(parts, L)),
        ("small nearest_triangles", lambda c: c.nearest_triangles(sx, sx, st)),
        ("small outlier", lambda c: c.statistical_outlier(pts, 8, 2.0, cell_size=0.02)),
        ("small components again", lambda c: c.mesh_components(st, SMALL * SMALL)),
    ]


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_a_dirty_scratch_does_not_show(device):
    """every call of the sequence on ONE context gives, bit for bit, what the same call gives on a fresh context"""
    calls = _calls(device)
    with _fresh() as one:
        shared = [_flat(call(one)) for _, call in calls]
    for (what, call), got in zip(calls, shared):
        with _fresh() as c:
            alone = _flat(call(c))
        assert len(got) == len(alone) and len(got) > 0, what
        for a, b in zip(got, alone):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
    for a, b in zip(shared[1], shared[-1]):
        assert a.dtype == b.dtype and np.array_equal(a, b), "components before and after"
