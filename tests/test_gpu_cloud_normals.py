"""GPU: normals and curvature of a point list by k-NN PCA (tl3d_estimate_normals, kernels_normals.hip)
against the fp64 references of tests/cloud_normals_common.py (held to each other and to known answers in
tests/test_cloud_normals_reference_cpu.py) at the edges of the search, of the two list sizes, of the tie rule, of the radius and of
the orientation; the bars are derived there.  Then the raw C ABI: cell size, repetition, host and device pointers, refusals."""
import ctypes as C

import numpy as np
import pytest

import cloud_normals_common as cn
import tl3d
from tl3d import _cabi as abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as c:
        yield c


def _run(ctx, name, k, **kw):
    return ctx.estimate_normals(cn.points(name), k, cell_size=cn.cell_size(name), curvature=True, **kw)


# ---- random clouds -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", cn.RANDOM_K, ids=cn.case_id)
def test_random_cases_meet_the_bar(ctx, name, k):
    r = cn.case_ref(name, k)
    assert not cn.excluded(r).any() and not r.degenerate.any()             # on the reference first
    n, c = _run(ctx, name, k)
    assert n.dtype == np.float32 and c.dtype == np.float32 and ctx.last_normals_degenerate == 0
    cn.check(n, c, r, False, f"{name} k={k}")


# ---- degenerate neighbourhoods ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_n1", "tiny_n2", "same"])
def test_all_degenerate(ctx, name):
    n, c = _run(ctx, name, 20)
    assert not n.any() and not c.any() and ctx.last_normals_degenerate == len(cn.points(name))
    assert not np.signbit(n).any() and not np.signbit(c).any()             # (0, 0, 0), not (-0, ..)


@pytest.mark.parametrize("k", [3, 4, 30])
def test_duplicates(ctx, k):
    r = cn.ref(cn.points("dups"), k)
    assert int(r.degenerate.sum()) == (35 if k < 30 else 0)                # exactly the 25 + 10 copies, on the reference
    n, c = _run(ctx, "dups", k)
    assert ctx.last_normals_degenerate == int(r.degenerate.sum())
    cn.check(n, c, r, False, f"dups k={k}")


# ---- exact answers with ties -----------------------------------------------------------------------------------------------------------
def test_plane_lattice_is_exact(ctx):
    n, c = _run(ctx, "plane_lattice", 9)
    assert np.all(n[:, :2] == 0) and np.all(np.abs(n[:, 2]) == 1) and np.all(c == 0) and ctx.last_normals_degenerate == 0


def test_line_gets_a_perpendicular_unit_vector(ctx):
    n, c = _run(ctx, "line", 20)
    assert ctx.last_normals_degenerate == 0
    assert np.all(np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1) <= cn.F32) and np.all(np.abs(n[:, 0]) <= cn.F32)


def test_isotropic_lattice_interior_is_unit(ctx):
    n, _ = _run(ctx, "lattice", 7)
    inside = cn.sc.lattice_interior()
    assert np.all(np.abs(np.linalg.norm(n[inside].astype(np.float64), axis=1) - 1) <= cn.F32) and ctx.last_normals_degenerate == 0


def test_the_tie_goes_to_the_smaller_index(ctx):
    z, y = [0, 0, 1], [0, 1, 0]
    n, _ = _run(ctx, "tie4", 3)
    assert np.array_equal(np.abs(n), np.float32([z, z, z, y]))
    rev, _ = _run(ctx, "tie4_reversed", 3)
    want = cn.brute(cn.points("tie4_reversed"), 3)
    assert np.array_equal(np.abs(rev), np.abs(want.normals).astype(np.float32))
    assert not np.array_equal(np.abs(rev)[::-1], np.abs(n))                # the same four points, other members


# ---- radius ----------------------------------------------------------------------------------------------------------------------------
def test_radius_keeps_a_point_on_it(ctx):
    for radius, deg in ((0.5, 5), (0.4999, 6)):
        r = cn.ref(cn.points("radius6"), 8, max_radius=radius)
        assert int(r.degenerate.sum()) == deg and r.members[0] == (5 if deg == 5 else 1)
        n, c = _run(ctx, "radius6", 8, max_radius=radius)
        assert ctx.last_normals_degenerate == deg
        cn.check(n, c, r, False, f"radius6 r={radius}")
        if deg == 5:
            assert np.array_equal(np.abs(n[0]), np.float32([0, 0, 1])) and not n[1:].any()


@pytest.mark.parametrize("radius", [0.05, 0.08])
def test_radius_on_a_cloud(ctx, radius):
    """0.05 cuts every neighbourhood of the ring short (down to 2 members: degenerate); at 0.08 a third of them, and the search of
    the others ends on the k-th neighbour; the uniform outliers are left alone either way"""
    r = cn.ref(cn.points("ring"), 30, max_radius=radius)
    assert (r.members < 30).any() and r.degenerate[4000:].any() and not r.degenerate.all() and not cn.excluded(r).any()
    assert (r.members == 30).any() == (radius == 0.08) and (r.members[:4000].min() < 3) == (radius == 0.05)
    n, c = _run(ctx, "ring", 30, max_radius=radius)
    assert ctx.last_normals_degenerate == int(r.degenerate.sum())
    cn.check(n, c, r, False, f"ring k=30 r={radius}")


# ---- orientation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["circle", "centre"])
def test_orientation_towards_the_nearest_viewpoint(ctx, which):
    vp = cn.ring_viewpoints() if which == "circle" else np.zeros((1, 3))
    p = cn.points("ring").astype(np.float64)
    r = cn.ref(p, 30, viewpoints=vp)
    d = vp[None, :, :] - p[:, None, :]
    to = d[np.arange(len(p)), (d * d).sum(axis=-1).argmin(axis=1)]
    assert np.all(np.abs((r.normals * to).sum(axis=1)) > 1e-9 * np.linalg.norm(to, axis=1))       # no reference point on the fence
    n, c = _run(ctx, "ring", 30, viewpoints=vp)
    assert np.all((n.astype(np.float64) * to).sum(axis=1) >= 0)
    cn.check(n, c, r, True, f"ring towards {which}")
    plain, _ = _run(ctx, "ring", 30)
    assert np.array_equal(np.abs(n), np.abs(plain)) and not np.array_equal(n, plain)                 # the sign is all that changes


def test_viewpoint_ties_and_chunks(ctx):
    vp = np.float64([[2, 0, 0], [2, 0, 0], [-2, 0, 0]])
    a, _ = _run(ctx, "ring", 30, viewpoints=vp)
    b, _ = _run(ctx, "ring", 30, viewpoints=vp[[0, 2]])
    assert np.array_equal(a, b)
    # more viewpoints than one staging chunk holds (256), the nearest one in the last, partial chunk
    far = np.tile(np.float64([[50.0, 50.0, 50.0]]), (600, 1)) + np.arange(600)[:, None]
    many = np.concatenate([far, cn.ring_viewpoints()])
    c, _ = _run(ctx, "ring", 30, viewpoints=many)
    d, _ = _run(ctx, "ring", 30, viewpoints=cn.ring_viewpoints())
    assert np.array_equal(c, d)


def test_a_viewpoint_in_the_plane_changes_nothing(ctx):
    plain = _run(ctx, "plane_lattice", 9)
    seen = _run(ctx, "plane_lattice", 9, viewpoints=np.float64([[1.0, 2.0, 0.25]]))
    assert np.array_equal(plain[0], seen[0]) and np.array_equal(plain[1], seen[1])
    above = _run(ctx, "plane_lattice", 9, viewpoints=np.float64([[1.0, 2.0, 3.0]]))[0]
    below = _run(ctx, "plane_lattice", 9, viewpoints=np.float64([[1.0, 2.0, -3.0]]))[0]
    assert np.all(above[:, 2] == 1) and np.all(below[:, 2] == -1)


# ---- invariance ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [30, 33])
def test_the_result_does_not_depend_on_the_cell(ctx, k):
    p = cn.points("k_edges")
    got = [ctx.estimate_normals(p, k, cell_size=c, viewpoints=cn.ring_viewpoints(), curvature=True) for c in cn.CELLS]
    for g in got[1:]:
        assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1])
    cn.check(got[0][0], got[0][1], cn.case_ref("k_edges", k), False, f"k_edges k={k} cell {cn.CELLS[0]}")


def test_repeatable_bit_for_bit(ctx):
    a, b = _run(ctx, "ring", 30), _run(ctx, "ring", 30)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the raw C ABI ---------------------------------------------------------------------------------------------------------------------
def _raw(ctx, xyz, n, k, normals, curvature=None, deg=None, radius=0.0, cell=0.05, vp=None, n_vp=0, h=0):
    return ctx._lib.tl3d_estimate_normals(ctx._h if h == 0 else h, abi.ptr(xyz), n, k, radius, cell, abi.ptr(vp), n_vp, abi.ptr(normals),
                                          abi.ptr(curvature), C.byref(deg) if deg is not None else None)


def test_device_pointers_give_the_host_result(ctx):
    import torch
    dev = torch.device("cuda", 0)
    p, cell, k = cn.points("k_edges"), cn.cell_size("k_edges"), 33
    n = len(p)
    vp = np.ascontiguousarray(cn.ring_viewpoints())
    host_n, host_c = ctx.estimate_normals(p, k, cell_size=cell, viewpoints=vp, curvature=True)
    p_dev = torch.from_numpy(np.array(p)).to(dev)
    for xyz_on_dev in (False, True):
        for out_on_dev in (False, True):
            xyz = p_dev if xyz_on_dev else p
            nrm = torch.full((n, 3), 7.0, dtype=torch.float32, device=dev) if out_on_dev else np.full((n, 3), 7.0, np.float32)
            cur = torch.full((n,), 7.0, dtype=torch.float32, device=dev) if out_on_dev else np.full(n, 7.0, np.float32)
            deg = C.c_int64(-1)
            assert _raw(ctx, xyz, n, k, nrm, cur, deg, cell=cell, vp=vp, n_vp=len(vp)) == abi.OK and deg.value == 0
            assert np.array_equal(nrm.cpu().numpy() if out_on_dev else nrm, host_n), (xyz_on_dev, out_on_dev)
            assert np.array_equal(cur.cpu().numpy() if out_on_dev else cur, host_c), (xyz_on_dev, out_on_dev)
    assert np.array_equal(p_dev.cpu().numpy(), p)                          # the input is read, never written
    out = ctx.estimate_normals(p_dev, k, cell_size=cell, viewpoints=vp, curvature=True)              # the binding: device in, device out
    assert out[0].is_cuda and np.array_equal(out[0].cpu().numpy(), host_n) and np.array_equal(out[1].cpu().numpy(), host_c)


def test_optional_outputs_and_argument_checks(ctx):
    p = np.array(cn.points("tiny_n19"))
    n = len(p)
    want_n, want_c = ctx.estimate_normals(p, 5, cell_size=0.05, curvature=True)
    nrm, cur, deg = np.full((n, 3), 7.0, np.float32), np.full(n, 7.0, np.float32), C.c_int64(-1)
    assert _raw(ctx, p, n, 5, nrm) == abi.OK and np.array_equal(nrm, want_n)                          # no curvature, no count
    assert _raw(ctx, p, n, 5, nrm, cur, deg) == abi.OK and np.array_equal(cur, want_c) and deg.value == 0
    for k in (3, 64):                                                      # the accepted bounds
        assert _raw(ctx, p, n, k, nrm, cur, deg) == abi.OK
    deg.value = -1
    assert _raw(ctx, p, 0, 5, nrm, cur, deg) == abi.OK and deg.value == 0  # n == 0
    assert len(ctx.estimate_normals(np.zeros((0, 3), np.float32))) == 0
    nrm[:], cur[:], deg.value = 7.0, 7.0, -1
    vp = np.float64([[0, 0, 1], [0, 1, 0]])
    bad_vp = [np.float64([[0, 0, 1], [0, v, 0]]) for v in (np.nan, np.inf, -np.inf)]
    both = np.full((n, 4), 7.0, np.float32)                                # one buffer for two outputs
    refused = [
        _raw(ctx, p, n, 5, nrm, cur, deg, h=None), _raw(ctx, None, n, 5, nrm, cur, deg), _raw(ctx, p, n, 5, None, cur, deg),
        _raw(ctx, p, -1, 5, nrm, cur, deg), _raw(ctx, p, 2 ** 31, 5, nrm, cur, deg),
        _raw(ctx, p, n, 2, nrm, cur, deg), _raw(ctx, p, n, 65, nrm, cur, deg), _raw(ctx, p, n, -1, nrm, cur, deg),
        _raw(ctx, p, n, 5, nrm, cur, deg, cell=0.0), _raw(ctx, p, n, 5, nrm, cur, deg, cell=-0.1),
        _raw(ctx, p, n, 5, nrm, cur, deg, vp=vp, n_vp=-1), _raw(ctx, p, n, 5, nrm, cur, deg, vp=None, n_vp=2),
        *[_raw(ctx, p, n, 5, nrm, cur, deg, vp=b, n_vp=2) for b in bad_vp],
        _raw(ctx, p, n, 5, p, cur, deg), _raw(ctx, p, n, 5, nrm, p, deg), _raw(ctx, p, n, 5, both, both, deg),
    ]
    assert refused == [abi.E_INVALID] * len(refused), refused
    for bad in (np.nan, np.inf):                                           # from the device pass in front of the search
        q = p.copy()
        q[7, 1] = bad
        assert _raw(ctx, q, n, 5, nrm, cur, deg) == abi.E_INVALID
    assert np.all(nrm == 7.0) and np.all(cur == 7.0) and np.all(both == 7.0) and deg.value == -1       # a refused call writes nothing
    assert np.array_equal(p, cn.points("tiny_n19"))
    with pytest.raises(abi.Tl3dError):
        ctx.estimate_normals(p, 2)
