"""GPU: planar regions of a cloud with normals (tl3d_segment_planes, kernels_planes.hip) against the numpy /
scipy formulations of tests/plane_segments_reference.py (held to each other and to known answers in
tests/test_plane_segments_reference_cpu.py): plane_id, the four counts and every plane's count and seed exactly, on the box corner,
at every decision edge one f32 ulp apart, on the union-find topologies and under every invariance; the plane parameters within the
bar derived in tests/plane_segments_common.py; then capacity and refusals on the raw C ABI."""
import ctypes as C

import numpy as np
import pytest

import plane_segments_common as pc
import plane_segments_reference as pr
import tl3d
from tl3d import _cabi as abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with tl3d.FusionContext(8, 8, 1.0, 1.0, 0.0, 0.0, n_slots=1) as c:
        yield c


def _params(prm, reserved=0):
    return abi.PlaneParams(radius=prm.radius, min_cos=prm.min_cos, max_offset=prm.max_offset, max_curvature=prm.max_curvature,
                           max_rms=prm.max_rms, min_points=prm.min_points, signed_normals=1 if prm.signed_normals else 0, reserved=reserved)


def _raw(ctx, xyz, nrm, curv, n, prm, plane_id, planes, cap, counts, cell=None, h=0):
    if not isinstance(prm, (abi.PlaneParams, type(None))):
        prm = _params(prm)
    cell = (prm.radius if prm is not None else 1.0) if cell is None else cell
    return ctx._lib.tl3d_segment_planes(ctx._h if h == 0 else h, abi.ptr(xyz), abi.ptr(nrm), abi.ptr(curv), n,
                                        C.byref(prm) if prm is not None else None, cell, abi.ptr(plane_id), abi.ptr(planes), cap, counts)


def _run(ctx, p, n, c, prm, cell=None):
    """(plane_id, planes, counts) through the C ABI with the exact parameters of `prm` (the binding takes an angle)"""
    m = len(p)
    cap = m // prm.min_points
    plane_id, planes, counts = np.full(m, -7, np.int32), np.zeros(max(cap, 1), abi.PLANE_DTYPE), (C.c_int64 * 4)(-1, -1, -1, -1)
    rc = _raw(ctx, np.ascontiguousarray(p), np.ascontiguousarray(n), None if c is None else np.ascontiguousarray(c), m, prm, plane_id,
              planes, cap, counts, cell=cell)
    assert rc == abi.OK, ctx._lib.tl3d_last_error()
    return plane_id, planes[:counts[3]], tuple(counts)


def _same(got, res, what):
    plane_id, planes, counts = got
    assert counts == res.counts, f"{what}: counts {counts}, reference {res.counts}"
    assert np.array_equal(plane_id, res.plane_id), f"{what}: {int((plane_id != res.plane_id).sum())} plane ids differ"
    assert np.array_equal(planes["count"], res.planes["count"]) and np.array_equal(planes["seed"], res.planes["seed"]), what


# ---- box corner ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise_mm", [0.0, 1.0])
def test_box_corner(ctx, noise_mm):
    res = pc.box_reference(noise_mm)
    assert res.counts[2:] == (5, 4)                              # on the reference first: three faces and the step; the cylinder is
    a, b = pc.BOX_PARTS["cylinder"]                              # one candidate region that max_rms rejects
    assert np.all(res.plane_id[a:b] == -1) and len(np.unique(res.label[a:b])) == 1 and res.label[a] >= 0
    p, n, c = pc.box_corner(noise_mm)
    got = _run(ctx, p, n, c, pc.BOX_PARAMS)
    _same(got, res, f"box corner, noise {noise_mm} mm")
    pc.check_planes(got[1], res, p, f"box corner, noise {noise_mm} mm")
    # the binding, with the angle in degrees
    plane_id, planes, counts = ctx.segment_planes(p, n, c, radius=pc.BOX_PARAMS.radius, max_angle_deg=10.0, max_offset=pc.BOX_PARAMS.max_offset,
                                                  max_curvature=0.05, min_points=pc.BOX_PARAMS.min_points, max_rms=pc.BOX_PARAMS.max_rms)
    assert counts == dict(zip(("eligible", "regions", "candidates", "planes"), res.counts)) and plane_id.dtype == np.int32
    assert np.array_equal(plane_id, got[0]) and planes.tobytes() == got[1].tobytes() and planes.dtype == abi.PLANE_DTYPE


# ---- decision edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.EDGES)
def test_decision_edges(ctx, name):
    p, n, c, prm, want = pc.EDGE_CASES[name]
    res = pr.segment_tree(p, n, c, prm)
    assert res.counts == want                                    # on the reference first
    got = _run(ctx, p, n, c, prm)
    _same(got, res, name)
    pc.check_planes(got[1], res, p, name)


# ---- signed / unsigned ---------------------------------------------------------------------------------------------------------------
def test_signed_and_unsigned_normals(ctx):
    p, n = pc.two_sheets()
    for signed, planes in ((True, 2), (False, 1)):
        prm = pc.SHEET_PARAMS.replace(signed_normals=signed)
        res = pr.segment_tree(p, n, None, prm)
        assert res.counts == (780, planes, planes, planes)
        got = _run(ctx, p, n, None, prm)
        _same(got, res, f"two sheets, signed {signed}")
        pc.check_planes(got[1], res, p, f"two sheets, signed {signed}")
        # the sign follows the sum of the members' normals: +z for the lower sheet and for both together (400 against 380), -z above
        assert [float(np.sign(z)) for z in got[1]["normal"][:, 2]] == ([1.0, -1.0] if signed else [1.0])


# ---- union-find topologies -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.TOPOLOGIES)
def test_union_find_topologies(ctx, name):
    p, n = pc.topology(name)
    want_id, want_counts, want_planes = pc.topology_answer(name)
    plane_id, planes, counts = _run(ctx, p, n, None, pc.TOPO_PARAMS)
    assert counts == want_counts
    assert np.array_equal(plane_id, want_id)
    assert list(zip(planes["count"].tolist(), planes["seed"].tolist())) == want_planes
    if name.startswith("strip"):                                 # (the other two: by reasoning, see topology_answer)
        _same((plane_id, planes, counts), pr.segment_tree(p, n, None, pc.TOPO_PARAMS), name)


# ---- invariances ---------------------------------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_the_cell(ctx):
    p, n, c = pc.box_corner(1.0)
    r = pc.BOX_PARAMS.radius
    base = _run(ctx, p, n, c, pc.BOX_PARAMS)
    _same(base, pc.box_reference(1.0), "cell = radius")
    for cell in (r / 4, 3 * r, 100 * r):
        got = _run(ctx, p, n, c, pc.BOX_PARAMS, cell=cell)
        assert np.array_equal(got[0], base[0]) and got[1].tobytes() == base[1].tobytes() and got[2] == base[2], cell
    # a box that forces the cell to double: two far points (not eligible: zero normals) stretch it to 4000 m per axis
    far = np.float32([[-2000, -2000, -2000], [2000, 2000, 2000]])
    p2, n2, c2 = np.concatenate([p, far]), np.concatenate([n, np.zeros((2, 3), np.float32)]), np.concatenate([c, np.zeros(2, np.float32)])
    assert (4000 / (r / 4)) ** 3 > 2 ** 27
    got = _run(ctx, p2, n2, c2, pc.BOX_PARAMS, cell=r / 4)
    assert np.array_equal(got[0][:-2], base[0]) and np.all(got[0][-2:] == -1) and got[1].tobytes() == base[1].tobytes() and got[2] == base[2]


def test_repeatable_and_host_or_device_pointers(ctx):
    import torch
    dev = torch.device("cuda", 0)
    p, n, c = pc.box_corner(1.0)
    m, cap = len(p), len(p) // pc.BOX_PARAMS.min_points
    a, b = _run(ctx, p, n, c, pc.BOX_PARAMS), _run(ctx, p, n, c, pc.BOX_PARAMS)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    pd, nd, cd = (torch.from_numpy(np.array(x)).to(dev) for x in (p, n, c))
    for in_dev in (False, True):
        for out_dev in (False, True):
            ids = torch.full((m,), -7, dtype=torch.int32, device=dev) if out_dev else np.full(m, -7, np.int32)
            planes = torch.zeros((cap, 10), dtype=torch.float64, device=dev) if out_dev else np.zeros(cap, abi.PLANE_DTYPE)
            counts = (C.c_int64 * 4)()
            ins = (pd, nd, cd) if in_dev else (p, n, c)
            assert _raw(ctx, *ins, m, pc.BOX_PARAMS, ids, planes, cap, counts) == abi.OK
            got_ids = ids.cpu().numpy() if out_dev else ids
            got_planes = planes.cpu().numpy().view(abi.PLANE_DTYPE).reshape(-1) if out_dev else planes
            assert np.array_equal(got_ids, a[0]) and got_planes[:counts[3]].tobytes() == a[1].tobytes() and tuple(counts) == a[2], (in_dev, out_dev)
    assert np.array_equal(pd.cpu().numpy(), p) and np.array_equal(nd.cpu().numpy(), n)          # the inputs are read, never written
    ids, planes, counts = ctx.segment_planes(pd, nd, cd, radius=pc.BOX_PARAMS.radius, max_offset=pc.BOX_PARAMS.max_offset, max_curvature=0.05,
                                             min_points=pc.BOX_PARAMS.min_points, max_rms=pc.BOX_PARAMS.max_rms)
    assert ids.is_cuda and np.array_equal(ids.cpu().numpy(), a[0]) and planes.tobytes() == a[1].tobytes()


def test_a_permuted_input_gives_the_same_partition(ctx):
    p, n, c = pc.box_corner(1.0)
    base = _run(ctx, p, n, c, pc.BOX_PARAMS)
    perm = np.random.default_rng(3).permutation(len(p))        # new index k holds old point perm[k]
    got = _run(ctx, p[perm], n[perm], c[perm], pc.BOX_PARAMS)
    assert got[2] == base[2]
    inv = np.argsort(perm)
    # a plane's new seed is the smallest new index of its members; its number follows the new seeds
    old_of_new, seeds = {}, []
    for k in range(len(base[1])):
        members_new = inv[np.flatnonzero(base[0] == k)]
        seeds.append(int(members_new.min()))
    for new_k, old_k in enumerate(np.argsort(seeds)):
        old_of_new[new_k] = int(old_k)
        assert int(got[1]["seed"][new_k]) == seeds[old_k] and got[1]["count"][new_k] == base[1]["count"][old_k]
    mapped = np.array([old_of_new.get(int(k), -1) for k in got[0]], np.int32)
    assert np.array_equal(mapped, base[0][perm])
    _same(got, pr.segment_tree(p[perm], n[perm], c[perm], pc.BOX_PARAMS), "permuted box corner")


# ---- capacity and refusals -----------------------------------------------------------------------------------------------------------
def test_capacity_one_short(ctx):
    p, n, c = (np.array(x) for x in pc.box_corner(0.0))
    m = len(p)
    want = _run(ctx, p, n, c, pc.BOX_PARAMS)
    for cap in (3, 0):
        ids, planes, counts = np.full(m, -7, np.int32), np.full(4 * 10, 7.0), (C.c_int64 * 4)(-1, -1, -1, -1)
        rc = _raw(ctx, p, n, c, m, pc.BOX_PARAMS, ids, planes if cap else None, cap, counts)
        assert rc == abi.E_CAPACITY and tuple(counts) == want[2] and counts[3] == 4
        assert np.array_equal(ids, want[0]) and np.all(planes == 7.0)              # plane_id written, no record
    ids, planes, counts = np.full(m, -7, np.int32), np.zeros(4, abi.PLANE_DTYPE), (C.c_int64 * 4)()
    assert _raw(ctx, p, n, c, m, pc.BOX_PARAMS, ids, planes, 4, counts) == abi.OK and planes.tobytes() == want[1].tobytes()
    with pytest.raises(abi.Tl3dError):
        ctx.segment_planes(p, n, radius=-1.0)


def test_refusals_write_nothing(ctx):
    p, n, c = (np.array(x) for x in pc.box_corner(0.0))
    m, cap, good = len(p), 55, pc.BOX_PARAMS
    ids, planes, counts = np.full(m, -7, np.int32), np.full(cap * 10, 7.0), (C.c_int64 * 4)(-1, -1, -1, -1)
    call = lambda **kw: _raw(ctx, **{**dict(xyz=p, nrm=n, curv=c, n=m, prm=good, plane_id=ids, planes=planes, cap=cap, counts=counts), **kw})
    assert call(n=0) == abi.OK and tuple(counts) == (0, 0, 0, 0) and np.all(ids == -7)                  # n == 0
    counts[:] = [-1, -1, -1, -1]
    both = np.full(m * 4, 7.0, np.float32)                                 # one buffer for an input and an output
    bad_params = [good.replace(radius=r) for r in (0.0, -1.0, np.nan, np.inf)] + [good.replace(min_cos=v) for v in (-0.01, 1.01, np.nan)] + \
                 [good.replace(max_offset=v) for v in (-1e-9, np.nan)] + [good.replace(min_points=v) for v in (2, 0, -5)]
    refused = [call(h=None), call(xyz=None), call(nrm=None), call(prm=None), call(plane_id=None), call(counts=None), call(n=-1), call(n=2 ** 31),
               call(planes=None), call(cap=-1), call(cell=0.0), call(cell=np.nan),
               *[call(prm=b) for b in bad_params], call(prm=_params(good, reserved=1)),
               call(plane_id=p.view(np.int32)), call(plane_id=n.view(np.int32)), call(plane_id=c.view(np.int32)),
               call(planes=p, cap=m * 12 // 80), call(plane_id=both.view(np.int32), planes=both, cap=m * 16 // 80)]
    assert refused == [abi.E_INVALID] * len(refused), refused

    def untouched():
        return bool(np.all(ids == -7) and np.all(planes == 7.0) and tuple(counts) == (-1, -1, -1, -1) and np.all(both == 7.0)
                    and np.array_equal(p, pc.box_corner(0.0)[0]) and np.array_equal(n, pc.box_corner(0.0)[1]) and np.array_equal(c, pc.box_corner(0.0)[2]))
    assert untouched()                                                     # every refusal in front of the device work
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 22, -(2.0 ** 22)):         # from the device pass in front of the index
        for row, axis in ((7, 1), (m - 1, 2)):
            q = p.copy()
            q[row, axis] = bad
            assert call(xyz=q) == abi.E_INVALID, bad
            assert untouched(), bad
    # the largest coordinate that is taken, into buffers of its own
    q = p.copy()
    q[7, 1] = np.nextafter(np.float32(2.0 ** 22), np.float32(0))
    ids2, planes2, counts2 = np.full(m, -7, np.int32), np.full(cap * 10, 7.0), (C.c_int64 * 4)(-1, -1, -1, -1)
    assert call(xyz=q, plane_id=ids2, planes=planes2, counts=counts2) == abi.OK and counts2[3] == 4 and not np.any(ids2 == -7)
    assert untouched()


def test_a_box_too_wide_for_the_64_bit_sums_is_refused(ctx):
    """sum e is kept in 64 bits: n * (extent * 2^20 + 1) must stay below 2^62 (tl3d.h).  2^20 points over 2^22 m are refused by the
    host check behind the bounds pass, with nothing written; the same points over 2^21 m are taken"""
    m = 1 << 20
    w = np.zeros((m, 3), np.float32)
    w[:, 1] = np.arange(m)                                                  # a row 1 m apart: further than the radius, nothing links
    w[0, 0], w[1, 0] = -(2.0 ** 21), 2.0 ** 21
    nrm = np.zeros((m, 3), np.float32)
    nrm[:, 2] = 1.0
    ids, planes, counts = np.full(m, -7, np.int32), np.full(10 * (m // 3), 7.0), (C.c_int64 * 4)(-1, -1, -1, -1)
    prm = pr.Params(radius=0.5, min_cos=0.5, max_offset=0.125, min_points=3)
    assert m * (2.0 ** 22 * 2.0 ** 20 + 1) >= 2.0 ** 62
    assert _raw(ctx, w, nrm, None, m, prm, ids, planes, m // 3, counts) == abi.E_INVALID
    assert np.all(ids == -7) and np.all(planes == 7.0) and tuple(counts) == (-1, -1, -1, -1)
    w[0, 0], w[1, 0] = -(2.0 ** 20), 2.0 ** 20
    assert _raw(ctx, w, nrm, None, m, prm, ids, planes, m // 3, counts) == abi.OK
    assert tuple(counts) == (m, m, 0, 0) and np.all(ids == -1)               # every point a region of its own
