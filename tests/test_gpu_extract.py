"""GPU: point extraction (tl3d_extract: extract_count_kernel, scan_kernel, extract_write_kernel) on the crafted grids of
tests/extract_common.py against the numpy restatement of tests/extract_reference.py -- count, order, positions and colours, bit for
bit against its `contract` form (and the C oracle where it applies), within the derived bound against its `exact` form
(tests/test_extract_reference_cpu.py has the bound and the conditions the grids meet).

Measured on the MI355X, GPU against the exact form: grid A 0 of 344 k coordinates over the sweep, grid B 0 of 55 k (the GPU
is bit-equal to the oracle, whose share on the CPU over 3.5 M coordinates of grid L is 4.5e-6, none further than 1 ulp)."""
import ctypes as C

import numpy as np
import pytest

import extract_common as ec
import extract_reference as er
import tl3d
from oracle import c_oracle
from tl3d import _cabi as abi

pytestmark = pytest.mark.gpu
BOTH = tl3d.CH_TSDF | tl3d.CH_CENTROID


def _ctx(g, channels=BOTH, pool_tsdf=0, pool_centroid=0):
    spec = tl3d.GridSpec(g["dims"], g["origin"], g["voxel"], 4 * g["voxel"], channels, pool_tsdf=pool_tsdf, pool_centroid=pool_centroid,
                         voxel_offset=g["voxel_offset"])
    return tl3d.FusionContext(n_slots=1, grid=spec, **ec.CAM)


def _upload(ctx, g, channels=BOTH):
    if channels & tl3d.CH_TSDF:
        ctx.upload_grid(tl3d.CH_TSDF, g["tsdf"])
    if channels & tl3d.CH_CENTROID:
        ctx.upload_grid(tl3d.CH_CENTROID, g["centroid"])


# ---- A: dense, a partial last chunk ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx_a():
    with _ctx(ec.grid("A")) as ctx:
        _upload(ctx, ec.grid("A"))
        yield ctx


@pytest.fixture(scope="module")
def oracle_a():
    g = ec.grid("A")
    orc = c_oracle.Oracle(ec.CAM["width"], ec.CAM["height"], ec.CAM["fx"], ec.CAM["fy"], ec.CAM["cx"], ec.CAM["cy"], dims=g["dims"],
                          origin=g["origin"], voxel_size=g["voxel"], sdf_trunc=4 * g["voxel"])
    orc.tsdf, orc.centroid = g["tsdf"], g["centroid"]
    return orc


@pytest.mark.parametrize("params", ec.SWEEP, ids=ec.sweep_id)
def test_crafted_grid_A_equals_both_references(ctx_a, oracle_a, params):
    got = ctx_a.extract(*params)
    assert len(got[0]) > 1000
    ec.assert_bit_equal(got, ec.swept("A", params, "contract"), "contract")
    ec.assert_bit_equal(got, oracle_a.extract(*params), "oracle")
    ec.assert_within_exact_bound(got, ec.swept("A", params, "exact"), f"A {ec.sweep_id(params)}")


def test_crafted_grid_A_with_one_channel():
    g = ec.grid("A")
    with _ctx(g, tl3d.CH_CENTROID) as ctx:                               # no TSDF channel: the gate is ignored
        _upload(ctx, g, tl3d.CH_CENTROID)
        for mc in ec.MIN_COUNTS:
            got = ctx.extract(tl3d.EXTRACT_CENTROID, mc, ec.MW, ec.HALF_GATE)
            ec.assert_bit_equal(got, ec.reference(g, 0, mc, ec.MW, ec.HALF_GATE, tsdf_channel=False), f"centroid only, count {mc}")
            assert len(got[0]) > len(ec.swept("A", (0, mc, ec.MW, ec.HALF_GATE), "contract")[0])
        with pytest.raises(tl3d.Tl3dError) as e:
            ctx.extract(tl3d.EXTRACT_TSDF)
        assert e.value.code == abi.E_STATE
    with _ctx(g, tl3d.CH_TSDF) as ctx:                                   # no centroid channel: crossings are grey
        _upload(ctx, g, tl3d.CH_TSDF)
        for mw in ec.MIN_WEIGHTS:
            got = ctx.extract(tl3d.EXTRACT_TSDF, 1, mw)
            ec.assert_bit_equal(got, ec.reference(g, 1, 1, mw, use_centroid=False), f"TSDF only, weight {mw}")
            assert (got[1] == 128).all() and np.array_equal(got[0], ec.swept("A", (1, 1, mw, 1.0), "contract")[0])
        with pytest.raises(tl3d.Tl3dError) as e:
            ctx.extract(tl3d.EXTRACT_CENTROID)
        assert e.value.code == abi.E_STATE


# ---- S: bricks with records in both channels, in one, in none -------------------------------------------------------------------
def test_crafted_grid_S_sparse_equals_dense_equals_reference():
    g = ec.grid("S")
    nt = int(g["tsdf"].reshape(-1, 512 * 2).any(axis=1).sum())
    nc = int(g["centroid"].reshape(-1, 512 * 4).any(axis=1).sum())
    assert 0 < nt < 64 and 0 < nc < 64
    with _ctx(g) as dense, _ctx(g, pool_tsdf=nt + 2, pool_centroid=nc + 2) as sparse:
        for ctx in (dense, sparse):
            _upload(ctx, g)
        st = sparse.stats()
        assert st["pool_refused"] == 0 and st["pool_slots_tsdf"] == nt and st["pool_slots_centroid"] == nc
        for params in ec.SWEEP:
            want = ec.reference(g, *params)
            assert len(want[0]) > 1000
            a, b = sparse.extract(*params), dense.extract(*params)
            ec.assert_bit_equal(a, b, f"sparse against dense {params}")
            ec.assert_bit_equal(a, want, f"sparse against the reference {params}")
        assert sparse.stats()["pool_refused"] == 0
        assert np.array_equal(sparse.download_grid(tl3d.CH_TSDF), g["tsdf"])
        assert np.array_equal(sparse.download_grid(tl3d.CH_CENTROID), g["centroid"])


# ---- B: a block with an offset and a core -------------------------------------------------------------------------------------
def test_crafted_grid_B_offset_and_core():
    g = ec.grid("B")
    lattice = [o + d for o, d in zip(g["voxel_offset"], g["dims"])]
    with _ctx(g) as ctx:
        _upload(ctx, g)
        for params in [(0, 1, 0, 1.0), (0, 2, ec.MW, ec.HALF_GATE), (1, 1, 0, 1.0), (1, 1, ec.MW, 1.0)]:
            whole = ctx.extract(*params)
            ec.assert_bit_equal(whole, ec.reference(g, *params, core=None), f"no core {params}")
            ctx.set_block_core(lattice, *g["core"])
            got = ctx.extract(*params)
            assert 1000 < len(got[0]) < len(whole[0])
            ec.assert_bit_equal(got, ec.reference(g, *params), f"core {params}")
            ec.assert_within_exact_bound(got, ec.reference(g, *params, form="exact"), f"B {ec.sweep_id(params)}")
            ctx.set_block_core()
            ec.assert_bit_equal(ctx.extract(*params), whole, f"core cleared {params}")


# ---- L: one chunk more than the single-block scan has threads ---------------------------------------------------------------------
def test_crafted_grid_L_scan_edge():
    g = ec.grid("L")
    xyz, rgb, d = ec.reference(g, 1, use_centroid=False, details=True)
    chunk = d["record"] // 2048
    assert len(g["tsdf"]) == 1024 * 2048 + 512 and chunk.max() == 1024 and (chunk == 1023).any() and (chunk == 1024).any()
    assert (np.bincount(chunk, minlength=1025) > 0).all()
    with _ctx(g, tl3d.CH_TSDF) as ctx:
        _upload(ctx, g, tl3d.CH_TSDF)
        ec.assert_bit_equal(ctx.extract(tl3d.EXTRACT_TSDF), (xyz, rgb), "L")
        ec.assert_bit_equal(ctx.extract(tl3d.EXTRACT_TSDF, 1, ec.MW), ec.reference(g, 1, 1, ec.MW, use_centroid=False), "L, weight 2")


# ---- pending free-space counts on crafted records -------------------------------------------------------------------------------
def test_crafted_records_with_pending_free_space():
    g = ec.grid("P")
    depth = np.full((ec.CAM["height"], ec.CAM["width"]), 3.0, np.float32)          # a wall 3 m away: the whole grid is free space
    pose = (np.eye(3), np.zeros(3))
    after = dict(sum=g["vol"]["sum"] + 32767, weight=g["vol"]["weight"] + 1)
    assert after["weight"].max() == abi.TSDF_MAX_WEIGHT and after["sum"].max() == 32767 * abi.TSDF_MAX_WEIGHT
    with _ctx(g, tl3d.CH_TSDF) as ctx:
        _upload(ctx, g, tl3d.CH_TSDF)
        ctx.upload(0, depth, None)
        ctx.integrate(0, pose)
        got = ctx.extract(tl3d.EXTRACT_TSDF)                                       # at once: nothing has read the channel yet
        want = ec.reference(g, 1, vol=after, use_centroid=False)
        assert len(want[0]) > 500 and len(want[0]) != len(ec.reference(g, 1, use_centroid=False)[0])
        ec.assert_bit_equal(got, want, "pending")
        ec.assert_bit_equal(ctx.extract(tl3d.EXTRACT_TSDF, 1, ec.MW), ec.reference(g, 1, 1, ec.MW, vol=after, use_centroid=False), "folded")
        assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), er.records_from_volumes(after)[0])
        assert np.array_equal(ctx.download_grid(tl3d.CH_TSDF), g["tsdf"] + np.array([32767, 1], np.int32))


# ---- size query and capacity ------------------------------------------------------------------------------------------------------
def _raw(ctx, params, xyz, rgb, cap):
    n = C.c_int64(-1)
    rc = ctx._lib.tl3d_extract(ctx._h, int(params[0]), int(params[1]), int(params[2]), float(params[3]), abi.ptr(xyz), abi.ptr(rgb),
                               int(cap), C.byref(n))
    return rc, n.value


@pytest.mark.parametrize("params", [(0, 2, ec.MW, ec.HALF_GATE), (1, 1, 0, 1.0)], ids=ec.sweep_id)
def test_size_query_and_capacity(ctx_a, params):
    want = ec.swept("A", params, "contract")
    n = len(want[0])
    ctx_a.set_block_core()                                               # a fresh count: no earlier call's result is reused
    xyz, rgb = np.full((n, 3), -7.0, np.float32), np.full((n, 3), 0xAB, np.uint8)
    assert _raw(ctx_a, params, xyz[:n - 1], rgb[:n - 1], n - 1) == (abi.E_CAPACITY, n)
    assert (xyz == -7.0).all() and (rgb == 0xAB).all()                   # both buffers untouched
    assert _raw(ctx_a, params, None, None, 0) == (abi.OK, n)             # the size query
    assert _raw(ctx_a, params, xyz[:n - 1], rgb[:n - 1], n - 1) == (abi.E_CAPACITY, n)    # ... and after it
    assert (xyz == -7.0).all() and (rgb == 0xAB).all()
    assert _raw(ctx_a, params, xyz, rgb, n) == (abi.OK, n)
    ec.assert_bit_equal((xyz, rgb), want, "cap = n")
