"""GPU: voxel-centroid accumulation (kernels_centroid.hip: centroid_points_kernel, centroid_frame_kernel, centroid_direct_kernel,
centroid_mark_kernel, bounds_kernel) on the crafted clouds and frames of tests/centroid_accumulate_common.py against its integer
model, bit for bit: records, the accepted / dropped counts, the slots a sparse grid hands out and the brick count of
tl3d_count_bricks.  tests/test_centroid_accumulate_reference_cpu.py pins the model and the conditions the inputs meet.

The frames' expected points come from the C oracle's back-projection (pinned to the reference's golden data), voxels and sums from
the model: nothing the library computes enters its own expectation."""
import functools

import numpy as np
import pytest
import torch

import centroid_accumulate_common as cc
import extract_reference as er
import tl3d
from oracle import c_oracle

pytestmark = pytest.mark.gpu
CH = tl3d.CH_CENTROID
LAYOUTS = ("dense", "sparse")
IDENTITY = (np.eye(3), np.zeros(3))


def _ctx(geo, pool=0, offset=(0, 0, 0), cam="64x48", n_slots=1):
    spec = tl3d.GridSpec(geo["dims"], geo["origin"], geo["voxel"], 4 * geo["voxel"], CH, pool_centroid=pool, voxel_offset=offset)
    return tl3d.FusionContext(n_slots=n_slots, grid=spec, min_depth=cc.MIN_DEPTH, max_depth=cc.MAX_DEPTH, **cc.CAMS[cam])


def _check(ctx, rec, n_core, n_rest, touched, sparse, what):
    got = ctx.download_grid(CH)
    st = ctx.stats()
    bad = np.flatnonzero((got != rec).any(axis=1))
    assert len(bad) == 0, (what, len(bad), "records differ; the first:", int(bad[0]), got[bad[0]].tolist(), rec[bad[0]].tolist())
    assert np.array_equal(got, rec), what
    assert (st["centroid_points"], st["centroid_dropped"]) == (n_core, n_rest), (what, st["centroid_points"], st["centroid_dropped"])
    assert st["pool_refused"] == 0, what
    if sparse and ctx.grid.pool_centroid < ctx.grid.nvox // 512:        # (a pool of every brick is a dense channel: every brick has a slot)
        assert st["pool_slots_centroid"] == touched, (what, st["pool_slots_centroid"], touched)
    return got


def _device(xyz, rgb):
    return torch.from_numpy(np.array(xyz)).cuda(), torch.from_numpy(np.array(rgb)).cuda()        # (copies: the lists are read-only)


# ---- point lists --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", cc.LIST_NAMES)
def test_crafted_list_equals_the_model(name, layout):
    c = cc.crafted_list(name)
    rec, n_core, n_dropped, touched = cc.list_model(name)
    sparse = layout == "sparse"
    images = []
    for order in ("forward", "reversed"):
        xyz, rgb = (c["xyz"], c["rgb"]) if order == "forward" else (c["xyz"][::-1].copy(), c["rgb"][::-1].copy())
        for where in ("host", "device"):
            with _ctx(c["geo"], pool=touched if sparse else 0) as ctx:
                ctx.accumulate_points(*(_device(xyz, rgb) if where == "device" else (xyz, rgb)))
                images.append(_check(ctx, rec, n_core, n_dropped, touched, sparse, f"{name} {layout} {order} {where}"))
    assert all(np.array_equal(images[0], im) for im in images[1:])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_voxel_holds_two_to_the_twenty_points(layout):
    sparse = layout == "sparse"
    a, b = cc.limit_points(0), cc.limit_points(1, 1 << 16)
    va, vb = cc.model_volumes(*a, **cc.GEO)[0], cc.model_volumes(*b, **cc.GEO)[0]
    vol = cc.add_volumes(va, vb, times=(1, 16))
    rec = cc.records_from_volumes(vol)
    top = cc.N_LIMIT * (cc.FRAC - 1)
    for v in cc.LIMIT_VOXELS:
        assert [int(vol[f][v]) for f in cc.FIELDS] == [cc.N_LIMIT, top, top, top] + [255 * cc.N_LIMIT] * 3
    assert cc.touched_bricks(vol) == 1 and int(rec.any(axis=1).sum()) == 2
    with _ctx(cc.GEO, pool=1 if sparse else 0) as ctx:
        ctx.accumulate_points(*(_device(*a) if sparse else a))          # 2^20 points of one voxel as ONE list
        for _ in range(16):                                              # its neighbour: 16 calls of 2^16
            ctx.accumulate_points(*b)
        _check(ctx, rec, 2 * cc.N_LIMIT, 0, 1, sparse, f"limit {layout}")
        got = ctx.extract(tl3d.EXTRACT_CENTROID)
        want = er.extract(vol, cc.GEO["dims"], cc.GEO["origin"], cc.GEO["voxel"], mode=0, tsdf_channel=False)
        assert len(want[0]) == 2 and (want[1] == 255).all()
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        # (S + n / 2) / (4096 n) with S = 4095 n: half a unit below the voxel's upper corner, on every axis
        for v, p in zip(cc.LIMIT_VOXELS, got[0]):
            assert np.array_equal(p, np.float32([cc.GEO["origin"][k] + (v[k] + 4095.5 / 4096) * cc.GEO["voxel"] for k in range(3)]))


def test_last_record_of_the_largest_grid_beside_lanes_without_a_voxel():
    """record 0xffffffff shares its low half with the key of a lane that has no voxel: its runs must still end where such a lane
    follows.  The grid is far too large to download: its three touched bricks are packed and compared."""
    c = cc.list_last_record()
    geo = c["geo"]
    nb = [d // 8 for d in geo["dims"]]
    _, _, ok = cc.point_voxels(c["xyz"], geo["origin"], geo["voxel"], (0, 0, 0), geo["dims"])
    bricks = [(0, 0, 0), (3, 2, 4), (nb[0] - 1, nb[1] - 1, nb[2] - 1)]   # the fillers' two and the last
    ids = [(b[2] * nb[1] + b[1]) * nb[0] + b[0] for b in bricks]
    assert ids[-1] == nb[0] * nb[1] * nb[2] - 1 == (1 << 23) - 1
    want = [cc.brick_model(c, b) for b in bricks]
    assert sum(n for _, n in want) == int(ok.sum()) and all(n > 0 for _, n in want)
    for where in ("host", "device"):
        with _ctx(geo, pool=3) as ctx:
            ctx.accumulate_points(*(_device(c["xyz"], c["rgb"]) if where == "device" else (c["xyz"], c["rgb"])))
            rows = torch.full((3, 2048), -1, dtype=torch.int64, device="cuda")
            idt = torch.tensor(ids, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.pack_bricks(CH, idt, rows)
            ctx.sync()
            got = rows.cpu().numpy().view(np.uint64).reshape(3, 512, 4)
            st = ctx.stats()
            for g, (w, _), b in zip(got, want, bricks):
                assert np.array_equal(g, w), (where, b, g[g.any(axis=1)].tolist(), w[w.any(axis=1)].tolist())
            assert (st["centroid_points"], st["centroid_dropped"]) == (int(ok.sum()), int((~ok).sum()))
            assert st["pool_refused"] == 0 and st["pool_slots_centroid"] == 3


@pytest.mark.parametrize("name", cc.DYADIC_GEO_LISTS)
def test_block_with_offset_and_core_equals_the_lattice_slice(name):
    c = cc.crafted_list(name)
    block, lattice = cc.block_geometry(c["geo"])
    off, dims = cc.BLOCK_OFFSET, c["geo"]["dims"]
    whole, _, _ = cc.model_volumes(c["xyz"], c["rgb"], lattice, block["origin"], block["voxel"])        # the single lattice
    cut = {f: whole[f][off[0]:off[0] + dims[0], off[1]:off[1] + dims[1], off[2]:off[2] + dims[2]] for f in cc.FIELDS}
    rec = cc.records_from_volumes(cut)
    n_in = int(cut["n"].sum())
    touched = cc.touched_bricks(cut)
    core = cc.core_of(c["geo"])
    n_core = int(cut["n"][tuple(slice(lo, hi) for lo, hi in zip(*core))].sum())
    assert 0 < n_core < n_in and cc.model_accumulate(c["xyz"], c["rgb"], offset=off, core=core, **block)[1] == n_core
    n = len(c["xyz"])
    with _ctx(block, offset=off) as ctx:
        ctx.accumulate_points(c["xyz"], c["rgb"])
        _check(ctx, rec, n_in, n - n_in, touched, False, f"{name} offset")
    with _ctx(block, pool=touched, offset=off) as ctx:
        ctx.set_block_core(lattice, *core)
        ctx.accumulate_points(*_device(c["xyz"], c["rgb"]))
        _check(ctx, rec, n_core, n - n_core, touched, True, f"{name} offset and core")       # the halo is accumulated all the same


# ---- frames -------------------------------------------------------------------------------------------------------------------------
GRIDS = dict(fine=cc.GRID_FINE, coarse=cc.GRID_COARSE)


def _oracle(cam):
    k = cc.CAMS[cam]
    return c_oracle.Oracle(k["width"], k["height"], k["fx"], k["fy"], k["cx"], k["cy"], min_depth=cc.MIN_DEPTH, max_depth=cc.MAX_DEPTH)


@functools.lru_cache(maxsize=None)
def _frame_models(cam, stride, grid):
    """[(volumes, n_accepted, n_dropped)] of the crafted frames of a camera, one by one: oracle points, model sums"""
    out = []
    for _, depth, bgr in cc.crafted_frames(cc.CAMS[cam]):
        xyz, rgb = _oracle(cam).backproject(depth, bgr, subsample=stride, min_depth=cc.MIN_DEPTH, max_depth=cc.MAX_DEPTH)
        out.append(cc.model_volumes(xyz, rgb, **GRIDS[grid]))
    return out


def _run_frames(cam, grid, layout, plan):
    """plan: [(frame, stride)] accumulated in that order without anything in between; the grid must hold the sum of the models"""
    frames = cc.crafted_frames(cc.CAMS[cam])
    parts = [_frame_models(cam, s, grid)[f] for f, s in plan]
    vol = cc.add_volumes(*[p[0] for p in parts])
    rec, touched = cc.records_from_volumes(vol), cc.touched_bricks(vol)
    sparse = layout == "sparse"
    with _ctx(GRIDS[grid], pool=max(touched, 1) if sparse else 0, cam=cam, n_slots=len(frames)) as ctx:
        for i, (_, depth, bgr) in enumerate(frames):
            ctx.upload(i, depth, bgr)
        for f, s in plan:
            ctx.accumulate_centroid(f, None, subsample=s)
        _check(ctx, rec, sum(p[1] for p in parts), sum(p[2] for p in parts), touched, sparse, f"{cam} {grid} {layout} {plan[:4]}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("stride", cc.STRIDES)
@pytest.mark.parametrize("cam", list(cc.CAMS))
def test_crafted_frames_equal_the_model(cam, stride, layout):
    for grid in GRIDS:
        for f in range(3):                                               # each frame alone ...
            _run_frames(cam, grid, layout, [(f, stride)])
        _run_frames(cam, grid, layout, [(f, stride) for f in range(3)])  # ... and the three in one launch


@pytest.mark.parametrize("stride", cc.STRIDES)
@pytest.mark.parametrize("cam", list(cc.CAMS))
def test_count_bricks_is_exact_on_the_crafted_frames(cam, stride):
    frames = cc.crafted_frames(cc.CAMS[cam])
    for grid, geo in GRIDS.items():
        spec = tl3d.GridSpec(geo["dims"], geo["origin"], geo["voxel"], 4 * geo["voxel"], CH)
        with _ctx(geo, cam=cam, n_slots=len(frames)) as ctx:
            for i, (_, depth, bgr) in enumerate(frames):
                ctx.upload(i, depth, bgr)
            models = _frame_models(cam, stride, grid)
            for pick in ([0], [1], [2], [0, 1, 2]):
                want = cc.touched_bricks(cc.add_volumes(*[models[f][0] for f in pick]))
                got = ctx.count_bricks(spec, pick, [IDENTITY] * len(pick), centroid_subsample=stride)
                assert got == (0, want), (cam, stride, grid, pick, got, want)
            assert not ctx.download_grid(CH).any()                       # counting touches no record


@pytest.mark.parametrize("stride", (2, 3))                               # the table kernel and the direct kernel
@pytest.mark.parametrize("n", cc.BATCHES)
def test_batches_of_one_stride_equal_the_sum_of_the_frames(n, stride):
    assert cc.BATCHES == (1, 15, 16, 17, 32, 33)                         # descriptor chunks of 16, launches of 32
    _run_frames("64x48", "fine", "sparse" if n % 2 else "dense", [(i % 3, stride) for i in range(n)])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_change_of_stride_cuts_the_batch(layout):
    assert cc.STRIDE_SEQUENCE == (1, 1, 2, 2, 1, 3, 3)
    _run_frames("64x48", "fine", layout, [(i % 3, s) for i, s in enumerate(cc.STRIDE_SEQUENCE)])
    _run_frames("61x47", "fine", layout, [((i + 1) % 3, s) for i, s in enumerate(cc.STRIDE_SEQUENCE)])


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
def test_points_bounds_on_the_crafted_lists():
    with _ctx(cc.GRID_COARSE) as ctx:
        for name, xyz in cc.bounds_lists():
            want = cc.bounds_reference(xyz)
            for where in ("host", "device"):
                got = ctx.points_bounds(torch.from_numpy(xyz).cuda() if where == "device" else xyz)
                print(name, where, got[0].tolist(), got[1].tolist(), "sign bits", np.signbit(got[0]).tolist(), np.signbit(got[1]).tolist())
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, where, got, want)
