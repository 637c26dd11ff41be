"""GPU: the device weld of the blocks' keyed meshes (tl3d_mesh_weld_keyed, FusionContext.weld_meshes)
against the crafted cases of tests/mesh_weld_common.py, whose welded mesh is known by construction, and against the host weld
(lattice.weld_meshes), byte for byte; its refusals with their counts; a real blocked mesh; the pipeline with mesh_weld="device"."""
import numpy as np
import pytest

import mesh_weld_common as mw
import tl3d
from helpers import SMALL, small_scene_frames
from tl3d import _cabi as abi
from tl3d import pipeline as pl
from tl3d.config import ReconstructionConfig
from tl3d.fusion import GridSpec
from tl3d.pipeline import DepthToReconstructionPipeline

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with tl3d.FusionContext(SMALL["width"], SMALL["height"], SMALL["fx"], SMALL["fy"], SMALL["cx"], SMALL["cy"], n_slots=8, grid=None) as c:
        yield c


def _to_device(parts):
    import torch
    out = []
    for x, r, t, k, lo, hi in parts:
        out.append((torch.from_numpy(x).cuda(), None if r is None else torch.from_numpy(r).cuda(),
                    torch.from_numpy(np.ascontiguousarray(t).view(np.int32)).cuda(), torch.from_numpy(k).cuda(), lo, hi))
    return out


def _to_host(mesh):
    x, r, t, k = mesh
    if hasattr(t, "data_ptr"):
        assert x.is_cuda and t.is_cuda and k.is_cuda
        x, r, t, k = x.cpu().numpy(), None if r is None else r.cpu().numpy(), t.cpu().numpy().view(np.uint32), k.cpu().numpy()
    return x, r, t, k


@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("name", mw.CASES)
def test_device_weld_gives_the_constructed_bytes(ctx, name, kind):
    L, parts, want, _info = mw.case(name)
    given = _to_device(parts) if kind == "device" else parts
    first = _to_host(ctx.weld_meshes(given, L))
    again = _to_host(ctx.weld_meshes(given, L))
    assert mw.same_bytes(first, want) and mw.same_bytes(again, want)
    assert mw.same_bytes(first, pl.weld_meshes(parts, L))


def test_wrapped_chains_report_no_vertex_twice_and_no_corner_unowned(ctx):
    """the key table at its smallest capacity, half full, every claim and every lookup wrapping round the end of the array: the call's
    own counts (the bytes are in the test above)"""
    L, parts, want, _info = mw.case("wrap")
    rc, msg, counts, outs = mw.raw_call(ctx._h, parts, L)
    assert rc == abi.OK, msg
    assert counts == [mw.WRAP_KEPT, len(want[2]), 0, 0]
    assert mw.same_bytes((outs[0][:counts[0]], outs[1][:counts[0]], outs[3], outs[2][:counts[0]]), want)


def test_variants(ctx):
    L, parts, want, _info = mw.case("soup_small")
    # without rgb
    x, r, t, k = ctx.weld_meshes([p[:1] + (None,) + p[2:] for p in parts], L)
    assert r is None and mw.same_bytes((x, want[1], t, k), want)
    # out_key_hd = NULL
    rc, msg, counts, outs = mw.raw_call(ctx._h, parts, L, outs=(np.empty((len(want[0]), 3), np.float32), np.empty((len(want[0]), 3), np.uint8), None,
                                                               np.empty((len(want[2]), 3), np.uint32)),
                                        vert_cap=len(want[0]), tri_cap=len(want[2]))       # (and capacities that fit exactly)
    assert rc == abi.OK and counts == [len(want[0]), len(want[2]), 0, 0]
    assert mw.same_bytes((outs[0], outs[1], outs[3], want[3]), want)
    # nothing to weld
    assert mw.same_bytes(ctx.weld_meshes([], L), pl.weld_meshes([], L))
    rc, msg, counts, _ = mw.raw_call(ctx._h, [], L)
    assert rc == abi.OK and counts == [0, 0, 0, 0]
    L2, seam, seam_want = mw.seam_case()
    no_vertex = [(p[0][:0], p[1][:0], p[2][:0], p[3][:0], p[4], p[5]) for p in seam]
    assert mw.same_bytes(ctx.weld_meshes(no_vertex, L2), pl.weld_meshes(no_vertex, L2))
    # empty cores: a part that owns nothing and names nothing changes nothing; with every core empty every vertex goes
    xa, ra, ta, ka = seam[0][:4]
    extra = (xa + 7, ra, ta[:0], ka, (3, 3, 3), (3, 8, 8))
    assert mw.same_bytes(ctx.weld_meshes(seam + [extra], L2), seam_want)
    gone = [(p[0], p[1], p[2][:0], p[3], (5, 5, 5), (5, 5, 5)) for p in seam]
    got = ctx.weld_meshes(gone, L2)
    assert [len(a) for a in got] == [0, 0, 0, 0] and mw.same_bytes(got, pl.weld_meshes(gone, L2))
    # cores that leave a gap: B's third vertex (owner voxel x = 12) lies in it and, named by no triangle, vanishes silently
    xb, rb, tb, kb = seam[1][:4]
    gap = [seam[0], (xb, rb, np.array([[0, 1, 1]], np.uint32), kb, (8, 0, 0), (10, 8, 8))]
    want_gap = (np.concatenate([xa[[0, 2, 3]], xb[:2]]), np.concatenate([ra[[0, 2, 3]], rb[:2]]), np.array([[0, 3, 1], [3, 4, 4]], np.uint32),
                np.concatenate([ka[[0, 2, 3]], kb[:2]]))
    got = ctx.weld_meshes(gap, L2)
    assert mw.same_bytes(got, want_gap) and mw.same_bytes(got, pl.weld_meshes(gap, L2))


def _with_copies(part, rows):
    x, r, t, k, lo, hi = part
    return np.concatenate([x, x[rows]]), np.concatenate([r, r[rows]]), t, np.concatenate([k, k[rows]]), lo, hi


def test_refusals_store_their_counts(ctx):
    L, parts, want, info = mw.case("soup_small")
    kept, ntri = len(want[0]), len(want[2])
    own0 = np.flatnonzero(mw.owner_part(parts[0][3], L, [parts[0][4:]]) == 0)
    # a kept vertex listed again in its part: one vertex twice more, one once more
    rc, msg, counts, _ = mw.raw_call(ctx._h, [_with_copies(parts[0], own0[[3, 3, 9]])] + parts[1:], L)
    assert rc == abi.E_INVALID and "a vertex is owned by two block cores" in msg and counts == [kept + 3, ntri, 3, 0]
    # ... and in a second part with the same core
    x, r, t, k, lo, hi = parts[0]
    rows = own0[:5]
    rc, msg, counts, _ = mw.raw_call(ctx._h, parts + [(x[rows], r[rows], t[:0], k[rows], lo, hi)], L)
    assert rc == abi.E_INVALID and "a vertex is owned by two block cores" in msg and counts == [kept + 5, ntri, 5, 0]
    with pytest.raises(abi.Tl3dError, match="owned by two block cores") as e:
        ctx.weld_meshes(parts + [(x[rows], r[rows], t[:0], k[rows], lo, hi)], L)
    assert e.value.code == abi.E_INVALID
    # the last part removed: the corners of the others that its core owns
    last = len(parts) - 1
    unowned = sum(int((o == last).sum()) for o in info["corner_owner"][:last])
    assert unowned >= 100
    rc, msg, counts, _ = mw.raw_call(ctx._h, parts[:last], L)
    n_last = int((info["part"][info["order"]] == last).sum())
    assert rc == abi.E_INVALID and "a triangle references a vertex no block core owns" in msg
    assert counts == [kept - n_last, ntri - len(parts[last][2]), 0, unowned]
    with pytest.raises(abi.Tl3dError, match="no block core owns"):
        ctx.weld_meshes(parts[:last], L)
    # an index >= its part's n_vert (below the next part's end: only the part's own size refuses it)
    t_bad = parts[2][2].copy()
    t_bad[7, 1] = len(parts[2][0])
    rc, msg, counts, _ = mw.raw_call(ctx._h, parts[:2] + [parts[2][:2] + (t_bad,) + parts[2][3:]] + parts[3:], L)
    assert rc == abi.E_INVALID and "1 triangle indices out of range" in msg and f"{len(parts[2][0])} in part 2" in msg
    assert counts == [0, 0, 0, 0]
    # keys out of range: 3 * nvox, and a negative one
    nvox = L[0] * L[1] * L[2]
    for bad in (3 * nvox, -1, np.iinfo(np.int64).min):
        k_bad = parts[1][3].copy()
        k_bad[len(k_bad) // 2] = bad
        rc, msg, counts, _ = mw.raw_call(ctx._h, parts[:1] + [parts[1][:3] + (k_bad,) + parts[1][4:]] + parts[2:], L)
        assert rc == abi.E_INVALID and "1 keys outside" in msg and counts == [0, 0, 0, 0], (bad, msg)
    k_top = parts[1][3].copy()                                               # the largest key there is, on a halo copy: no key refusal
    assert 3 * nvox - 1 not in set(want[3].tolist())
    k_top[int(np.flatnonzero(mw.owner_part(k_top, L, [parts[1][4:]]) != 0)[0])] = 3 * nvox - 1
    rc, msg, counts, _ = mw.raw_call(ctx._h, parts[:1] + [parts[1][:3] + (k_top,) + parts[1][4:]] + parts[2:], L)
    assert "keys outside" not in msg and counts[:2] == [kept, ntri]
    # short capacities
    rc, msg, counts, _ = mw.raw_call(ctx._h, parts, L, vert_cap=kept - 1)
    assert rc == abi.E_CAPACITY and counts == [kept, ntri, 0, 0]
    rc, msg, counts, _ = mw.raw_call(ctx._h, parts, L, tri_cap=ntri - 1)
    assert rc == abi.E_CAPACITY and counts == [kept, ntri, 0, 0]
    rc, msg, counts, outs = mw.raw_call(ctx._h, parts, L, vert_cap=kept, tri_cap=ntri)
    assert rc == abi.OK and counts == [kept, ntri, 0, 0]
    assert mw.same_bytes((outs[0][:kept], outs[1][:kept], outs[3][:ntri], outs[2][:kept]), want)


# ---- a real mesh: the 256^3 lattice, frames and 8 blocks of tests/test_gpu_blocks.py ------------------------------------------------

LATTICE = GridSpec((256, 256, 256), (-1.28, -1.28, -1.28), 0.01, 0.04)


@pytest.mark.parametrize("sparse", [False, True])
def test_real_blocked_mesh_welds_to_the_host_welds_bytes(ctx, sparse):
    poses, frames = small_scene_frames(n=8, deg=12.0, radius=1.0)
    index = list(range(len(poses)))
    for i, (d, c) in enumerate(frames):
        ctx.upload(i, d, c)
    parts = []
    blocks = pl.plan_blocks(LATTICE, 136 ** 3)
    for b in blocks:
        g = b.grid
        if sparse:
            t, c = ctx.count_bricks(g, index, poses, centroid_subsample=1)
            g = GridSpec(g.dims, g.origin, g.voxel_size, g.sdf_trunc, g.channels, pool_tsdf=t + 64, pool_centroid=c + 64, voxel_offset=g.voxel_offset)
        assert g.sparse == sparse
        ctx.attach_grid(g)
        ctx.set_block_core(LATTICE.dims, b.lo, b.hi)
        ctx.fuse_frames(index, poses, centroid_subsample=1)
        off = np.asarray(g.voxel_offset)
        parts.append(tuple(ctx.extract_mesh(keys=True)) + (off + np.asarray(b.lo), off + np.asarray(b.hi)))
        ctx.detach_grid()
    want = pl.weld_meshes(parts, LATTICE.dims)
    assert len(blocks) >= 2 and len(want[2]) > 5000 and sum(len(p[0]) for p in parts) > len(want[0])
    assert mw.same_bytes(ctx.weld_meshes(parts, LATTICE.dims), want)
    assert mw.same_bytes(_to_host(ctx.weld_meshes(_to_device(parts), LATTICE.dims)), want)


# ---- the pipeline: the forced-blocks run of tests/test_gpu_mesh_smooth.py ----------------------------------------------------------

def _lattice_run(kw, frames, poses, limit):
    old = pl.MAX_BLOCK_VOXELS
    try:
        if limit is not None:
            pl.MAX_BLOCK_VOXELS = limit
        pipe = DepthToReconstructionPipeline(ReconstructionConfig(**kw))
        pipe.set_frames([c for d, c in frames], [d for d, c in frames])
        pipe.reconstruct(poses=poses)
    finally:
        pl.MAX_BLOCK_VOXELS = old
    return pipe


def test_pipeline_device_weld_gives_the_host_welds_mesh():
    poses, frames = small_scene_frames(n=3)
    cam = {k: SMALL[k] for k in ("fx", "fy", "cx", "cy")}
    base = dict(**cam, voxel_size=0.02, subsample_factor=1, grid_dim=128, outlier_filter=False, extract_mesh=True)
    one = _lattice_run(dict(base, mesh_weld="device"), frames, poses, None)                  # one block: nothing to weld, no stats
    assert one.stats["blocks"] == 1 and "mesh_weld" not in one.stats and "mesh_weld_s" not in one.timings
    limit = one.grid.nvox // 3
    for opts in (dict(), dict(mesh_min_component_triangles=20, mesh_simplify_cell=0.04, mesh_smooth_iterations=2, mesh_normals=True)):
        host = _lattice_run(dict(base, **opts), frames, poses, limit)
        dev = _lattice_run(dict(base, mesh_weld="device", **opts), frames, poses, limit)
        assert host.stats["blocks"] >= 2 and dev.stats["blocks"] == host.stats["blocks"] and len(host.mesh[2]) > 1000
        for a, b, dtype in zip(dev.mesh, host.mesh, (np.float32, np.uint8, np.uint32)):
            assert a.dtype == b.dtype == dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        if opts:
            assert dev.mesh_normals.tobytes() == host.mesh_normals.tobytes()
        assert "mesh_weld" not in host.stats and "mesh_weld_s" not in host.timings
        assert dev.stats["mesh_weld"]["parts"] == dev.stats["blocks"] and "mesh_weld_s" in dev.timings
        assert dev.stats["mesh_weld"]["vertices_in"] > dev.stats["mesh_weld"]["vertices"] > 0
        assert set(dev.stats) - {"mesh_weld"} == set(host.stats) and set(dev.timings) - {"mesh_weld_s"} == set(host.timings)

