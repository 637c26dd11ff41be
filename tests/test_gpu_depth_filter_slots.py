"""GPU: tl3d_filter_depth_slots leaves nothing stale behind.  A slot's frame feeds a normal map, an averaged depth, the TSDF tile
cache and the classification cache; the filter rewrites the frame, so each of them must be rebuilt from the filtered image: after
fuse -> normals -> filter -> reset -> fuse, the grids equal, bit for bit, those of a fresh context that uploaded the frames as the
numpy reference filters them.  And a filter issued while a registration still reads the slot waits for it."""
import numpy as np
import pytest

import depth_filter_common as dc
import depth_filter_reference as dr
import tl3d
from tl3d import synth
from helpers import TINY

pytestmark = pytest.mark.gpu

N = 3
PRM = dc.prm(min_region=30)
SPEC = dict(dims=(32, 32, 32), origin=(-0.16, -0.16, -0.16), voxel=0.01, trunc=0.04)


def box3(d):
    """3 x 3 box blur, zero beyond the border: every silhouette becomes a ramp of pixels that lie on no surface"""
    p = np.pad(d.astype(np.float64), 1)
    h, w = d.shape
    return (sum(p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0).astype(np.float32)


@pytest.fixture(scope="module")
def frames():
    """{kind: (poses, [(depth, colour)], [(reference-filtered depth, counts)])}, computed once"""
    scene = synth.Scene(spheres=[((0.0, 0.0, 0.0), 0.10), ((0.07, 0.03, 0.0), 0.06)])
    poses = synth.orbit_poses(N, 0.5, 15.0)
    out = {}
    for kind in ("f32", "u16"):
        fr = []
        for p in poses:
            d, c = synth.render(scene, p, **TINY)
            d = box3(d)
            if kind == "u16":
                d = np.rint(d * 1000.0).astype(np.uint16)
            fr.append((d, c))
        ref = [dr.filter_shifted(d, **PRM) for d, _c in fr]
        assert all(r[1][1] > 20 for r in ref), [r[1] for r in ref]           # the ramps are there, and they go
        out[kind] = (poses, fr, ref)
    return out


def context(n_slots=N):
    spec = tl3d.GridSpec(SPEC["dims"], SPEC["origin"], SPEC["voxel"], SPEC["trunc"])
    return tl3d.FusionContext(TINY["width"], TINY["height"], TINY["fx"], TINY["fy"], TINY["cx"], TINY["cy"], n_slots=n_slots, grid=spec)


def fused(ctx, poses):
    ctx.fuse_frames(list(range(N)), poses, centroid_subsample=1)
    return ctx.download_grid(tl3d.CH_TSDF), ctx.download_grid(tl3d.CH_CENTROID)


@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_refusion_after_the_filter_equals_a_fresh_context(frames, kind):
    poses, fr, ref = frames[kind]
    with context() as fresh:
        for i, (f, _cnt) in enumerate(ref):
            fresh.upload(i, np.array(f), fr[i][1])
        want_tsdf, want_cen = fused(fresh, poses)
        fresh.build_normals_many(list(range(N)))
        want_normals = [fresh.download_normals(i) for i in range(N)]
        want_depth = [fresh.download_depth(i) for i in range(N)]
    with context() as ctx:
        for i, (d, c) in enumerate(fr):
            ctx.upload(i, d, c)
        raw_tsdf, _raw_cen = fused(ctx, poses)                               # builds the tile and class caches
        assert not np.array_equal(raw_tsdf, want_tsdf)                       # (the filter matters to the grid)
        ctx.build_normals_many(list(range(N)))
        raw_normals = ctx.download_normals(1)
        counts = ctx.filter_depth_slots(list(range(N)), **PRM)
        assert counts.tolist() == [r[1].tolist() for r in ref]
        ctx.reset()
        tsdf, cen = fused(ctx, poses)
        assert np.array_equal(tsdf, want_tsdf) and np.array_equal(cen, want_cen)
        for i in range(N):
            assert np.array_equal(ctx.download_depth(i).view(np.uint32), want_depth[i].view(np.uint32)), i
        # the old normal maps are void: a registration on them is refused until they are rebuilt, and the rebuilt ones are the fresh context's
        with pytest.raises(tl3d.Tl3dError):
            ctx.icp(0, 1, iters=2, stride=2, max_dist=0.1)
        ctx.build_normals_many(list(range(N)))
        for i in range(N):
            assert np.array_equal(ctx.download_normals(i).view(np.uint32), want_normals[i].view(np.uint32)), i
        assert not np.array_equal(raw_normals.view(np.uint32), want_normals[1].view(np.uint32))
        # once more through the warm caches: fuse on top, then a second filter (nothing left to remove but what the reference says)
        again = [dr.filter_shifted(np.array(r[0]), **PRM) for r in ref]
        counts = ctx.filter_depth_slots(list(range(N)), **PRM)
        assert counts.tolist() == [a[1].tolist() for a in again]


@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_filter_waits_for_an_uncollected_registration(frames, kind):
    poses, fr, ref = frames[kind]
    kw = dict(iters=6, stride=1, max_dist=0.1)
    with context() as ctx:
        for i, (d, c) in enumerate(fr):
            ctx.upload(i, d, c)
        ctx.build_normals(1)
        undisturbed = ctx.icp(0, 1, **kw)
        ctx.icp_enqueue(2, 0, 1, **kw)
        ctx.filter_depth_slots([0, 1], counts=False, **PRM)                  # rewrites the depth and voids the normal map the run reads
        got = ctx.icp_collect(2)
        assert np.array_equal(got["T"], undisturbed["T"]) and got["n_corr"] == undisturbed["n_corr"] and got["iters_run"] == undisturbed["iters_run"]
        assert undisturbed["n_corr"] > 100
        ctx.upload(2, np.array(ref[0][0]))
        assert np.array_equal(ctx.download_depth(0).view(np.uint32), ctx.download_depth(2).view(np.uint32))
