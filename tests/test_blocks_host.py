"""CPU: the host side of blocked fusion -- plan_blocks (disjoint cores that tile the lattice, halos on the + sides that have a
neighbour, blocks within the voxel limit), the keyed mesh weld, and the layout helpers keeping a block's voxel_offset."""
import numpy as np
import pytest

from tl3d import _cabi as abi
from tl3d import pipeline as pl
from tl3d.fusion import GridSpec


def _lattice(extent, voxel=0.005):
    mn = np.zeros(3)
    return pl.plan_lattice(mn, np.asarray(extent, np.float64), voxel, 512)


def _check_tiling(lat, blocks, limit):
    L = np.asarray(lat.dims, np.int64)
    cover = 0
    boxes = []
    for b in blocks:
        off = np.asarray(b.grid.voxel_offset, np.int64)
        lo, hi = np.asarray(b.lo), np.asarray(b.hi)
        dims = np.asarray(b.grid.dims, np.int64)
        assert tuple(lo) == (0, 0, 0)
        assert np.all(off % 8 == 0) and np.all(dims % 8 == 0) and np.all(hi % 8 == 0)
        assert b.grid.nvox <= limit
        assert b.grid.origin == lat.origin and b.grid.voxel_size == lat.voxel_size and b.grid.channels == lat.channels
        end = off + hi
        assert np.all(end <= L)
        # halo: one brick on the + sides with a next block, none elsewhere
        for a in range(3):
            assert dims[a] == hi[a] + (8 if end[a] < L[a] else 0)
        cover += int(np.prod(hi))
        boxes.append((off, end))
    assert cover == int(np.prod(L))                    # cores hold the lattice's voxel count ...
    for i in range(len(boxes)):                        # ... and are pairwise disjoint: they tile it
        for j in range(i + 1, len(boxes)):
            (a0, a1), (b0, b1) = boxes[i], boxes[j]
            assert np.any(np.minimum(a1, b1) <= np.maximum(a0, b0)), (boxes[i], boxes[j])


def test_plan_blocks_tiles_a_lattice_beyond_2_32():
    lat = _lattice((60.0, 26.0, 3.0))
    assert lat.nvox > 2 ** 32
    blocks = pl.plan_blocks(lat)
    assert len(blocks) >= 4
    _check_tiling(lat, blocks, pl.MAX_BLOCK_VOXELS)


@pytest.mark.parametrize("limit", [1 << 20, 3 * (1 << 18) + 4096, 136 ** 3])
def test_plan_blocks_respects_lower_limits(limit):
    lat = GridSpec((256, 200, 96), (0.0, 0.0, 0.0), 0.01, 0.04)
    blocks = pl.plan_blocks(lat, limit)
    assert len(blocks) > 1
    _check_tiling(lat, blocks, limit)


def test_plan_blocks_of_a_lattice_within_the_limit_is_plan_grid():
    mn, mx = np.array([-1.0, -1.2, -0.5]), np.array([1.0, 1.2, 12.0])
    grid, clipped = pl.plan_grid(mn, mx, 0.005, 1024)
    assert not clipped
    lat = pl.plan_lattice(mn, mx, 0.005, 1024)
    assert lat == grid
    blocks = pl.plan_blocks(lat)
    assert len(blocks) == 1
    b = blocks[0]
    assert b.grid is lat and b.grid.voxel_offset == (0, 0, 0) and b.lo == (0, 0, 0) and b.hi == tuple(grid.dims)
    assert b.grid.dims == grid.dims and b.grid.origin == grid.origin


def test_plan_lattice_is_never_shaved():
    mn, mx = np.array([-1.0, -1.2, -0.5]), np.array([1.0, 1.2, 120.0])
    grid, clipped = pl.plan_grid(mn, mx, 0.005, 512)
    assert clipped                                     # plan_grid itself still shaves (its contract is unchanged)
    lat = pl.plan_lattice(mn, mx, 0.005, 512)
    assert lat.nvox > 2 ** 32 and lat.dims[2] * 0.005 >= 120.5 - 1e-9
    assert np.allclose(lat.origin, mn - 0.0025)


def test_split_block_halves_the_core_with_halos():
    lat = GridSpec((256, 128, 64), (0.0, 0.0, 0.0), 0.01, 0.04)
    whole = pl._make_block(lat, (0, 0, 0), lat.dims)
    a, b = pl.split_block(lat, whole)
    assert a.grid.voxel_offset == (0, 0, 0) and a.hi == (128, 128, 64) and a.grid.dims == (136, 128, 64)
    assert b.grid.voxel_offset == (128, 0, 0) and b.hi == (128, 128, 64) and b.grid.dims == (128, 128, 64)


def _key(i, j, k, axis, L):
    return 3 * ((k * L[1] + j) * L[0] + i) + axis


def test_weld_joins_seam_vertices_and_keeps_unreferenced_ones():
    L = (16, 8, 8)
    # block A: core x in [0, 8), halo x = 8..15; block B: core x in [8, 16)
    ka = np.array([_key(7, 0, 0, 0, L), _key(8, 0, 0, 1, L), _key(7, 1, 0, 1, L), _key(3, 3, 3, 2, L), _key(9, 2, 2, 0, L)], np.int64)
    xa = np.arange(15, dtype=np.float32).reshape(5, 3)
    ra = np.arange(15, dtype=np.uint8).reshape(5, 3)
    ta = np.array([[0, 1, 2]], np.uint32)             # references the halo-owned vertex 1 (owned by B's core)
    kb = np.array([_key(8, 0, 0, 1, L), _key(9, 2, 2, 0, L), _key(12, 4, 4, 2, L)], np.int64)
    xb = np.array([[3, 4, 5], [12, 13, 14], [100, 100, 100]], np.float32)
    rb = np.array([[3, 4, 5], [12, 13, 14], [9, 9, 9]], np.uint8)
    tb = np.array([[0, 1, 2]], np.uint32)
    parts = [(xa, ra, ta, ka, (0, 0, 0), (8, 8, 8)), (xb, rb, tb, kb, (8, 0, 0), (16, 8, 8))]
    xyz, rgb, tris, keys = pl.weld_meshes(parts, L)
    # A keeps its three core-owned vertices (one of them unreferenced), B its three
    assert len(xyz) == 6 and len(np.unique(keys)) == 6
    assert sorted(keys.tolist()) == sorted([ka[0], ka[2], ka[3], kb[0], kb[1], kb[2]])
    tk = keys[tris.astype(np.int64)]
    assert tk.tolist() == [[ka[0], ka[1], ka[2]], [kb[0], kb[1], kb[2]]]
    for v in range(len(xyz)):                         # every kept vertex carries its own block's position and colour
        src = {int(k): (x, r) for k, x, r in zip(list(ka) + list(kb), list(xa) + list(xb), list(ra) + list(rb))}
        x, r = src[int(keys[v])]
        if int(keys[v]) in (int(ka[1]),):
            continue
        assert np.array_equal(xyz[v], x) and np.array_equal(rgb[v], r)


def test_weld_keeps_coincident_vertices_with_different_keys_apart():
    L = (16, 8, 8)
    # a voxel centre with t = 0 exactly: the x- and y-edge vertices of one owner sit at the same position, different keys
    k = np.array([_key(7, 3, 3, 0, L), _key(7, 3, 3, 1, L), _key(6, 3, 3, 2, L)], np.int64)
    x = np.array([[1, 1, 1], [1, 1, 1], [2, 2, 2]], np.float32)
    r = np.zeros((3, 3), np.uint8)
    t = np.array([[0, 1, 2]], np.uint32)
    xyz, _rgb, tris, keys = pl.weld_meshes([(x, r, t, k, (0, 0, 0), (8, 8, 8)), (x[:0], r[:0], t[:0], k[:0], (8, 0, 0), (16, 8, 8))], L)
    assert len(xyz) == 3 and len(set(tris[0].tolist())) == 3


def test_weld_refuses_a_reference_no_core_owns():
    L = (16, 8, 8)
    k = np.array([_key(7, 0, 0, 0, L), _key(9, 0, 0, 0, L), _key(6, 0, 0, 0, L)], np.int64)
    x = np.zeros((3, 3), np.float32)
    r = np.zeros((3, 3), np.uint8)
    t = np.array([[0, 1, 2]], np.uint32)
    with pytest.raises(ValueError):
        pl.weld_meshes([(x, r, t, k, (0, 0, 0), (8, 8, 8))], L)


def test_layout_helpers_keep_the_voxel_offset():
    g = GridSpec((512, 512, 4096), (0.0, 0.0, 0.0), 0.005, 0.02, voxel_offset=(0, 0, 8192))
    out = pl.layout_from_counts(g, 1000, 500)
    assert out.voxel_offset == (0, 0, 8192) and out.sparse

    class _Ctx:
        def count_bricks(self, grid, *a, **k):
            assert grid.voxel_offset == (0, 0, 8192)
            return 1000, 500
    out = pl.choose_layout(_Ctx(), g, [0], [(np.eye(3), np.zeros(3))], [1.0], 2, log=lambda *a: None)
    assert out.voxel_offset == (0, 0, 8192)
    small = GridSpec((64, 64, 64), (0.0, 0.0, 0.0), 0.005, 0.02, voxel_offset=(64, 0, 8))
    assert pl.choose_layout(None, small, [], [], [], 2).voxel_offset == (64, 0, 8)


def test_binding_declares_the_block_entry_points():
    for name in ("tl3d_detach_grid", "tl3d_set_block_core", "tl3d_extract_mesh_keyed"):
        assert name in abi.SYMBOLS


# ---- the tiler, against what it gave before the two copies of the halving rule became one ------------------------------

# (core offset, core dims, grid dims = core + halo) in plan_blocks' order
_BLOCKS_60_26_3 = [
    ((0, 0, 0), (1504, 2608, 608), (1512, 2616, 608)), ((1504, 0, 0), (1504, 2608, 608), (1512, 2616, 608)),
    ((3008, 0, 0), (1504, 2608, 608), (1512, 2616, 608)), ((4512, 0, 0), (1496, 2608, 608), (1504, 2616, 608)),
    ((6008, 0, 0), (1504, 2608, 608), (1512, 2616, 608)), ((7512, 0, 0), (1496, 2608, 608), (1504, 2616, 608)),
    ((9008, 0, 0), (1504, 2608, 608), (1512, 2616, 608)), ((10512, 0, 0), (1496, 2608, 608), (1496, 2616, 608)),
    ((0, 2608, 0), (1504, 2600, 608), (1512, 2600, 608)), ((1504, 2608, 0), (1504, 2600, 608), (1512, 2600, 608)),
    ((3008, 2608, 0), (1504, 2600, 608), (1512, 2600, 608)), ((4512, 2608, 0), (1496, 2600, 608), (1504, 2600, 608)),
    ((6008, 2608, 0), (1504, 2600, 608), (1512, 2600, 608)), ((7512, 2608, 0), (1496, 2600, 608), (1504, 2600, 608)),
    ((9008, 2608, 0), (1504, 2600, 608), (1512, 2600, 608)), ((10512, 2608, 0), (1496, 2600, 608), (1496, 2600, 608))]
_BLOCKS_256_200_96_EIGHT = [
    ((0, 0, 0), (64, 104, 96), (72, 112, 96)), ((64, 0, 0), (64, 104, 96), (72, 112, 96)),
    ((128, 0, 0), (64, 104, 96), (72, 112, 96)), ((192, 0, 0), (64, 104, 96), (64, 112, 96)),
    ((0, 104, 0), (64, 96, 96), (72, 96, 96)), ((64, 104, 0), (64, 96, 96), (72, 96, 96)),
    ((128, 104, 0), (64, 96, 96), (72, 96, 96)), ((192, 104, 0), (64, 96, 96), (64, 96, 96))]
_BLOCKS_256_200_96 = {
    1 << 20: _BLOCKS_256_200_96_EIGHT,
    3 * (1 << 18) + 4096: _BLOCKS_256_200_96_EIGHT,
    136 ** 3: [((0, 0, 0), (128, 104, 96), (136, 112, 96)), ((128, 0, 0), (128, 200, 96), (128, 200, 96)),
               ((0, 104, 0), (128, 96, 96), (136, 96, 96))]}


def _as_rows(blocks):
    return [(tuple(b.grid.voxel_offset), tuple(b.hi), tuple(b.grid.dims)) for b in blocks]


def test_plan_blocks_gives_the_recorded_blocks_in_the_recorded_order():
    lat = _lattice((60.0, 26.0, 3.0))
    assert lat.dims == (12008, 5208, 608)
    assert _as_rows(pl.plan_blocks(lat)) == _BLOCKS_60_26_3
    lat = GridSpec((256, 200, 96), (0.0, 0.0, 0.0), 0.01, 0.04)
    for limit, want in _BLOCKS_256_200_96.items():
        assert _as_rows(pl.plan_blocks(lat, limit)) == want, limit


def test_tile_without_halo_gives_the_recorded_merge_blocks():
    """What DenseReconstructor's merge fuses a 61 m x 26 m x 3 m cloud at 5 mm in: cores of at most 2^31 voxels, no halo."""
    from tl3d.lattice import lattice_extent, tile
    _origin, dims = lattice_extent(np.zeros(3), np.array([61.0, 26.0, 3.0]), 0.005)
    assert tuple(dims) == (12208, 5208, 608)
    want = [((x, y, 0), (dx, dy, 608)) for y, dy in ((0, 1304), (1304, 1304), (2608, 1304), (3912, 1296))
            for x, dx in ((0, 1528), (1528, 1528), (3056, 1528), (4584, 1520), (6104, 1528), (7632, 1528), (9160, 1528), (10688, 1520))]
    got = tile(dims, lambda off, d: d[0] * d[1] * d[2] <= 1 << 31)
    assert [(tuple(o), tuple(d)) for o, d in got] == want


# ---- the fusion body, driven with a stand-in for FusionContext ---------------------------------------------------------

class _RecordingContext:
    """Logs (method, args, kwargs) and answers with tiny arrays.  Every block reports 12 valid samples, 5, 4, 3, ... of them in its
    core, two points, and one triangle on three vertices its own core owns."""
    H, W = 4, 6

    def __init__(self):
        self.log, self.grid, self.core, self.fused = [], None, None, 0

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def call(*a, **k):
            self.log.append((name, a, k))
            answer = type(self).__dict__.get("_" + name)
            return answer(self, *a, **k) if answer else None
        return call

    def names(self):
        return [n for n, _a, _k in self.log]

    def _attach_grid(self, grid):
        self.grid, self.core = grid, None

    def _set_block_core(self, lattice_dims, lo, hi):
        self.core = (lattice_dims, lo, hi)

    def _fuse_frames(self, *a, **k):
        self.fused += 1

    def _stats(self):
        return dict(centroid_points=6 - self.fused, centroid_dropped=6 + self.fused, pool_slots_tsdf=0, pool_slots_centroid=0, pool_refused=0)

    def _extract(self, *a, **k):
        return np.full((2, 3), self.fused, np.float32), np.full((2, 3), self.fused, np.uint8)

    def _extract_mesh(self, min_weight=0, keys=False):
        xyz = np.arange(9, dtype=np.float32).reshape(3, 3) + 100 * self.fused
        mesh = (xyz, np.full((3, 3), self.fused, np.uint8), np.array([[2, 0, 1]], np.uint32))
        if not keys:
            return mesh
        L, off = self.core[0], np.asarray(self.grid.voxel_offset) + np.asarray(self.core[1])
        return mesh + (np.array([_key(*off, axis, L) for axis in range(3)], np.int64),)

    def _statistical_outlier(self, xyz, *a, **k):
        keep = np.ones(len(xyz), bool)
        keep[0] = False
        return keep

    def _raycast(self, pose, **k):
        return np.ones((self.H, self.W), np.float32), None, np.zeros((self.H, self.W, 3), np.uint8)

    def _download_depth(self, slot):
        return np.full((self.H, self.W), 1.5, np.float32)


def _pipe(monkeypatch, **cfg):
    from tl3d.config import ReconstructionConfig
    monkeypatch.setattr(pl, "device_free_bytes", lambda device: 1 << 40)
    pipe = pl.DepthToReconstructionPipeline(ReconstructionConfig(extract_mesh=True, outlier_filter=True, **cfg))
    pipe.frame_index, pipe.scales, pipe.image_names = [0, 1], [1.0, 1.0], ["a.png", "b.png"]
    pipe.camera_poses = [(np.eye(3), np.zeros((3, 1)))] * 2
    return pipe


_LATTICE = GridSpec((256, 200, 96), (0.0, 0.0, 0.0), 0.01, 0.04)
_PER_BLOCK = ["attach_grid", "set_block_core", "reset_stats", "fuse_frames", "stats", "extract", "extract_mesh", "detach_grid"]


def test_fusion_body_one_block_has_no_core_no_keys_and_stays_attached_for_the_ray_caster(monkeypatch, tmp_path, capsys):
    pipe, ctx = _pipe(monkeypatch, render_dir=str(tmp_path)), _RecordingContext()
    blocks = pl.plan_blocks(_LATTICE)
    assert len(blocks) == 1
    xyz, rgb = pipe._fuse_blocks(ctx, _LATTICE, blocks)
    names = ctx.names()
    assert names == ["attach_grid", "reset_stats", "fuse_frames", "stats", "extract", "extract_mesh", "statistical_outlier",
                     "raycast", "download_depth", "raycast", "download_depth"]
    assert "set_block_core" not in names and "detach_grid" not in names[:names.index("raycast")]
    assert [k for n, _a, k in ctx.log if n == "extract_mesh"] == [dict(min_weight=pipe.config.tsdf_min_weight, keys=False)]
    assert len(xyz) == 1 and len(rgb) == 1                                  # the stand-in's filter drops the first of two points
    want = _RecordingContext()
    want.fused = 1
    for got, ref in zip(pipe.mesh, want._extract_mesh()):                   # the mesh as extracted: same vertices, same order
        assert np.array_equal(got, ref)
    assert pipe.stats == dict(points_accumulated=5, points_dropped=7, voxels=2, after_outlier_filter=1, sparse=False, bricks_tsdf=0,
                              bricks_centroid=0, pool_refused=0, blocks=1, mesh_vertices=3, mesh_triangles=1, render_views=2,
                              render_residual_mm=[500.0, 500.0])
    assert sorted(pipe.timings) == ["bound_and_allocate_s", "extract_and_filter_s", "fuse_s", "mesh_s", "render_s"]
    assert pipe.grid == ctx.log[0][1][0] and pipe.blocks == [pipe.grid] and pipe.grid.dims == _LATTICE.dims
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("  Grid (256, 200, 96) @ 10 mm, origin")
    assert out[1:] == ["", "--- Step 3: Fuse depth frames (TSDF + voxel centroids) ---", "Camera 0: fused", "Camera 1: fused", "",
                       "--- Step 4: Extract and clean point cloud ---", "  Mesh: 3 vertices, 1 triangles",
                       f"  Rendered the model at 2 cameras into {tmp_path}", "", "Final reconstruction: 1 points, 2 cameras"]


def test_fusion_body_takes_a_given_layout_as_it_is(monkeypatch):
    pipe, ctx = _pipe(monkeypatch), _RecordingContext()
    grid = GridSpec((1024, 1024, 1024), (0.0, 0.0, 0.0), 0.005, 0.02, pool_tsdf=5000, pool_centroid=4000)     # 40 GiB if dense: would be counted
    pipe._fuse_blocks(ctx, grid, [pl.Block(grid, (0, 0, 0), grid.dims)], layout_given=True)
    assert ctx.names()[0] == "attach_grid" and ctx.log[0][1][0] is grid and "count_bricks" not in ctx.names()
    assert pipe.grid is grid and pipe.stats["sparse"] and "render_s" not in pipe.timings and "blocks_s" not in pipe.timings


def test_fusion_body_three_blocks_attach_core_fuse_extract_detach_then_one_filter(monkeypatch, capsys):
    pipe, ctx = _pipe(monkeypatch), _RecordingContext()
    blocks = pl.plan_blocks(_LATTICE, 136 ** 3)
    assert len(blocks) == 3
    xyz, rgb = pipe._fuse_blocks(ctx, _LATTICE, blocks)
    assert ctx.names() == _PER_BLOCK * 3 + ["statistical_outlier"]
    calls = [c for c in ctx.log if c[0] in ("attach_grid", "set_block_core", "extract_mesh")]
    for k, b in enumerate(blocks):
        attach, core, mesh = calls[3 * k:3 * k + 3]
        assert attach[1][0] == b.grid and core[1] == (_LATTICE.dims, b.lo, b.hi) and mesh[2]["keys"] is True
    assert np.array_equal(xyz[:, 0], [1, 2, 2, 3, 3]) and len(rgb) == 5       # the three clouds in block order, filtered once
    vx, vr, vt = pipe.mesh
    assert vx[:, 0].tolist() == [100, 103, 106, 200, 203, 206, 300, 303, 306] and vr[:, 0].tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 3]
    assert vt.tolist() == [[2, 0, 1], [5, 3, 4], [8, 6, 7]]
    assert pipe.stats == dict(points_accumulated=12, points_dropped=0, voxels=6, after_outlier_filter=5, sparse=False, bricks_tsdf=0,
                              bricks_centroid=0, pool_refused=0, blocks=3, mesh_vertices=9, mesh_triangles=3)
    assert sorted(pipe.timings) == ["blocks_s", "bound_and_allocate_s", "extract_and_filter_s", "fuse_s", "mesh_s"]
    assert pipe.grid is _LATTICE and pipe.blocks == [b.grid for b in blocks]
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "  Lattice (256, 200, 96) @ 10 mm, origin [0. 0. 0.]: 4915200 voxels in 3 blocks"
    assert out[1:3] == ["", "--- Step 3: Fuse depth frames block by block (TSDF + voxel centroids) ---"]
    assert [l.split(",")[0] for l in out[3:6]] == ["  Block 1 at (0", "  Block 2 at (128", "  Block 3 at (0"]
    assert out[6:] == ["Camera 0: fused", "Camera 1: fused", "", "--- Step 4: Extract and clean point cloud ---",
                       "  Mesh: 9 vertices, 3 triangles (welded from 3 blocks)", "", "Final reconstruction: 5 points, 2 cameras"]


def test_fusion_body_refuses_render_dir_with_three_blocks_before_attaching(monkeypatch, tmp_path):
    pipe, ctx = _pipe(monkeypatch, render_dir=str(tmp_path)), _RecordingContext()
    with pytest.raises(ValueError, match="render_dir"):
        pipe._fuse_blocks(ctx, _LATTICE, pl.plan_blocks(_LATTICE, 136 ** 3))
    assert ctx.log == []
