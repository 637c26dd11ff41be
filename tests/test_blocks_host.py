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
