"""The voxel lattice of a scene on the host: its origin and dims (Open3D's voxel origin), the grid or the blocks it is fused in, and
the weld of the blocks' meshes.  Geometry only: numpy, GridSpec and the channel constants -- no device call."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from ._cabi import CH_CENTROID, CH_TSDF
from .fusion import GridSpec

MAX_BLOCK_VOXELS = 1 << 32            # voxels of one grid, halo included: its brick table is direct-indexed


def lattice_extent(bounds_min, bounds_max, voxel_size):
    """(origin, dims) of the lattice that covers the bounds: Open3D's voxel origin (min_bound - voxel/2), dims in multiples of 8."""
    v = float(voxel_size)
    origin = np.asarray(bounds_min, np.float64) - 0.5 * v
    dims = np.floor((np.asarray(bounds_max, np.float64) - origin) / v).astype(np.int64) + 1
    return origin, np.maximum(8, ((dims + 7) // 8) * 8)


def plan_grid(bounds_min, bounds_max, voxel_size, grid_dim, channels=CH_TSDF | CH_CENTROID, trunc_voxels=4.0,
              max_voxels=None, sparse_bytes=None):
    """Grid with Open3D's voxel origin (min_bound - voxel/2) covering the bounds.

    Up to a voxel BUDGET (default grid_dim^3 voxels in total; not a cube: a 2 m x 2.4 m x 12 m corridor at 5 mm becomes
    400 x 480 x 2400 voxels) the grid is dense.  Beyond it the grid is SPARSE, as the reference's hash-map merge is
    (D2R:404-410): the same dims, records only for the bricks the data touches, pools sized by sparse_bytes (default: the dense
    budget's bytes) -- a GUESS when nothing is known about the frames; choose_layout() replaces it by a count.  Only a scene of
    more than 2^32 voxels is shrunk about its centre -- longest axis first -- and `clipped` returned True (points outside are
    dropped and counted by the accumulation kernels; the caller prints the warning)."""
    v = float(voxel_size)
    mn, mx = np.asarray(bounds_min, np.float64), np.asarray(bounds_max, np.float64)
    origin, dims = lattice_extent(mn, mx, v)
    budget = int(grid_dim) ** 3 if max_voxels is None else int(max_voxels)
    budget = max(512, min(budget, 1 << 32))
    clipped = False
    want = dims.copy()
    while int(dims[0]) * int(dims[1]) * int(dims[2]) > (1 << 32):    # shave the (currently) longest axis, 8 voxels at a time
        a = int(np.argmax(dims))
        if dims[a] <= 8:
            break
        dims[a] -= 8
        clipped = True
    for a in range(3):
        if dims[a] < want[a]:
            origin[a] = 0.5 * (mn[a] + mx[a]) - 0.5 * dims[a] * v
    nvox = int(dims[0]) * int(dims[1]) * int(dims[2])
    pool_t = pool_c = 0
    if nvox > budget:
        per_vox = (8 if channels & CH_TSDF else 0) + (32 if channels & CH_CENTROID else 0)
        mem = int(sparse_bytes) if sparse_bytes is not None else budget * per_vox
        # surfaces: the TSDF band is ~3 bricks thick where the centroid channel holds one layer: 12 KB + 16 KB per surface brick
        unit = (3 * 4096 if channels & CH_TSDF else 0) + (16384 if channels & CH_CENTROID else 0)
        surf = max(4096, mem // unit)
        pool_t = int(min(nvox // 512, 3 * surf)) if channels & CH_TSDF else 0
        pool_c = int(min(nvox // 512, surf)) if channels & CH_CENTROID else 0
    return GridSpec(tuple(int(d) for d in dims), tuple(float(o) for o in origin), v, trunc_voxels * v, channels,
                    pool_tsdf=pool_t, pool_centroid=pool_c), clipped


def plan_lattice(bounds_min, bounds_max, voxel_size, grid_dim, channels=CH_TSDF | CH_CENTROID, trunc_voxels=4.0) -> GridSpec:
    """The whole lattice of the scene, never shaved: lattice_extent()'s origin and dims.  A lattice of at most 2^32 voxels is
    plan_grid()'s grid exactly (its layout guess included); a larger one is fused block by block (plan_blocks) and each block
    chooses its own layout."""
    grid, clipped = plan_grid(bounds_min, bounds_max, voxel_size, grid_dim, channels=channels, trunc_voxels=trunc_voxels)
    if not clipped:
        return grid
    v = float(voxel_size)
    origin, dims = lattice_extent(bounds_min, bounds_max, v)
    return GridSpec(tuple(int(d) for d in dims), tuple(float(o) for o in origin), v, trunc_voxels * v, channels)


def layout_from_counts(grid: GridSpec, bricks_tsdf: int, bricks_centroid: int) -> GridSpec:
    """Per channel: a pool of the counted bricks (+ 3 % + 2048: a slot lost to a race between two waves is not reused) when that
    is less than half of the dense channel, else the dense channel."""
    nbr = grid.nvox // 512
    pool_t = pool_c = 0
    if grid.channels & CH_TSDF:
        want = int(bricks_tsdf * 1.03) + 2048
        pool_t = want if 2 * want < nbr else 0
    if grid.channels & CH_CENTROID:
        want = int(bricks_centroid * 1.03) + 2048
        pool_c = want if 2 * want < nbr else 0
    return GridSpec(grid.dims, grid.origin, grid.voxel_size, grid.sdf_trunc, grid.channels, pool_tsdf=pool_t, pool_centroid=pool_c,
                    voxel_offset=grid.voxel_offset)


def halve(off, core):
    """THE halving rule: a box of voxels (offset, dims; multiples of 8) cut across its longest axis at a multiple of 8."""
    a = int(np.argmax(core))
    if core[a] <= 8:
        raise ValueError(f"block {tuple(core)} at {tuple(off)} cannot be split further")
    h = ((int(core[a]) // 2 + 7) // 8) * 8
    c0, c1, o1 = list(core), list(core), list(off)
    c0[a], c1[a], o1[a] = h, int(core[a]) - h, int(off[a]) + h
    return (tuple(off), tuple(c0)), (tuple(o1), tuple(c1))


def tile(dims, fits):
    """[(offset, dims)] of disjoint boxes that tile a lattice of `dims` voxels, halved until fits(offset, dims) holds for every one;
    sorted by offset z, y, x."""
    out, todo = [], [((0, 0, 0), tuple(int(d) for d in dims))]
    while todo:
        off, core = todo.pop()
        if fits(off, core):
            out.append((off, core))
        else:
            todo.extend(halve(off, core))
    return sorted(out, key=lambda b: b[0][::-1])


@dataclass
class Block:
    """One block of a lattice: its grid (core + halo, grid.voxel_offset = the core's first lattice voxel) and its core [lo, hi) in
    grid-local voxels.  The halo is one brick on every + side that has a next block: what the last cell layer of the core reads."""
    grid: GridSpec
    lo: Tuple[int, int, int]
    hi: Tuple[int, int, int]


def _make_block(lattice: GridSpec, off, core) -> Block:
    dims = tuple(int(core[a]) + (8 if int(off[a]) + int(core[a]) < int(lattice.dims[a]) else 0) for a in range(3))
    grid = GridSpec(dims, lattice.origin, lattice.voxel_size, lattice.sdf_trunc, lattice.channels,
                    voxel_offset=tuple(int(o) for o in off))
    return Block(grid, (0, 0, 0), tuple(int(c) for c in core))


def split_block(lattice: GridSpec, block: Block) -> List[Block]:
    """The block's core halved (halve), each half with its own halo."""
    core = tuple(h - l for h, l in zip(block.hi, block.lo))
    return [_make_block(lattice, o, c) for o, c in halve(block.grid.voxel_offset, core)]


def plan_blocks(lattice: GridSpec, max_voxels: Optional[int] = None) -> List[Block]:
    """Disjoint block cores that tile the lattice (tile), each block's grid -- core PLUS halo -- of at most max_voxels (default
    MAX_BLOCK_VOXELS).  A lattice within the limit is ONE block: the lattice grid itself, offset 0, no halo, no core."""
    limit = MAX_BLOCK_VOXELS if max_voxels is None else int(max_voxels)
    if lattice.nvox <= limit:
        return [Block(lattice, (0, 0, 0), tuple(int(d) for d in lattice.dims))]
    return [_make_block(lattice, o, c) for o, c in tile(lattice.dims, lambda o, c: _make_block(lattice, o, c).grid.nvox <= limit)]


def _core_owned(keys, lattice_dims, lo, hi):
    """Which keyed vertices (key = 3 * lattice linear index of the owner voxel + axis) have their owner in the lattice box [lo, hi)."""
    lx, ly = int(lattice_dims[0]), int(lattice_dims[1])
    idx = np.asarray(keys, np.int64) // 3
    x, y, z = idx % lx, (idx // lx) % ly, idx // (lx * ly)
    return ((x >= lo[0]) & (x < hi[0]) & (y >= lo[1]) & (y < hi[1]) & (z >= lo[2]) & (z < hi[2]))


def weld_meshes(parts, lattice_dims):
    """One mesh from the keyed meshes of the blocks of a lattice.  parts: [(xyz, rgb, tris, keys, core_lo, core_hi)] with the core
    in LATTICE voxels.  Every vertex whose owner voxel lies in its block's core is kept (each owned edge vertex exists in exactly one
    core, the unreferenced ones included, as in a single grid); a triangle's halo-owned vertices are found through their keys among
    the kept ones.  Returns (xyz, rgb, tris, keys)."""
    kx, kr, kk = [], [], []
    for xyz, rgb, _tris, keys, lo, hi in parts:
        own = _core_owned(keys, lattice_dims, lo, hi)
        kx.append(np.asarray(xyz)[own])
        kr.append(np.asarray(rgb)[own])
        kk.append(np.asarray(keys, np.int64)[own])
    xyz = np.concatenate(kx) if kx else np.zeros((0, 3), np.float32)
    rgb = np.concatenate(kr) if kr else np.zeros((0, 3), np.uint8)
    allk = np.concatenate(kk) if kk else np.zeros(0, np.int64)
    order = np.argsort(allk, kind="stable")
    sk = allk[order]
    if len(sk) > 1 and np.any(sk[1:] == sk[:-1]):
        raise ValueError("weld_meshes: a vertex is owned by two block cores (the cores overlap)")
    out = []
    for _xyz, _rgb, tris, keys, _lo, _hi in parts:
        tris = np.asarray(tris)
        if len(tris) == 0:
            continue
        tk = np.asarray(keys, np.int64)[tris.astype(np.int64)]
        pos = np.searchsorted(sk, tk)
        pos = np.minimum(pos, max(0, len(sk) - 1))
        if len(sk) == 0 or not np.array_equal(sk[pos], tk):
            raise ValueError("weld_meshes: a triangle references a vertex no block core owns (a halo is missing)")
        out.append(order[pos].astype(np.uint32))
    tris = np.concatenate(out) if out else np.zeros((0, 3), np.uint32)
    return xyz, rgb, tris, allk


def align_grid_to_open3d(grid: GridSpec, min_bound) -> GridSpec:
    """Shift a grid by less than one voxel so its lattice coincides with Open3D's (voxel origin = min_bound - voxel/2,
    depth_to_reconstruction.py:410).  With the lattices in phase the fused centroids are the reference's centroids up
    to the accumulator quantum; out of phase, two 5 mm samplings of one surface sit 1-2 mm apart."""
    v = float(grid.voxel_size)
    o3d = np.asarray(min_bound, np.float64) - 0.5 * v
    org = np.asarray(grid.origin, np.float64)
    shift = np.mod(o3d - org, v)                       # in [0, v)
    return GridSpec(grid.dims, tuple(float(x) for x in org + shift - v), grid.voxel_size, grid.sdf_trunc, grid.channels)
