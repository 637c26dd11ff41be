"""Inputs the mesh component tests share (CPU and GPU): the crafted grid of test_gpu_mesh.py with its pinned figures, the
topologies on which a union-find goes wrong, and a small scene with a flying speck."""
import numpy as np

import mesh_reference as mr
from helpers import SMALL, small_scene_frames

# ---- the crafted grid of test_gpu_mesh.py: three spheres, 2 % exact zeros, unobserved slabs ---------------------------------
DIMS, VOXEL, CENTRE = (40, 24, 72), 0.02, (0.3, 0.2, 0.7)
# kept vertices / triangles / components by min_triangles, at min_weight 0 (measured with the references on the CPU)
KEPT = {0: (5135, 9188, 119), 1: (5096, 9188, 80), 10: (4769, 8940, 9), 11: (4741, 8910, 6), 19: (4705, 8869, 3),
        1565: (3860, 7305, 2), 5445: (2877, 5445, 1), 5446: (0, 0, 0)}


def crafted_records():
    """(records, origin): `_crafted` of test_gpu_mesh.py, over the origin make_pair gives the grid"""
    origin = tuple(CENTRE[i] - 0.5 * DIMS[i] * VOXEL for i in range(3))
    dims, voxel = DIMS, VOXEL
    rng = np.random.default_rng(7)
    ii, jj, kk = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    p = np.stack([origin[a] + (g + 0.5) * voxel for a, g in enumerate((ii, jj, kk))], axis=-1)
    s1 = np.linalg.norm(p - np.array([0.1, 0.05, 0.3]), axis=-1) - 0.17
    s2 = np.linalg.norm(p - np.array([0.45, 0.2, 0.9]), axis=-1) - 0.3
    s3 = np.linalg.norm(p - np.array([0.2, 0.1, 1.4]), axis=-1) - 0.2
    sdf = np.minimum(np.minimum(s1, s2), s3)
    t = np.clip(sdf / (3 * voxel), -1.0, 1.0)
    w = rng.integers(1, 4, size=dims)
    q = np.rint(t * 32767.0).astype(np.int64)
    q[rng.random(dims) < 0.02] = 0
    s = q * w
    s[np.abs(sdf) > 3.5 * voxel] = np.sign(sdf[np.abs(sdf) > 3.5 * voxel]).astype(np.int64) * 32767 * w[np.abs(sdf) > 3.5 * voxel]
    w[:, :, 30:33] = 0
    s[:, :, 30:33] = 0
    w[5:9, 3:7, :] = 0
    s[5:9, 3:7, :] = 0
    return mr.records_from_volume(s, w), origin


_MESHES = {}


def crafted_mesh(min_weight):
    """the reference mesh of the crafted grid, computed once and shared (read-only)"""
    if min_weight not in _MESHES:
        rec, origin = crafted_records()
        mesh = mr.extract_mesh(rec, DIMS, origin, VOXEL, min_weight=min_weight)
        for a in mesh:
            a.setflags(write=False)
        _MESHES[min_weight] = mesh
    return _MESHES[min_weight]


# ---- topologies where a union-find goes wrong: long chains across every XCD, one contended word --------------------------------
def _strip(ids):
    """the triangle strip (ids[j], ids[j + 1], ids[j + 2]) over the vertices ids, in strip order"""
    ids = np.asarray(ids, np.uint32)
    return np.stack([ids[:-2], ids[1:-1], ids[2:]], axis=1)


def topology(name):
    """(tris u32 [T,3], n_vert)"""
    n = 1 << 20
    if name == "strip ascending":
        return _strip(np.arange(n)), n
    if name == "strip descending":
        return _strip(np.arange(n)[::-1]), n
    if name == "strip permuted":
        rng = np.random.default_rng(11)
        tris = _strip(rng.permutation(n))
        return np.ascontiguousarray(tris[rng.permutation(len(tris))]), n
    if name == "4096 strips interleaved":                          # vertex j of strip s has id j * 4096 + s
        ids = np.arange(256)[None, :] * 4096 + np.arange(4096)[:, None]
        return np.ascontiguousarray(np.concatenate([_strip(row) for row in ids])), n
    if name in ("fan, hub last", "fan, hub first"):                # one hub in 2^18 triangles with 2^19 rim vertices
        m = 1 << 18
        rim = np.arange(2 * m, dtype=np.uint32).reshape(m, 2)
        hub = 2 * m if name == "fan, hub last" else 0
        rim = rim + (0 if hub else 1)
        return np.ascontiguousarray(np.concatenate([np.full((m, 1), hub, np.uint32), rim], axis=1)), 2 * m + 1
    if name == "one vertex 65536 times":                           # (7, 7, 7) among isolated vertices
        return np.full((1 << 16, 3), 7, np.uint32), 1000
    raise KeyError(name)


TOPOLOGIES = ("strip ascending", "strip descending", "strip permuted", "4096 strips interleaved", "fan, hub last", "fan, hub first",
              "one vertex 65536 times")


# ---- a small scene with a flying speck -------------------------------------------------------------------------------------------
SPECK_GRID = dict(dims=(96, 96, 96), voxel=0.025, centre=(0.0, -0.2, 0.0))
SPECK_MIN_TRIANGLES = 100


def speck_scene():
    """(poses, frames, speck): three frames of the small scene; frames 1 and 2 see a 44-pixel patch of near depth at ONE world
    point 0.45 m in front of camera 1 (two of three observations, so the speck's zero crossing survives the averaging).  With the
    references (oracle TSDF, mesh_reference, mesh_components_reference; test_mesh_components_reference_cpu.py) the mesh over
    SPECK_GRID has one component of 6 562 triangles, the speck's of 68 within 0.1 m of `speck`, and fragments of at most 20."""
    poses, frames = small_scene_frames(n=3, deg=4.0)
    frames = [(d.copy(), c.copy()) for d, c in frames]
    R1, t1 = np.asarray(poses[1][0]), np.asarray(poses[1][1]).reshape(3)
    speck = R1.T @ (np.array([-0.12, -0.10, 0.45]) - t1)
    for i in (1, 2):
        R, t = np.asarray(poses[i][0]), np.asarray(poses[i][1]).reshape(3)
        q = R @ speck + t
        u, v = int(round(SMALL["fx"] * q[0] / q[2] + SMALL["cx"])), int(round(SMALL["fy"] * q[1] / q[2] + SMALL["cy"]))
        frames[i][0][v - 22:v + 22, u - 22:u + 22] = q[2]
    return poses, frames, speck
