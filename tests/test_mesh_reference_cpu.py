"""CPU: the numpy marching cubes of tests/mesh_reference.py on an analytic sphere, the PLY mesh writer,
and the command line's --mesh-output flag."""
import os
import subprocess
import sys

import numpy as np

import mesh_reference as mr
from tl3d import fileio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, VOXEL, ORIGIN = (40, 24, 48), 0.02, (-0.41, -0.23, -0.47)
CENTRE, RADIUS, TRUNC = np.array([0.0, 0.0, 0.02]), 0.17, 4 * 0.02


def sphere_grid():
    """record-ordered {sum, weight} of a sphere SDF truncated at 4 voxels, weight 3, no voxel at exactly sum = 0"""
    ii, jj, kk = np.meshgrid(*[np.arange(n) for n in DIMS], indexing="ij")
    p = np.stack([ORIGIN[a] + (g + 0.5) * VOXEL for a, g in enumerate((ii, jj, kk))], axis=-1)
    sdf = np.linalg.norm(p - CENTRE, axis=-1) - RADIUS
    t = np.clip(sdf / TRUNC, -1.0, 1.0)
    q = np.rint(t * 32767.0).astype(np.int64)
    assert not (q == 0).any()
    w = 3
    return mr.records_from_volume(q * w, np.full(DIMS, w)), sdf


def test_sphere_mesh_is_closed_genus_zero_outward_and_interpolated():
    rec, sdf = sphere_grid()
    xyz, rgb, tris = mr.extract_mesh(rec, DIMS, ORIGIN, VOXEL)
    assert len(tris) > 1000 and (rgb == 128).all()
    t = tris.astype(np.int64)
    # closed: every undirected edge in exactly two triangles, once in each direction
    directed = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    keys = directed[:, 0] * len(xyz) + directed[:, 1]
    assert len(np.unique(keys)) == len(keys)                          # no directed edge twice
    rev = directed[:, 1] * len(xyz) + directed[:, 0]
    assert np.isin(rev, keys).all()                                    # every edge's reverse is there
    used = np.unique(t)
    assert len(used) == len(xyz)                                       # (inside the band every vertex is in a triangle)
    n_edges = len(keys) // 2
    assert len(used) - n_edges + len(t) == 2                           # Euler characteristic of a sphere
    # outward: the face normal points away from the centre
    p = xyz.astype(np.float64)
    n = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    c = p[t].mean(axis=1) - CENTRE
    assert (np.einsum("ij,ij->i", n, c) > 0).all()
    # vertices where linear interpolation of the (unquantised) SDF along the edge puts them
    g = (p - np.array(ORIGIN)) / VOXEL - 0.5                           # grid coordinates
    lo = np.floor(g + 1e-6).astype(np.int64)
    ax = np.argmax(np.abs(g - lo) > 1e-6, axis=1)
    hi = lo.copy()
    hi[np.arange(len(hi)), ax] += 1
    sa = sdf[lo[:, 0], lo[:, 1], lo[:, 2]]
    sb = sdf[hi[:, 0], hi[:, 1], hi[:, 2]]
    frac = sa / (sa - sb)
    expect = lo + 0.0
    expect[np.arange(len(hi)), ax] += frac
    assert np.abs(g - expect).max() < 1e-3
    # and close to the sphere itself (a linear interpolation of a curved field)
    assert np.abs(np.linalg.norm(p - CENTRE, axis=1) - RADIUS).max() < 0.1 * VOXEL


def test_reference_vertices_follow_the_rule_and_zeros_get_vertices():
    """t == 0 at one end: the mesh has a vertex there (frac 0 or 1), TSDF-mode extraction (t_a * t_b < 0) has none; rim and
    unobserved / truncated voxels produce nothing."""
    dims = (8, 8, 16)
    s = np.zeros(dims, np.int64)
    w = np.ones(dims, np.int64)
    s[:, :, :8] = -1000
    s[:, :, 8] = 0                                # an exact zero layer
    s[:, :, 9:] = 1000
    s[:, :, 14:] = 32767                          # truncated: not usable
    w[0, 0, :] = 0                                # an unobserved column
    xyz, _, tris = mr.extract_mesh(mr.records_from_volume(s, w), dims, (0.0, 0.0, 0.0), 1.0)
    z = xyz[:, 2]
    assert len(xyz) == 8 * 8 - 1 and np.allclose(z, 8.5)               # edge (7, 8): frac 1, the vertex sits on the zero voxel
    assert len(tris) == 2 * 7 * 7 - 2                                  # a plane over the 7 x 7 cells, one cell dropped at the hole


def _read_ply_mesh(path):
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    nv = int(next(l for l in head if l.startswith("element vertex")).split()[-1])
    nf = int(next(l for l in head if l.startswith("element face")).split()[-1])
    assert head[1] in ("format binary_little_endian 1.0", "format ascii 1.0")
    assert "property list uchar int vertex_indices" in head
    if head[1].startswith("format ascii"):
        rows = data[end:].decode("ascii").splitlines()
        v = np.array([r.split() for r in rows[:nv]], dtype=object)
        xyz = v[:, :3].astype(np.float32) if nv else np.zeros((0, 3), np.float32)
        rgb = v[:, 3:].astype(np.uint8) if nv else np.zeros((0, 3), np.uint8)
        f = np.array([[int(x) for x in r.split()] for r in rows[nv:nv + nf]], np.int64).reshape(-1, 4)
        assert (f[:, 0] == 3).all() and len(rows) == nv + nf
        return xyz, rgb, f[:, 1:]
    vt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert len(data) == end + nv * vt.itemsize + nf * ft.itemsize
    v = np.frombuffer(data, vt, nv, end)
    f = np.frombuffer(data, ft, nf, end + nv * vt.itemsize)
    assert (f["n"] == 3).all()
    return (np.stack([v["x"], v["y"], v["z"]], 1), np.stack([v["r"], v["g"], v["b"]], 1), f["v"].astype(np.int64))


def test_ply_mesh_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(50, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, size=(50, 3)).astype(np.uint8)
    tris = rng.integers(0, 50, size=(70, 3)).astype(np.uint32)
    for ascii_ in (False, True):
        path = tmp_path / "m_ascii.ply" if ascii_ else tmp_path / "sub" / "m.ply"
        fileio.write_ply_mesh(path, xyz, rgb, tris, ascii=ascii_)
        a, b, c = _read_ply_mesh(path)
        assert np.array_equal(a, xyz) and np.array_equal(b, rgb) and np.array_equal(c, tris.astype(np.int64))
    fileio.write_ply_mesh(tmp_path / "empty.ply", np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    a, b, c = _read_ply_mesh(tmp_path / "empty.ply")
    assert len(a) == 0 and len(c) == 0


def test_cli_lists_mesh_output():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "depth_to_reconstruction.py"), "--help"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "--mesh-output" in out.stdout
