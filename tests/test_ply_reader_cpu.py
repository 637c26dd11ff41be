"""CPU: fileio.read_ply_points reads what the project's three PLY writers write and what the reference writes."""
import os

import numpy as np
import pytest

from tl3d import fileio


def _cloud(n=257, seed=0):
    r = np.random.default_rng(seed)
    return (r.normal(size=(n, 3)) * 3).astype(np.float32), r.integers(0, 256, (n, 3)).astype(np.uint8)


def test_round_trips_the_ascii_writer(tmp_path):
    xyz, rgb = _cloud()
    fileio.write_ply_ascii(tmp_path / "a.ply", xyz, rgb)
    got = fileio.read_ply_points(tmp_path / "a.ply")
    assert got.dtype == np.float32 and np.array_equal(got, xyz)              # str() of a float32 round-trips


@pytest.mark.parametrize("double_xyz", [True, False])
def test_round_trips_the_binary_writer(tmp_path, double_xyz):
    xyz, rgb = _cloud(seed=1)
    fileio.write_ply_binary(tmp_path / "b.ply", xyz.astype(np.float64) if double_xyz else xyz, rgb, double_xyz=double_xyz)
    got = fileio.read_ply_points(tmp_path / "b.ply")
    assert got.dtype == np.float32 and got.shape == (len(xyz), 3) and np.array_equal(got, xyz)


@pytest.mark.parametrize("ascii", [False, True])
@pytest.mark.parametrize("normals", [False, True])
def test_round_trips_the_mesh_writer_and_skips_faces(tmp_path, ascii, normals):
    xyz, rgb = _cloud(n=40, seed=2)
    tris = np.random.default_rng(3).integers(0, 40, (70, 3)).astype(np.uint32)
    fileio.write_ply_mesh(tmp_path / "m.ply", xyz, rgb, tris, ascii=ascii, normals=_cloud(n=40, seed=4)[0] if normals else None)
    assert np.array_equal(fileio.read_ply_points(tmp_path / "m.ply"), xyz)


def test_empty_cloud_and_errors(tmp_path):
    fileio.write_ply_binary(tmp_path / "e.ply", np.zeros((0, 3)), np.zeros((0, 3), np.uint8))
    assert fileio.read_ply_points(tmp_path / "e.ply").shape == (0, 3)
    (tmp_path / "x.ply").write_bytes(b"not a ply")
    with pytest.raises(ValueError):
        fileio.read_ply_points(tmp_path / "x.ply")
    (tmp_path / "be.ply").write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
    with pytest.raises(ValueError):
        fileio.read_ply_points(tmp_path / "be.ply")
    xyz, rgb = _cloud(n=5)
    fileio.write_ply_binary(tmp_path / "t.ply", xyz, rgb)
    data = (tmp_path / "t.ply").read_bytes()
    (tmp_path / "t.ply").write_bytes(data[:-10])
    with pytest.raises(ValueError):
        fileio.read_ply_points(tmp_path / "t.ply")


@pytest.mark.parametrize("name", ["ascii_d2r.ply", "ascii_der.ply"])
def test_reads_the_references_files(golden_dir, name):
    path = os.path.join(golden_dir, name)
    got = fileio.read_ply_points(path)
    with open(path) as f:
        lines = f.read().split("end_header\n", 1)[1].splitlines()
    want = np.array([ln.split()[:3] for ln in lines if ln.strip()], dtype=np.float64).astype(np.float32)
    assert len(got) > 0 and got.dtype == np.float32 and np.array_equal(got, want)
