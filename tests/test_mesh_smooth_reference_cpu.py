"""CPU: the rules of mesh smoothing and vertex normals do what smoothing should, on the reference alone
(tests/mesh_smooth_reference.py), plus everything around the kernels that needs no GPU: dbl(), the renumbering property, the PLY
writer with normals, the configuration checks, the command-line errors and the argument checks of the two calls."""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import mesh_smooth_reference as ref
from mesh_smooth_common import SMALL_SHAPES, SPHERE, extremes, fan, noisy_sphere, radial, renumber, small_shape, soup
from tl3d import _cabi as abi
from tl3d import fileio
from tl3d.config import ReconstructionConfig
from tl3d.pipeline import DepthToReconstructionPipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rms_dev(xyz):
    r = radial(xyz)
    return float(np.sqrt(np.mean((r - r.mean()) ** 2)))


def test_sphere_is_the_issue_s_sphere():
    xyz, tris, _ = noisy_sphere()
    _, val = ref.unique_edges(tris, len(xyz))
    assert len(xyz) == 642 and len(tris) == 1280 and sorted(set(val.tolist())) == [5, 6] and (val == 5).sum() == 12


def test_taubin_smooths_without_shrinking_and_laplace_shrinks():
    xyz, tris, _ = noisy_sphere()
    out, info = ref.smooth(xyz, tris, 10)
    ratio, drift = _rms_dev(out) / _rms_dev(xyz), radial(out).mean() / radial(xyz).mean() - 1.0
    lap, _ = ref.smooth(xyz, tris, 10, mu=0.0)
    shrink = radial(lap).mean() / radial(xyz).mean() - 1.0
    print(f"rms radial deviation x{ratio:.3f}, mean radius {drift:+.3%}; mu = 0: {shrink:+.3%}; {info['edges']} edges")
    assert info["edges"] == 1920 and info["max_valence"] == 6
    assert ratio < 0.6
    assert abs(drift) < 0.01
    assert shrink < -0.03


def test_normals_point_outward_after_three_iterations():
    xyz, tris, d = noisy_sphere()
    out, _ = ref.smooth(xyz, tris, 3)
    n, zero = ref.normals(out, tris)
    dots = (n.astype(np.float64) * d).sum(axis=1)
    print(f"smallest dot product with the radial direction {dots.min():.4f}")
    assert zero == 0 and dots.min() > 0.98
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 1e-6


@pytest.mark.parametrize("name", ["sphere", "fan", "soup", "extremes"] + list(SMALL_SHAPES))
def test_renumbered_mesh_gives_the_renumbered_result(name):
    """the contract's point: permuting the vertices, shuffling the triangles and rotating their corners changes nothing but the order"""
    build = {"sphere": lambda: noisy_sphere()[:2], "fan": lambda: fan(256), "soup": soup, "extremes": extremes}
    xyz, tris = build[name]() if name in build else small_shape(name)
    if name == "soup":
        xyz, tris = xyz[:4096], tris[(tris < 4096).all(axis=1)]
    it = 3
    out, info = ref.smooth(xyz, tris, it)
    nrm, nz = ref.normals(out, tris)
    xyz2, tris2, perm = renumber(xyz, tris, seed=11)
    out2, info2 = ref.smooth(xyz2, tris2, it)
    nrm2, nz2 = ref.normals(out2, tris2)
    assert info2["edges"] == info["edges"] and nz2 == nz
    assert np.array_equal(info2["valence"][perm], info["valence"])
    assert out2[perm].tobytes() == out.tobytes() and nrm2[perm].tobytes() == nrm.tobytes()


def test_dbl_takes_sign_and_magnitude_apart():
    assert ref.dbl(-5) == -5.0 and ref.dbl(5) == 5.0 and ref.dbl(0) == 0.0
    assert ref.dbl(1 << 64) == 2.0 ** 64 and ref.dbl(-(1 << 64)) == -(2.0 ** 64)
    assert ref.dbl((1 << 64) + 5) == 2.0 ** 64                       # 5 is below half an ulp of 2^64
    assert ref.dbl(-((3 << 64) + (1 << 63))) == -(3.5 * 2.0 ** 64)
    assert ref.dbl((1 << 122) + (1 << 70)) == 2.0 ** 122 + 2.0 ** 70 and ref.dbl(-((1 << 122) + 1)) == -(2.0 ** 122)
    n = (1 << 64) + (1 << 11) + 1
    assert ref.dbl(n) == float(1 << 64) + float((1 << 11) + 1) == 2.0 ** 64 + 4096.0 and float(n) == 2.0 ** 64 + 4096.0
    # hi and lo are rounded apart and their sum once more: not always the nearest double of N, but the contract's
    n = (((1 << 53) + 1) << 64) + (1 << 63)
    assert ref.dbl(n) == 2.0 ** 117 and float(n) == 2.0 ** 117 + 2.0 ** 65
    # the array form agrees with the scalar one
    vals = [0, 1, -1, 5, -5, (1 << 62) + 12345, -((1 << 62) + 12345), (1 << 53) + 1, -((1 << 53) + 1)]
    a = np.array(vals, object)
    assert np.array_equal(ref._dbl_array(a), np.array([ref.dbl(v) for v in vals]))
    # (a low word of 2^63 and more that no double holds: where a signed or a truncating conversion of it would show)
    wide = np.array(vals + [(1 << 75) + 12345, -((1 << 100) + (1 << 40) + 1), (5 << 64) + (1 << 63) + 12345, -((1 << 63) + 12345),
                            (1 << 64) - 1, -((7 << 64) + (1 << 64) - 1025)], object)
    assert np.array_equal(ref._dbl_array(wide), np.array([ref.dbl(v) for v in wide]))


def test_quantisation():
    x = np.array([0.5, -0.5, 1048576.0, -1048576.0, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, 0.1], np.float32)
    q = ref.quantise(x)
    assert q.tolist()[:7] == [1 << 23, -(1 << 23), 1 << 44, -(1 << 44), 0, 2, 1]          # halves to even
    big = np.array([0.5, 0.75, 1.0000001, 123.456, 1048575.9], np.float32)
    assert np.array_equal(ref.quantise(big).astype(np.float64) / 16777216.0, big.astype(np.float64))     # exact from 0.5 m upward


def test_reference_against_rationals_on_a_small_mesh():
    """one step and the normal sums again, with Python sets, loops and Fractions"""
    xyz, tris = small_shape("(a, a, b) beside a triangle")
    nb = {v: set() for v in range(len(xyz))}
    for t in tris.tolist():
        for u in t:
            for v in t:
                if u != v:
                    nb[u].add(v)
    q = [[int(round(Fraction(float(c)) * (1 << 24))) for c in p] for p in xyz]      # (round() of a Fraction: halves to even)
    edges, val = ref.unique_edges(tris, len(xyz))
    assert val.tolist() == [len(nb[v]) for v in range(len(xyz))] == [3, 2, 2, 1] and len(edges) == 4
    got = ref.step(xyz, edges, val, 0.5)
    for v in range(len(xyz)):
        for a in range(3):
            D = sum(q[j][a] for j in nb[v]) - len(nb[v]) * q[v][a]
            want = np.float32(float(xyz[v, a]) + 0.5 * (ref.dbl(D) / (float(len(nb[v])) * 16777216.0)))
            assert got[v, a] == want
    N = ref.normal_sums(xyz, tris)
    e1, e2 = [q[1][a] - q[0][a] for a in range(3)], [q[2][a] - q[0][a] for a in range(3)]
    F = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    assert [list(N[v]) for v in range(4)] == [F, F, F, [0, 0, 0]]


def test_small_shapes():
    n, z = ref.normals(*small_shape("pair that cancels"))
    assert z == 3 and not n.any()
    xyz, tris = small_shape("twice and reversed")
    n, z = ref.normals(xyz, tris)
    one, _ = ref.normals(xyz, tris[:1])
    assert z == 0 and n.tobytes() == one.tobytes()                  # F + F - F = F
    n, z = ref.normals(*small_shape("(a, a, b)"))
    assert z == 3 and not n.any()
    out, info = ref.smooth(*small_shape("(a, a, b)"), 1)
    assert info["valence"].tolist() == [1, 2, 1] and info["edges"] == 2
    out, info = ref.smooth(*small_shape("two triangles on one edge"), 2)
    assert info["edges"] == 5 and info["valence"].tolist() == [2, 3, 3, 2]
    xyz, tris = small_shape("isolated vertex")
    out, info = ref.smooth(xyz, tris, 2)
    assert info["valence"].tolist() == [2, 2, 2, 0, 0] and out[3:].tobytes() == xyz[3:].tobytes() and out[:3].tobytes() != xyz[:3].tobytes()
    out, info = ref.smooth(xyz, tris, 0)
    assert out.tobytes() == xyz.tobytes() and info["edges"] == 3
    out, info = ref.smooth(*small_shape("no triangle"), 5)
    assert info["edges"] == 0 and info["max_valence"] == 0 and out.tobytes() == small_shape("no triangle")[0].tobytes()
    out, info = ref.smooth(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), 3)
    assert out.shape == (0, 3) and info["edges"] == 0 and info["max_valence"] == 0 and len(info["valence"]) == 0
    n, z = ref.normals(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    assert n.shape == (0, 3) and z == 0


def test_mu_zero_adds_exactly_nothing():
    xyz, tris, _ = noisy_sphere()
    edges, val = ref.unique_edges(tris, len(xyz))
    assert ref.step(xyz, edges, val, 0.0).tobytes() == xyz.tobytes()
    assert ref.step(xyz, edges, val, -0.0).tobytes() == xyz.tobytes()


def test_reference_refuses_what_the_call_refuses():
    xyz, tris = small_shape("one triangle")
    for bad in (np.nan, np.inf, 1048577.0, -2.0e6):
        x = xyz.copy()
        x[1, 2] = bad
        with pytest.raises(ValueError):
            ref.smooth(x, tris, 1)
        with pytest.raises(ValueError):
            ref.normals(x, tris)
    with pytest.raises(ValueError):
        ref.smooth(xyz, np.array([[0, 1, 3]], np.uint32), 1)
    for kw in (dict(lam=0.0), dict(lam=1.5), dict(lam=float("nan")), dict(mu=0.1), dict(mu=-2.5), dict(iterations=-1), dict(iterations=1001)):
        with pytest.raises(ValueError):
            ref.smooth(xyz, tris, **dict(dict(iterations=1), **kw))


# ---- PLY ------------------------------------------------------------------------------------------------------------------------
def _ply_mesh():
    xyz, tris, _ = noisy_sphere()
    rgb = np.random.default_rng(1).integers(0, 256, size=(len(xyz), 3), dtype=np.uint8)
    nrm, _ = ref.normals(xyz, tris)
    return xyz, rgb, tris, nrm


def _header(data):
    end = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:end].decode("ascii").splitlines(), end


def test_ply_with_normals_round_trips_in_binary(tmp_path):
    xyz, rgb, tris, nrm = _ply_mesh()
    fileio.write_ply_mesh(tmp_path / "n.ply", xyz, rgb, tris, normals=nrm)
    data = (tmp_path / "n.ply").read_bytes()
    head, end = _header(data)
    props = [l.split()[1:] for l in head if l.startswith("property") and "list" not in l]
    assert props == [["float", k] for k in ("x", "y", "z", "nx", "ny", "nz")] + [["uchar", k] for k in ("red", "green", "blue")]
    v = np.frombuffer(data, np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]), len(xyz), end)
    f = np.frombuffer(data, np.dtype([("k", "u1"), ("i", "<i4", 3)]), len(tris), end + 27 * len(xyz))
    assert len(data) == end + 27 * len(xyz) + 13 * len(tris)
    assert v["p"].tobytes() == xyz.tobytes() and v["n"].tobytes() == nrm.tobytes() and np.array_equal(v["c"], rgb)
    assert (f["k"] == 3).all() and np.array_equal(f["i"].astype(np.uint32), tris)


def test_ply_with_normals_round_trips_in_ascii(tmp_path):
    xyz, rgb, tris, nrm = _ply_mesh()
    fileio.write_ply_mesh(tmp_path / "n.ply", xyz, rgb, tris, ascii=True, normals=nrm)
    lines = (tmp_path / "n.ply").read_text().splitlines()
    at = lines.index("end_header") + 1
    assert lines[1] == "format ascii 1.0" and [l.split()[-1] for l in lines[3:12]] == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    rows = np.array([l.split() for l in lines[at:at + len(xyz)]])
    assert rows.shape == (len(xyz), 9)
    assert rows[:, :3].astype(np.float32).tobytes() == xyz.tobytes() and rows[:, 3:6].astype(np.float32).tobytes() == nrm.tobytes()
    assert np.array_equal(rows[:, 6:].astype(np.uint8), rgb)
    faces = np.array([l.split() for l in lines[at + len(xyz):]], np.int64)
    assert np.array_equal(faces[:, 1:].astype(np.uint32), tris) and (faces[:, 0] == 3).all()


@pytest.mark.parametrize("ascii", [False, True])
def test_ply_without_normals_is_what_it_was(tmp_path, ascii):
    xyz, rgb, tris, _ = _ply_mesh()
    fileio.write_ply_mesh(tmp_path / "a.ply", xyz, rgb, tris, ascii=ascii)
    fileio.write_ply_mesh(tmp_path / "b.ply", xyz, rgb, tris, ascii=ascii, normals=None)
    data = (tmp_path / "a.ply").read_bytes()
    assert data == (tmp_path / "b.ply").read_bytes()
    head, end = _header(data)
    assert [l.split()[-1] for l in head if l.startswith("property") and "list" not in l] == ["x", "y", "z", "red", "green", "blue"]
    if not ascii:                                                   # 15 bytes per vertex, 13 per face, as before
        assert len(data) == end + 15 * len(xyz) + 13 * len(tris)
        v = np.frombuffer(data, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]), len(xyz), end)
        assert v["p"].tobytes() == xyz.tobytes() and np.array_equal(v["c"], rgb)
    else:
        first = data[end:].decode("ascii").splitlines()[0]
        assert first == f"{xyz[0, 0]} {xyz[0, 1]} {xyz[0, 2]} {int(rgb[0, 0])} {int(rgb[0, 1])} {int(rgb[0, 2])}"


# ---- configuration and command line -------------------------------------------------------------------------------------------
def test_config_defaults():
    cfg = ReconstructionConfig()
    assert (cfg.mesh_smooth_iterations, cfg.mesh_smooth_lambda, cfg.mesh_smooth_mu, cfg.mesh_normals) == (0, 0.5, -0.53, False)
    assert DepthToReconstructionPipeline(cfg).mesh_normals is None


@pytest.mark.parametrize("kw,match", [
    (dict(mesh_smooth_iterations=3), "extract_mesh"), (dict(mesh_normals=True), "extract_mesh"),
    (dict(extract_mesh=True, mesh_smooth_iterations=-1), "mesh_smooth_iterations"),
    (dict(extract_mesh=True, mesh_smooth_iterations=1001), "mesh_smooth_iterations"),
    (dict(extract_mesh=True, mesh_smooth_iterations=2.5), "mesh_smooth_iterations"),
    (dict(extract_mesh=True, mesh_smooth_iterations=2, mesh_smooth_lambda=0.0), "mesh_smooth_lambda"),
    (dict(extract_mesh=True, mesh_smooth_iterations=2, mesh_smooth_lambda=1.01), "mesh_smooth_lambda"),
    (dict(extract_mesh=True, mesh_smooth_iterations=2, mesh_smooth_lambda=float("nan")), "mesh_smooth_lambda"),
    (dict(extract_mesh=True, mesh_smooth_iterations=2, mesh_smooth_mu=0.01), "mesh_smooth_mu"),
    (dict(extract_mesh=True, mesh_smooth_iterations=2, mesh_smooth_mu=-2.01), "mesh_smooth_mu"),
    (dict(extract_mesh=True, mesh_smooth_mu=float("nan")), "mesh_smooth_mu"),
])
def test_config_is_checked_before_anything_runs(kw, match):
    """reconstruct() refuses at once: no frame is loaded, so anything later would fail differently"""
    pipe = DepthToReconstructionPipeline(ReconstructionConfig(fx=100.0, fy=100.0, cx=50.0, cy=50.0, **kw))
    with pytest.raises(ValueError, match=match):
        pipe.reconstruct()
    with pytest.raises(ValueError, match=match):
        pipe._check_mesh_filter_config()


def test_valid_config_passes_the_check():
    for kw in (dict(), dict(extract_mesh=True, mesh_smooth_iterations=1000, mesh_smooth_lambda=1.0, mesh_smooth_mu=-2.0, mesh_normals=True),
               dict(extract_mesh=True, mesh_smooth_iterations=1, mesh_smooth_mu=0.0)):
        DepthToReconstructionPipeline(ReconstructionConfig(fx=100.0, fy=100.0, cx=50.0, cy=50.0, **kw))._check_mesh_filter_config()


@pytest.mark.parametrize("extra", [("--mesh-smooth", "3"), ("--mesh-normals",), ("--mesh-smooth", "3", "--mesh-normals")])
def test_cli_flags_need_a_mesh_output(tmp_path, extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "depth_to_reconstruction.py"), "--rgb-folder", str(tmp_path), "--depth-folder",
                        str(tmp_path), "--output", str(tmp_path / "o.ply"), *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--mesh-output" in r.stderr and "--mesh-smooth / --mesh-normals" in r.stderr


def test_cli_help_names_the_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "depth_to_reconstruction.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--mesh-smooth N" in r.stdout and "--mesh-normals" in r.stdout


# ---- the calls' argument checks need no device ----------------------------------------------------------------------------------
def test_calls_are_exported_and_bound():
    lib = abi.load()
    for name, nargs in (("tl3d_mesh_smooth_taubin", 11), ("tl3d_mesh_vertex_normals", 7)):
        assert name in abi.SYMBOLS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs and getattr(lib, name).restype is C.c_int


def test_argument_validation_needs_no_gpu():
    """everything decided before any device call answers TL3D_E_INVALID with a null context too (the null-context check is last)"""
    lib = abi.load()
    xyz, tris = small_shape("one triangle")
    xyz, tris = xyz.copy(), tris.copy()
    out, val, ne = np.zeros_like(xyz), np.zeros(3, np.uint32), C.c_int64(7)
    p = abi.ptr

    def smooth(xyz_p=p(xyz), nv=3, tri_p=p(tris), nt=1, it=1, lam=0.5, mu=-0.53, out_p=p(out), val_p=p(val), ne_p=C.byref(ne)):
        return lib.tl3d_mesh_smooth_taubin(None, xyz_p, nv, tri_p, nt, it, lam, mu, out_p, val_p, ne_p)

    def message():
        return lib.tl3d_last_error().decode()
    cases = [(dict(nv=-1), "negative"), (dict(nt=-1), "negative"), (dict(nv=1 << 31), "2^31"), (dict(nt=1 << 32), "2^32"),
             (dict(tri_p=None), "null"), (dict(xyz_p=None), "null"), (dict(out_p=None), "null"), (dict(ne_p=None), "null"),
             (dict(it=-1), "iterations"), (dict(it=1001), "iterations"), (dict(lam=0.0), "lambda"), (dict(lam=1.0001), "lambda"),
             (dict(lam=float("nan")), "lambda"), (dict(mu=1e-9), "mu"), (dict(mu=-2.0001), "mu"), (dict(mu=float("nan")), "mu"),
             (dict(out_p=p(xyz)), "aliases"), (dict(val_p=p(tris)), "aliases"), (dict(val_p=p(out)), "aliases"),
             (dict(out_p=C.c_void_p(xyz.ctypes.data + 12), nv=2), "aliases"), (dict(), "null ctx")]
    for kw, word in cases:
        assert smooth(**kw) == abi.E_INVALID and word in message(), (kw, message())
    assert ne.value == 7 and not out.any()
    nz = C.c_int64(7)

    def normals(xyz_p=p(xyz), nv=3, tri_p=p(tris), nt=1, out_p=p(out), nz_p=C.byref(nz)):
        return lib.tl3d_mesh_vertex_normals(None, xyz_p, nv, tri_p, nt, out_p, nz_p)
    for kw, word in [(dict(nv=-1), "negative"), (dict(nv=1 << 31), "2^31"), (dict(nt=1 << 32), "2^32"), (dict(tri_p=None), "null"),
                     (dict(xyz_p=None), "null"), (dict(out_p=None), "null"), (dict(nz_p=None), "null"), (dict(out_p=p(xyz)), "aliases"),
                     (dict(out_p=p(tris), nv=1), "aliases"), (dict(), "null ctx")]:
        assert normals(**kw) == abi.E_INVALID and word in message(), (kw, message())
    assert nz.value == 7 and not out.any()
