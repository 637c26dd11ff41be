"""CPU: the two fp64 references of the cloud normals (tests/cloud_normals_common.py) against each other and against known answers,
the facts the GPU tests rest on (no ties at the k-th distance and no excluded point in the random cases, the degenerate counts, the
margin of the orientation cases), the PLY writers with normals and curvature, read_ply_points on those files, and the refusals of
the configuration and the command lines."""
import numpy as np
import pytest

import cloud_normals_common as cn
from tl3d import fileio
from tl3d import pipeline as pl
from tl3d.config import ReconstructionConfig


# ---- the references against each other ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", cn.RANDOM_K, ids=cn.case_id)
def test_random_cases_have_no_ties_and_no_excluded_points_and_the_references_agree(name, k):
    p = cn.points(name)
    r = cn.case_ref(name, k)
    idx, d2 = cn.case_neighbours(name)
    kk = min(k, len(p))
    if kk < d2.shape[1]:
        assert np.all(d2[:, kk - 1] < d2[:, kk]), "a tie at the k-th distance: the tree may pick another member than the tie rule"
    assert not r.degenerate.any() and not cn.excluded(r).any()
    gap = ((r.lam[:, 1] - r.lam[:, 0]) / r.lam[:, 2]).min()
    print(f"{name} k={k}: smallest (l1 - l0) / l2 = {gap:.3g}, largest bound {cn.angle_bound(r.lam).max():.3g}")
    b = cn.brute(p, k, neighbours=(idx, d2))
    assert np.array_equal(b.members, r.members) and np.all(r.members == kk)
    cn.check(b.normals, b.curvature, r, False, f"brute against ref, {name} k={k}")


def test_summing_in_reverse_order_stays_far_inside_the_bar():
    """what the bar allows for (another association of the same sums) measured on the largest random case"""
    p = cn.points("ring").astype(np.float64)
    idx, _ = cn.case_neighbours("ring")
    r = cn.case_ref("ring", 30)
    e = p[idx[:, :30][:, ::-1]] - p[:, None, :]
    d = e - e.mean(axis=1, keepdims=True)
    _, vec = np.linalg.eigh(np.einsum("nki,nkj->nij", d, d))
    s = cn.sin_angle(vec[:, :, 0], r.normals)
    assert np.all(s <= 16 * 2.0 ** -52 * r.lam[:, 2] / (r.lam[:, 1] - r.lam[:, 0]))


# ---- known answers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", [cn.ref, cn.brute], ids=["ref", "brute"])
def test_degenerate_neighbourhoods(fn):
    for name in ("tiny_n1", "tiny_n2", "same"):
        r = fn(cn.points(name), 20)
        assert r.degenerate.all() and not r.normals.any() and not r.curvature.any()
    p = cn.points("dups")
    for k in (3, 4):
        r = fn(p, k)
        assert int(r.degenerate.sum()) == 35 and r.degenerate[3000:].all() and r.degenerate[:2].all()      # the 25 + 10 copies
    assert not fn(p, 30).degenerate.any()


@pytest.mark.parametrize("fn", [cn.ref, cn.brute], ids=["ref", "brute"])
def test_plane_lattice_is_exact(fn):
    r = fn(cn.points("plane_lattice"), 9)
    assert not r.degenerate.any()
    assert np.all(r.normals[:, :2] == 0) and np.all(np.abs(r.normals[:, 2]) == 1)
    assert np.all(np.abs(r.curvature) <= 1e-15)


def test_line_and_isotropic_lattice():
    r = cn.ref(cn.points("line"), 20)
    assert not r.degenerate.any() and np.all(np.abs(r.normals[:, 0]) <= cn.F32)
    assert np.all(np.abs(np.linalg.norm(r.normals, axis=1) - 1) <= 1e-12)
    r = cn.ref(cn.points("lattice"), 7)
    assert not r.degenerate.any()
    inside = cn.sc.lattice_interior()
    assert np.all(r.lam[inside, 1] - r.lam[inside, 0] <= 1e-12) and cn.excluded(r)[inside].all()        # gap 0: no direction to check


def test_the_tie_rule_decides_the_four_point_case():
    z, y, x = [0, 0, 1], [0, 1, 0], [1, 0, 0]
    b = cn.brute(cn.points("tie4"), 3)
    assert np.array_equal(np.abs(b.normals), np.float64([z, z, z, y]))
    rev = cn.brute(cn.points("tie4_reversed"), 3)
    assert np.array_equal(np.abs(rev.normals), np.float64([x, x, y, x]))
    assert not np.array_equal(np.abs(rev.normals)[::-1], np.abs(b.normals))                              # the same points, another order


@pytest.mark.parametrize("fn", [cn.ref, cn.brute], ids=["ref", "brute"])
def test_radius_keeps_points_on_it(fn):
    r = fn(cn.points("radius6"), 8, max_radius=0.5)
    assert r.members.tolist() == [5, 2, 2, 2, 2, 1] and r.degenerate[5] and not r.degenerate[0]
    assert np.array_equal(np.abs(r.normals[0]), [0, 0, 1])
    assert int(r.degenerate.sum()) == 5                                    # the four rim points see only the origin besides themselves
    r = fn(cn.points("radius6"), 8, max_radius=0.4999)
    assert r.members.tolist() == [1] * 6 and r.degenerate.all()


def test_orientation_cases_have_a_margin():
    p = cn.points("ring").astype(np.float64)
    for vp in (cn.ring_viewpoints(), np.zeros((1, 3))):
        r = cn.ref(p, 30, viewpoints=vp)
        d = vp[None, :, :] - p[:, None, :]
        to = d[np.arange(len(p)), (d * d).sum(axis=-1).argmin(axis=1)]
        dots = (r.normals * to).sum(axis=1)
        assert np.all(np.abs(dots) > 1e-9 * np.linalg.norm(to, axis=1)) and np.all(dots > 0)
    # two identical viewpoints and a third: the smaller index wins, so the result is that of the first two alone
    vp = np.float64([[2, 0, 0], [2, 0, 0], [-2, 0, 0]])
    assert np.array_equal(cn.ref(p, 30, viewpoints=vp).normals, cn.ref(p, 30, viewpoints=vp[[0, 2]]).normals)


# ---- files ---------------------------------------------------------------------------------------------------------------------------
def _cloud(n=61, seed=0):
    r = np.random.default_rng(seed)
    nrm = r.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return ((r.normal(size=(n, 3)) * 3).astype(np.float32), r.integers(0, 256, (n, 3)).astype(np.uint8), nrm.astype(np.float32),
            r.uniform(0, 1 / 3, n).astype(np.float32))


def _header(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:end].decode("ascii").splitlines(), data[end:]


def _props(header):
    return [ln.split()[1:] for ln in header if ln.startswith("property")]


def test_writers_without_attributes_write_the_same_bytes(tmp_path):
    xyz, rgb, _, _ = _cloud()
    fileio.write_ply_binary(tmp_path / "a.ply", xyz.astype(np.float64), rgb)
    fileio.write_ply_binary(tmp_path / "b.ply", xyz.astype(np.float64), rgb, normals=None, curvature=None)
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes()
    head, body = _header(tmp_path / "a.ply")
    assert _props(head) == [["double", "x"], ["double", "y"], ["double", "z"], ["uchar", "red"], ["uchar", "green"], ["uchar", "blue"]]
    assert len(body) == len(xyz) * 27
    fileio.write_ply_ascii(tmp_path / "c.ply", xyz, rgb)
    want = ("ply\nformat ascii 1.0\n" + f"element vertex {len(xyz)}\n" + "property float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
            + "".join(f"{p[0]} {p[1]} {p[2]} {int(c[0])} {int(c[1])} {int(c[2])}\n" for p, c in zip(xyz, rgb)))
    assert (tmp_path / "c.ply").read_text() == want


@pytest.mark.parametrize("double_xyz", [True, False])
@pytest.mark.parametrize("with_curvature", [False, True])
def test_binary_writer_with_normals(tmp_path, double_xyz, with_curvature):
    xyz, rgb, nrm, cur = _cloud(seed=1)
    path = tmp_path / "n.ply"
    fileio.write_ply_binary(path, xyz.astype(np.float64) if double_xyz else xyz, rgb, double_xyz=double_xyz, normals=nrm,
                            curvature=cur if with_curvature else None)
    t = "double" if double_xyz else "float"
    head, body = _header(path)
    assert _props(head) == ([[t, a] for a in ("x", "y", "z", "nx", "ny", "nz")] + [["uchar", a] for a in ("red", "green", "blue")]
                            + ([["float", "curvature"]] if with_curvature else []))
    ft = "<f8" if double_xyz else "<f4"
    rec = np.frombuffer(body, dtype=[(a, ft) for a in ("x", "y", "z", "nx", "ny", "nz")] + [(a, "u1") for a in "rgb"]
                        + ([("c", "<f4")] if with_curvature else []))
    assert len(rec) == len(xyz)
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32), xyz)
    assert np.array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], 1).astype(np.float32), nrm)
    assert np.array_equal(np.stack([rec["r"], rec["g"], rec["b"]], 1), rgb)
    assert not with_curvature or np.array_equal(rec["c"], cur)
    assert np.array_equal(fileio.read_ply_points(path), xyz)               # the reader skips what it does not know


@pytest.mark.parametrize("with_curvature", [False, True])
def test_ascii_writer_with_normals(tmp_path, with_curvature):
    xyz, rgb, nrm, cur = _cloud(seed=2)
    path = tmp_path / "n.ply"
    fileio.write_ply_ascii(path, xyz, rgb, normals=nrm, curvature=cur if with_curvature else None)
    head, body = _header(path)
    assert _props(head) == ([["float", a] for a in ("x", "y", "z", "nx", "ny", "nz")] + [["uchar", a] for a in ("red", "green", "blue")]
                            + ([["float", "curvature"]] if with_curvature else []))
    tab = np.array([ln.split() for ln in body.decode("ascii").splitlines()])
    assert tab.shape == (len(xyz), 10 if with_curvature else 9)
    assert np.array_equal(tab[:, :3].astype(np.float32), xyz) and np.array_equal(tab[:, 3:6].astype(np.float32), nrm)
    assert np.array_equal(tab[:, 6:9].astype(np.int64), rgb)
    assert not with_curvature or np.array_equal(tab[:, 9].astype(np.float32), cur)
    assert np.array_equal(fileio.read_ply_points(path), xyz)


def test_save_reconstruction_passes_the_attributes_on(tmp_path):
    xyz, rgb, nrm, cur = _cloud(seed=3)
    for ascii in (False, True):
        a, b = tmp_path / f"a{ascii}.ply", tmp_path / f"b{ascii}.ply"
        assert fileio.save_reconstruction(xyz.astype(np.float64), rgb, a, ascii=ascii, normals=nrm, curvature=cur)
        (fileio.write_ply_ascii if ascii else fileio.write_ply_binary)(b, xyz.astype(np.float64), rgb, normals=nrm, curvature=cur)
        assert a.read_bytes() == b.read_bytes()
        pl.DepthToReconstructionPipeline().save_reconstruction(xyz.astype(np.float64), rgb, str(tmp_path / "c.ply"), ascii=ascii,
                                                              normals=nrm, curvature=cur)
        assert (tmp_path / "c.ply").read_bytes() == a.read_bytes()
    with pytest.raises(AssertionError):
        fileio.write_ply_binary(tmp_path / "x.ply", xyz, rgb, normals=nrm[:-1])


# ---- configuration, command lines ----------------------------------------------------------------------------------------------------
def test_config_defaults_and_refusals(capsys):
    cfg = ReconstructionConfig()
    assert (cfg.cloud_normals, cfg.cloud_normals_neighbors, cfg.cloud_normals_radius, cfg.cloud_curvature) == (False, 30, 0.0, False)
    p = pl.DepthToReconstructionPipeline(cfg)
    assert p.cloud_normals is None and p.cloud_curvature is None
    for kw, text in ((dict(cloud_curvature=True), "needs cloud_normals"),
                     (dict(cloud_normals=True, cloud_normals_neighbors=2), r"\[3, 64\]"),
                     (dict(cloud_normals=True, cloud_normals_neighbors=65), r"\[3, 64\]"),
                     (dict(cloud_normals=True, cloud_normals_radius=-1.0), "cloud_normals_radius"),
                     (dict(cloud_normals=True, cloud_normals_radius=float("nan")), "cloud_normals_radius")):
        with pytest.raises(ValueError, match=text):                        # before anything is loaded, let alone fused
            pl.DepthToReconstructionPipeline(ReconstructionConfig(**kw)).reconstruct()
    import depth_enhanced_reconstruction as der
    import depth_to_reconstruction as d2r
    for cli, args in ((d2r, ["--rgb-folder", "a", "--depth-folder", "b"]), (der, ["--input", "a", "--output", "b"])):
        with pytest.raises(SystemExit):
            cli.main(args + ["--cloud-curvature"])
        assert "--cloud-curvature comes out of the normal estimation: it needs --cloud-normals" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            cli.main(args + ["--cloud-normals", "--cloud-normals-neighbors", "2"])
        assert "--cloud-normals-neighbors must lie in [3, 64]" in capsys.readouterr().err
