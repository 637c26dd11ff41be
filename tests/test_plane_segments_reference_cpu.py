"""CPU: the two formulations of tests/plane_segments_reference.py agree with each other and with known answers on the crafted clouds
of tests/plane_segments_common.py (what the GPU tests of tl3d_segment_planes are held to); the PLY writers' `plane` property; the
configuration checks of cloud_planes."""
import numpy as np
import pytest

import plane_segments_common as pc
import plane_segments_reference as pr
from tl3d import fileio

QSTEP = 2.0 ** -20      # the tree formulation fits the quantised coordinates, the growing one the f32 coordinates themselves


def _agree(a, b, what):
    assert a.counts == b.counts and np.array_equal(a.plane_id, b.plane_id), what
    assert np.array_equal(a.planes["count"], b.planes["count"]) and np.array_equal(a.planes["seed"], b.planes["seed"]), what
    for x, y in zip(a.planes, b.planes):
        assert abs(x["rms"] - y["rms"]) <= QSTEP and np.all(np.abs(x["centroid"] - y["centroid"]) <= QSTEP), what


@pytest.mark.parametrize("noise_mm", [0.0, 1.0])
def test_box_corner_known_answer(noise_mm):
    a = pc.box_reference(noise_mm)
    b = pr.segment_grow(*pc.box_corner(noise_mm), pc.BOX_PARAMS)
    _agree(a, b, f"box corner, noise {noise_mm} mm")
    assert a.counts[2:] == (5, 4)
    parts = pc.BOX_PARTS
    for k, name in enumerate(("face_z", "face_x", "face_y", "step")):          # ascending seed = the order the parts were laid down in
        lo, hi = parts[name]
        ids = a.plane_id[lo:hi]
        assert set(np.unique(ids)) <= {-1, k} and (ids == k).sum() >= (1300 if k < 3 else 150), name
        axis = dict(face_z=2, face_x=0, face_y=1, step=2)[name]
        assert a.planes["normal"][k][axis] > 0.999 and a.planes["rms"][k] <= pc.BOX_PARAMS.max_rms
        assert abs(a.planes["d"][k] - (0.02 if name == "step" else 0.0)) < 1e-3
    lo, hi = parts["cylinder"]
    assert np.all(a.plane_id[lo:hi] == -1) and len(np.unique(a.label[lo:hi])) == 1      # one region, rejected by max_rms


@pytest.mark.parametrize("name", pc.EDGES)
def test_decision_edges_known_answers(name):
    p, n, c, prm, want = pc.EDGE_CASES[name]
    a, b = pr.segment_tree(p, n, c, prm), pr.segment_grow(p, n, c, prm)
    _agree(a, b, name)
    assert a.counts == want


def test_signed_and_unsigned():
    p, n = pc.two_sheets()
    for signed, planes in ((True, 2), (False, 1)):
        prm = pc.SHEET_PARAMS.replace(signed_normals=signed)
        a, b = pr.segment_tree(p, n, None, prm), pr.segment_grow(p, n, None, prm)
        _agree(a, b, f"signed {signed}")
        assert a.counts == (780, planes, planes, planes)
        assert [float(np.sign(z)) for z in a.planes["normal"][:, 2]] == ([1.0, -1.0] if signed else [1.0])


@pytest.mark.parametrize("name", ["strip ascending", "strip descending", "strip permuted", "4096 strips interleaved"])
def test_topology_answers(name):
    strips = 128
    p, n = pc.topology(name, strips)
    want_id, want_counts, want_planes = pc.topology_answer(name, strips)
    a = pr.segment_tree(p, n, None, pc.TOPO_PARAMS)
    assert a.counts == want_counts and np.array_equal(a.plane_id, want_id)
    assert list(zip(a.planes["count"].tolist(), a.planes["seed"].tolist())) == want_planes


def test_hub_is_one_clique():
    p, _ = pc.topology("hub")
    ext = p.max(axis=0).astype(np.float64) - p.min(axis=0)
    assert float((ext * ext).sum()) <= pc.TOPO_PARAMS.radius ** 2 and np.all(p[:, 2] == 0)     # every pair within the radius, offsets 0


def test_integer_sums_and_the_extended_plane():
    p, n, c = pc.box_corner(1.0)
    a = pc.box_reference(1.0)
    assert pc.check_planes(a.planes, a, p, "tree formulation against the extended-precision plane") <= 1.0
    members = np.flatnonzero(a.plane_id == 0)
    cnt, se, see, sn = pr.integer_sums(p, n, members, int(members.min()))
    q = pr.quantise(p).astype(object)
    e = q[members] - q[members.min()]
    assert cnt == len(members) and se == [sum(e[:, k]) for k in range(3)] and see[3] == sum(e[:, 0] * e[:, 1])


# ---- the writers --------------------------------------------------------------------------------------------------------------------
def _cloud(m=7):
    rng = np.random.default_rng(1)
    return (rng.random((m, 3)).astype(np.float32), rng.integers(0, 255, (m, 3)).astype(np.uint8), rng.random((m, 3)).astype(np.float32),
            rng.random(m).astype(np.float32), np.arange(m, dtype=np.int32) - 2)


def test_ply_writers_plane_property(tmp_path):
    xyz, rgb, nrm, curv, planes = _cloud()
    for writer, name in ((fileio.write_ply_ascii, "a"), (fileio.write_ply_binary, "b")):
        old, new, bare = (str(tmp_path / f"{name}{k}.ply") for k in range(3))
        writer(old, xyz, rgb, normals=nrm, curvature=curv)
        writer(new, xyz, rgb, normals=nrm, curvature=curv, planes=planes)
        writer(bare, xyz, rgb, normals=nrm, curvature=curv, planes=None)
        assert open(old, "rb").read() == open(bare, "rb").read()                   # without it every byte is as ever
        head = open(new, "rb").read().split(b"end_header\n")[0].decode().splitlines()
        props = [l for l in head if l.startswith("property")]
        assert props[-1] == "property int plane" and props[-2] == "property float curvature"
        assert [l for l in head if not l.startswith("property int plane")] == open(old, "rb").read().split(b"end_header\n")[0].decode().splitlines()
        body = open(new, "rb").read().split(b"end_header\n", 1)[1]
        if writer is fileio.write_ply_ascii:
            assert [int(l.split()[-1]) for l in body.decode().splitlines()] == planes.tolist()
        else:
            stride = len(body) // len(xyz)
            assert stride * len(xyz) == len(body)
            got = np.frombuffer(body, np.uint8).reshape(len(xyz), stride)[:, -4:].copy().view("<i4").reshape(-1)
            assert got.tolist() == planes.tolist()
    # without normals too
    fileio.write_ply_ascii(str(tmp_path / "c.ply"), xyz, rgb, planes=planes)
    assert b"property int plane\nend_header" in open(tmp_path / "c.ply", "rb").read()


# ---- the configuration, the command lines ------------------------------------------------------------------------------------------
def test_config_defaults_and_checks(capsys):
    from tl3d import pipeline
    from tl3d.config import ReconstructionConfig
    cfg = ReconstructionConfig()
    assert cfg.cloud_planes is False and cfg.cloud_planes_radius == 0.0 and cfg.cloud_planes_angle_deg == 10.0
    assert cfg.cloud_planes_offset == 0.0 and cfg.cloud_planes_max_curvature == 0.05 and cfg.cloud_planes_min_points == 200
    assert cfg.cloud_planes_max_rms == 0.0
    p = pipeline.DepthToReconstructionPipeline(cfg)
    assert p.cloud_plane_ids is None and p.cloud_planes is None
    for kw, text in ((dict(cloud_planes=True), "needs cloud_normals"),
                     (dict(cloud_planes=True, cloud_normals=True, cloud_planes_min_points=2), "cloud_planes_min_points"),
                     (dict(cloud_planes=True, cloud_normals=True, cloud_planes_angle_deg=91.0), "cloud_planes_angle_deg"),
                     (dict(cloud_planes=True, cloud_normals=True, cloud_planes_radius=-1.0), "cloud_planes_radius"),
                     (dict(cloud_planes=True, cloud_normals=True, cloud_planes_max_rms=float("nan")), "cloud_planes_max_rms")):
        with pytest.raises(ValueError, match=text):                        # before anything is loaded, let alone fused
            pipeline.DepthToReconstructionPipeline(ReconstructionConfig(**kw)).reconstruct()
    on = dict(cloud_planes=True, cloud_normals=True, voxel_size=0.004)
    prm = pipeline.cloud_plane_parameters(ReconstructionConfig(**on))
    assert prm == dict(radius=0.01, max_angle_deg=10.0, max_offset=0.004, max_curvature=0.05, min_points=200, max_rms=0.002)
    prm = pipeline.cloud_plane_parameters(ReconstructionConfig(cloud_planes_radius=0.02, cloud_planes_offset=0.001, cloud_planes_max_rms=0.003, **on))
    assert (prm["radius"], prm["max_offset"], prm["max_rms"]) == (0.02, 0.001, 0.003)
    import depth_enhanced_reconstruction as der
    import depth_to_reconstruction as d2r
    for cli, args in ((d2r, ["--rgb-folder", "a", "--depth-folder", "b"]), (der, ["--input", "a", "--output", "b"])):
        for extra in (["--cloud-planes"], ["--cloud-planes-report", "x.json"], ["--cloud-normals", "--cloud-planes-report", "x.json"]):
            with pytest.raises(SystemExit):
                cli.main(args + extra)
            assert "--cloud-planes segments the cloud by its normals: it needs --cloud-normals" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            cli.main(args + ["--cloud-normals", "--cloud-planes", "--cloud-planes-min-points", "2"])
        assert "--cloud-planes-min-points must be 3 at the least" in capsys.readouterr().err


def test_plane_report(tmp_path):
    import json
    planes = pc.box_reference(0.0).planes
    fileio.write_plane_report(tmp_path / "sub" / "planes.json", planes)
    rows = json.load(open(tmp_path / "sub" / "planes.json"))["planes"]
    assert len(rows) == 4 and set(rows[0]) == {"normal", "d", "centroid", "rms", "count"}
    assert [r["count"] for r in rows] == planes["count"].tolist() and rows[3]["normal"] == planes["normal"][3].tolist()
