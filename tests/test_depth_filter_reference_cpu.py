"""CPU: the two numpy formulations of the depth-frame filter (depth_filter_reference.py) agree on every crafted case and give the
hand-written answers of the smallest ones; the configuration check and both drivers' argument parsers."""
import numpy as np
import pytest

import depth_filter_common as dc
import depth_filter_reference as dr


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(dr.bits(a), dr.bits(b))


@pytest.mark.parametrize("case", dc.hand_cases(), ids=lambda c: c[0])
def test_hand_written_answers(case):
    _name, img, prm, want, want_counts = case
    for fn in (dr.filter_shifted, dr.filter_loops):
        out, counts = fn(img, **prm)
        assert _same(out, want), (fn.__name__, out, want)
        assert counts.tolist() == list(want_counts), (fn.__name__, counts)


def test_formulations_agree_on_every_crafted_case():
    cases = dc.crafted_cases()
    assert len(cases) > 300
    for name, img, prm in cases:
        if img.size > 12000:                    # the loops take seconds on the largest images; the GPU tests use the shifted form there
            continue
        a, ca = dr.filter_shifted(img, **prm)
        b, cb = dr.filter_loops(img, **prm)
        assert _same(a, b), name
        assert ca.tolist() == cb.tolist(), (name, ca, cb)
        # the filter only writes zeros, and only over valid pixels
        changed = dr.bits(a) != dr.bits(img)
        assert not changed[~dr.valid_mask(dr.as_f32(img))].any(), name
        assert (a[changed] == 0).all(), name
        assert ca[0] == int(dr.valid_mask(dr.as_f32(img)).sum()) and int(changed.sum()) == ca[1] + ca[3], name


def test_largest_cases_agree_once():
    name, img, prm = next(c for c in dc.crafted_cases() if c[0] == "noise_f32_big")
    a, ca = dr.filter_shifted(img, **prm)
    b, cb = dr.filter_loops(img, **prm)
    assert _same(a, b) and ca.tolist() == cb.tolist()
    assert ca[1] > 0 and ca[3] > 0 and ca[2] > 1


def test_link_boundaries_straddle_the_decision():
    """the boundary pairs really sit on both sides: per (jump, lo) the `at` pair is linked where the product is exact, `above2` never"""
    res = {}
    for name, img, prm in dc.link_boundary_cases():
        if name.endswith("_a") and name.startswith("link_j"):
            out, counts = dr.filter_shifted(img, **prm)
            res[name] = int(counts[1]) == 0                    # both kept = linked
    assert res["link_j0.0625_lo1_at_lo_hi_a"] and res["link_j0.0625_lo1_at_hi_lo_a"]
    assert not res["link_j0.0625_lo1_above_lo_hi_a"] and not res["link_j0.0625_lo1_above_hi_lo_a"]
    assert res["link_j0.0625_lo1_below_lo_hi_a"]
    assert res["link_j0.25_lo3_at_lo_hi_a"] and not res["link_j0.25_lo3_above_lo_hi_a"]
    for jump, lo in (("0.05", "1"), ("0.05", "2.71828"), ("0.3", "0.001")):
        got = [res[f"link_j{jump}_lo{lo}_{tag}_lo_hi_a"] for tag in ("below", "at", "above", "above2")]
        assert got[0] and not got[3], (jump, lo, got)          # linked below, apart two ulps above
        assert got == sorted(got, reverse=True)                # one switch
        assert got == [res[f"link_j{jump}_lo{lo}_{tag}_hi_lo_a"] for tag in ("below", "at", "above", "above2")]


def test_crafted_topologies_do_what_they_are_for():
    by_name = {c[0]: c for c in dc.crafted_cases()}

    def run(name):
        _n, img, prm = by_name[name]
        return (img,) + dr.filter_shifted(img, **prm)
    img, out, c = run("cut_f32_no_a")                    # one region of 39 stays
    assert c.tolist() == [39, 0, 1, 0] and _same(out, img)
    img, out, c = run("cut_f32_a")                       # stage A cuts it, stage B removes the halves
    assert c.tolist() == [39, 1, 2, 38] and not out.any()
    img, out, c = run("spiral_f32_keep")                 # one long path
    assert c[2] == 1 and c[1] == 0 and c[3] == 0 and c[0] > 2000
    img, out, c = run("spiral_f32_drop")
    assert c[2] == 1 and c[3] == c[0] and not out.any()
    img, out, c = run("comb_f32_keep")                   # teeth join in the last row: one region
    assert c[2] == 1 and c[3] == 0 and c[0] == 75 * 50 + 75
    img, out, c = run("comb_f32_drop")
    assert c[3] == c[0]
    img, out, c = run("slope_comb_keep")                 # one region although its ends are far apart in depth
    assert c[2] == 1 and c[3] == 0 and float(img.max()) > 2.0 * float(img[img > 0].min())
    img, out, c = run("checker_f32_b")                   # every square is a region of its own
    assert c[2] == c[0] - c[1] and c[3] == c[2]
    img, out, c = run("blobs_f32_7")                     # exactly min_region stays, min_region - 1 goes
    assert c.tolist() == [3 * 7 + 3 * 6, 0, 6, 18]
    for r in (1, 2, 3):                                  # the seam pairs support each other at their radius only
        img, out, c = run(f"seams_f32_r{r}")
        assert c[0] >= 20 and c[1] == 0
        if r > 1:
            _o, c1 = dr.filter_shifted(img, **dict(by_name[f"seams_f32_r{r}"][2], radius=r - 1))
            assert c1[1] == c1[0]
        n = (2 * r + 1) ** 2
        for ms in (0, 1, n - 1):                         # the ladder: centre k has exactly k supporters
            img, out, c = run(f"ladder_f32_r{r}_s{ms}")
            pitch, win = 2 * (2 * r + 1) + 1, 2 * r + 1
            kept = [bool(out[(k // 6) * pitch + win, (k % 6) * pitch + win]) for k in range(n)]
            assert kept == [k >= ms for k in range(n)], (r, ms, kept)


def test_config_defaults_and_checks(capsys):
    from tl3d import pipeline
    from tl3d.config import ReconstructionConfig
    cfg = ReconstructionConfig()
    assert cfg.depth_filter is False and cfg.depth_filter_jump == 0.05 and cfg.depth_filter_radius == 1
    assert cfg.depth_filter_min_support == 4 and cfg.depth_filter_min_region == 0
    pipeline.check_depth_filter_options(cfg)
    pipeline.check_depth_filter_options(ReconstructionConfig(depth_filter_radius=9))               # off: nothing is checked
    pipeline.check_depth_filter_options(ReconstructionConfig(depth_filter=True, depth_filter_radius=3, depth_filter_min_support=48))
    assert pipeline.depth_filter_parameters(ReconstructionConfig(depth_filter=True, depth_filter_min_region=50)) == dict(
        jump_rel=0.05, radius=1, min_support=4, min_region=50)
    for kw, text in ((dict(depth_filter_jump=0.0), "depth_filter_jump"), (dict(depth_filter_jump=float("nan")), "depth_filter_jump"),
                     (dict(depth_filter_jump=float("inf")), "depth_filter_jump"), (dict(depth_filter_radius=0), "depth_filter_radius"),
                     (dict(depth_filter_radius=4), "depth_filter_radius"), (dict(depth_filter_radius=1.5), "depth_filter_radius"),
                     (dict(depth_filter_min_support=9), "depth_filter_min_support"), (dict(depth_filter_min_support=-1), "depth_filter_min_support"),
                     (dict(depth_filter_radius=2, depth_filter_min_support=25), "depth_filter_min_support"),
                     (dict(depth_filter_min_region=-1), "depth_filter_min_region")):
        with pytest.raises(ValueError, match=text):
            pipeline.check_depth_filter_options(ReconstructionConfig(depth_filter=True, **kw))
        with pytest.raises(ValueError, match=text):                        # before anything is loaded, let alone fused
            pipeline.DepthToReconstructionPipeline(ReconstructionConfig(depth_filter=True, **kw)).reconstruct()
    import depth_enhanced_reconstruction as der
    import depth_to_reconstruction as d2r
    for cli, args in ((d2r, ["--rgb-folder", "a", "--depth-folder", "b"]), (der, ["--input", "a", "--output", "b"])):
        for extra, text in ((["--depth-filter-radius", "4"], "depth_filter_radius"), (["--depth-filter-jump", "0"], "depth_filter_jump"),
                            (["--depth-filter-min-support", "9"], "depth_filter_min_support"),
                            (["--depth-filter-min-region", "-2"], "depth_filter_min_region")):
            with pytest.raises(SystemExit):
                cli.main(args + ["--depth-filter"] + extra)
            assert "--depth-filter: " + text in capsys.readouterr().err
    with pytest.raises(SystemExit):                                        # refused before any process is started
        d2r.main(["--rgb-folder", "a", "--depth-folder", "b", "--gpus", "2", "--depth-filter"])
    assert "--depth-filter needs a single GPU" in capsys.readouterr().err


def test_sharded_run_refuses_the_filter():
    from tl3d import pipeline
    from tl3d.config import ReconstructionConfig
    p = pipeline.DepthToReconstructionPipeline(ReconstructionConfig(depth_filter=True))
    with pytest.raises(ValueError, match="depth_filter needs a single GPU"):
        p.reconstruct_sharded(None)
