"""CPU: the compare_align_global settings (ReconstructionConfig, both command lines) are checked before any work: what is refused and
with what message."""
import numpy as np
import pytest


def test_compare_align_global_options(tmp_path):
    from tl3d import pipeline
    from tl3d.config import ReconstructionConfig
    cfg = ReconstructionConfig()
    assert cfg.compare_align_global is False and cfg.compare_align_global_voxel is None
    assert pipeline.check_compare_options(cfg) is None
    ok = dict(compare_to="scan.ply", compare_align=True, compare_align_global=True)
    assert pipeline.check_compare_options(ReconstructionConfig(**ok)) is None
    assert pipeline.check_compare_options(ReconstructionConfig(compare_align_global_voxel=0.04, **ok)) is None
    for kw, text in ((dict(compare_align_global=True, compare_to="s.ply"), "need compare_align"),
                     (dict(compare_align_global_voxel=0.05, compare_to="s.ply"), "need compare_align"),
                     (dict(compare_align=True, compare_to="s.ply", compare_align_global_voxel=0.05), "needs compare_align_global"),
                     (dict(ok, compare_align_init=np.eye(4)), "cannot be combined with compare_align_init"),
                     (dict(ok, compare_align_scale=True), "rigid only.*compare_align_scale"),
                     (dict(ok, compare_align_global_voxel=0.0), "finite and positive"),
                     (dict(ok, compare_align_global_voxel=float("nan")), "finite and positive"),
                     (dict(compare_align=True, compare_align_global=True), "needs compare_to")):
        with pytest.raises(ValueError, match=text):
            pipeline.check_compare_options(ReconstructionConfig(**kw))
        with pytest.raises(ValueError, match=text):                        # before anything is loaded, let alone fused
            pipeline.DepthToReconstructionPipeline(ReconstructionConfig(**kw)).reconstruct()


def test_both_command_lines_take_the_flags(tmp_path, capsys):
    import depth_enhanced_reconstruction as der
    import depth_to_reconstruction as d2r
    np.savetxt(tmp_path / "init.txt", np.eye(4))
    for cli, args in ((d2r, ["--rgb-folder", "a", "--depth-folder", "b"]), (der, ["--input", "a", "--output", "b"])):
        for extra, text in ((["--compare-align-global", "--compare-to", "s.ply"], "need compare_align"),
                            (["--compare-align-global-voxel", "0.05", "--compare-to", "s.ply", "--compare-align"], "needs compare_align_global"),
                            (["--compare-align", "--compare-align-global"], "needs compare_to"),
                            (["--compare-align", "--compare-align-global", "--compare-to", "s.ply", "--compare-align-scale"], "rigid only"),
                            (["--compare-align", "--compare-align-global", "--compare-to", "s.ply", "--compare-align-init", str(tmp_path / "init.txt")],
                             "cannot be combined with compare_align_init"),
                            (["--compare-align", "--compare-align-global", "--compare-to", "s.ply", "--compare-align-global-voxel", "-1"],
                             "finite and positive")):
            with pytest.raises(SystemExit):
                cli.main(args + extra)
            err = capsys.readouterr().err
            assert "--compare-align: " in err and text in err
    # accepted: the run then ends for want of input, not in the argument parser
    assert der.main(["--input", str(tmp_path / "none"), "--output", str(tmp_path / "o"), "--compare-to", "s.ply", "--compare-align",
                     "--compare-align-global", "--compare-align-global-voxel", "0.04"]) == 1
    assert "Need at least 2 images" in capsys.readouterr().out


def test_the_align_line_names_the_global_start():
    from tl3d import metrics
    al = dict(T=np.eye(4).tolist(), scale=1.0, fitness=1.0, rmse=0.0, n_corr=5, iters_run=2, status=1)
    assert metrics.format_alignment(al).startswith("Align: status 1")
    al["global"] = dict(T=np.eye(4).tolist(), inliers=57, n_corr=603, n_passed=665, hypotheses=100000, voxel=0.03, mutual=True)
    line = metrics.format_alignment(al)
    assert line.startswith("Align: global start (57 of 603 feature pairs, 665 of 100000 samples scored), status 1")
