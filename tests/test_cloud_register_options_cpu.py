"""CPU: the compare_align settings (ReconstructionConfig, both command lines) are checked before any work: what is refused, with what
message, and what the initial matrix may be."""
import numpy as np
import pytest


def test_compare_align_options(tmp_path):
    from tl3d import pipeline
    from tl3d.config import ReconstructionConfig
    cfg = ReconstructionConfig()
    assert cfg.compare_align is False and cfg.compare_align_scale is False and cfg.compare_align_init is None
    assert pipeline.check_compare_options(cfg) is None
    assert pipeline.check_compare_options(ReconstructionConfig(compare_to="scan.ply", compare_align=True, compare_align_scale=True)) is None
    for kw, text in ((dict(compare_align=True), "needs compare_to"), (dict(compare_align_scale=True, compare_to="s.ply"), "need compare_align"),
                     (dict(compare_align_init=np.eye(4), compare_to="s.ply"), "need compare_align"),
                     (dict(compare_align=True, compare_to="s.ply", compare_align_init=np.eye(3)), "4 x 4"),
                     (dict(compare_align=True, compare_to="s.ply", compare_align_init=np.full((4, 4), np.nan)), "4 x 4"),
                     (dict(compare_align=True, compare_to="s.ply", compare_align_init=str(tmp_path / "none.txt")), "cannot read")):
        with pytest.raises(ValueError, match=text):
            pipeline.check_compare_options(ReconstructionConfig(**kw))
        with pytest.raises(ValueError, match=text):                        # before anything is loaded, let alone fused
            pipeline.DepthToReconstructionPipeline(ReconstructionConfig(**kw)).reconstruct()
    T = np.eye(4)
    T[:3, 3] = (0.25, -1.0, 3.5)
    np.save(tmp_path / "init.npy", T)
    np.savetxt(tmp_path / "init.txt", T)
    for init in (T, T.tolist(), str(tmp_path / "init.npy"), tmp_path / "init.txt"):
        got = pipeline.check_compare_options(ReconstructionConfig(compare_to="s.ply", compare_align=True, compare_align_init=init))
        assert got.dtype == np.float64 and np.array_equal(got, T)


def test_both_command_lines_take_the_flags(tmp_path, capsys):
    import depth_enhanced_reconstruction as der
    import depth_to_reconstruction as d2r
    np.savetxt(tmp_path / "init.txt", np.eye(4))
    for cli, args in ((d2r, ["--rgb-folder", "a", "--depth-folder", "b"]), (der, ["--input", "a", "--output", "b"])):
        for extra, text in ((["--compare-align"], "needs compare_to"), (["--compare-align-scale", "--compare-to", "s.ply"], "need compare_align"),
                            (["--compare-align-init", str(tmp_path / "init.txt"), "--compare-to", "s.ply"], "need compare_align"),
                            (["--compare-align", "--compare-to", "s.ply", "--compare-align-init", str(tmp_path / "none.npy")], "cannot read")):
            with pytest.raises(SystemExit):
                cli.main(args + extra)
            assert "--compare-align: " in capsys.readouterr().err
    # accepted: the run then ends for want of input, not in the argument parser
    assert der.main(["--input", str(tmp_path / "none"), "--output", str(tmp_path / "o"), "--compare-to", "s.ply", "--compare-align", "--compare-align-scale",
                     "--compare-align-init", str(tmp_path / "init.txt")]) == 1
    assert "Need at least 2 images" in capsys.readouterr().out


def test_move_points_is_one_rounding():
    from tl3d import metrics
    rng = np.random.default_rng(0)
    p = rng.normal(size=(50, 3)).astype(np.float32)
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = (0.5, 0.25, -2.0)
    got = metrics.move_points(p, T, 2.0)
    want = np.stack([-2.0 * p[:, 1].astype(np.float64) + 0.5, 2.0 * p[:, 0].astype(np.float64) + 0.25, 2.0 * p[:, 2].astype(np.float64) - 2.0], axis=1)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    assert "Align: status 1" in metrics.format_alignment(dict(T=T.tolist(), scale=1.0, fitness=1.0, rmse=0.0, n_corr=5, iters_run=2, status=1))
