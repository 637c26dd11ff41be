"""CPU: bench.py's command line -- a plain run measures the headline only; --full and --dump-outputs are opt-in."""
import sys

import bench  # stdlib only at import: nothing touches a GPU


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_command_line_defaults(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "5", "--warmup", "2")
    assert a.gpus == 1 and a.steps == 5 and a.warmup == 2
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_outputs(monkeypatch, tmp_path):
    a = _parse(monkeypatch, "--full", "--dump-outputs", str(tmp_path), "--no-rows")
    assert a.full is True and a.dump_outputs == str(tmp_path) and a.no_rows is True
