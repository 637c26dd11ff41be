"""CPU: the beads meshes of the compaction edge tests (tests/compaction_edges_common.py) give, with the component reference and
the simplification reference, the figures the GPU test pins; a generator that drifts is noticed without a GPU."""
from compaction_edges_common import FIGURES, SIZES, figures


def test_beads_figures():
    assert SIZES == (1, 255, 256, 257, 2047, 2048, 2049, 4097)
    for n_tri in SIZES:
        assert figures(n_tri) == FIGURES[n_tri], n_tri
