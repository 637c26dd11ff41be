"""The batches of tests/update_trip_counts_common.py take every path of the update kernel's pair loop -- shown without a GPU, from
the prep chain's numpy model alone (prep_classes_reference.classify_frame): the number of MIXED sub-bricks m of every brick gives
its pair count P = n m when the frame is fused n times, and over the batches P takes every value the loop's shape can tell apart.
If an image stops giving this coverage, change the image, not the assertions."""
import numpy as np

import update_trip_counts_common as tc


def test_images_are_whole_millimetres_with_holes():
    for name in tc.IMAGES:
        mm = tc.image_mm(name)
        assert mm.shape == (tc.H, tc.W) and mm.dtype == np.uint16
        assert np.array_equal(np.rint(tc.image_f32(name).astype(np.float64) * 1000.0), mm)
    assert (tc.image_mm("step")[:3] == 0).all() and tc.image_mm("plane").min() > 0


def test_bricks_with_one_to_eight_mixed_sub_bricks_occur():
    seen = {m for name in tc.IMAGES for m, _ in tc.mixed_per_brick(name).values()}
    assert seen >= set(range(1, 9)), sorted(seen)


def test_a_brick_without_pairs_whose_only_contribution_is_free_sub_bricks():
    assert any(m == 0 and free > 0 for name in tc.IMAGES for m, free in tc.mixed_per_brick(name).values())


def test_pair_counts_take_every_path_of_the_loop():
    counts = {p for ps in tc.pair_counts().values() for p in ps}
    for unroll in tc.UNROLLS:
        for r in range(unroll):
            assert any(p % unroll == r and p < unroll for p in counts), (unroll, r, "below one loop body")
            assert any(p % unroll == r and p >= unroll for p in counts), (unroll, r, "with whole loop bodies")
    assert {1, 2, 3} <= counts                                    # at or below the depth of the pipeline
    assert tc.PIPE_DEPTH == 3
    assert any(p >= 12 for p in counts)                           # two whole bodies and more
    assert max(counts) <= 256                                     # what a batch of 32 frames can hold: the kernel's division by 6


def test_one_batch_holds_many_paths_at_once():
    """every batch mixes bricks of different P mod 6, so a wave meets different paths brick after brick"""
    for (name, n), ps in tc.pair_counts().items():
        if n % 6:
            assert len({p % 6 for p in ps}) >= 2, (name, n)
