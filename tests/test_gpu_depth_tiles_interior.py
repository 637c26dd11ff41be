"""The depth-tiles kernel takes a wave-uniform path for 32x32-pixel regions that lie wholly inside the image (no per-pixel
in-image tests) and the general path for the last region column and row of a ragged image.  Both must give the pyramid the
per-voxel rule relies on: the grid stays the oracle's bit for bit."""
import numpy as np
import pytest

import tl3d
from helpers import make_pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["f32", "u16"])
@pytest.mark.parametrize("wh", [(256, 192), (260, 200), (128, 36), (32, 32)])
def test_whole_and_partial_regions_give_the_oracle_grid(kind, wh):
    """Widths that are multiples of 4 (the row-vector loads): all regions whole (256 x 192, 32 x 32), whole regions beside a
    partial last column and row (260 x 200), a partial last row only (128 x 36).  Scattered holes, out-of-range depths and one
    whole region with no valid pixel; several frames per launch."""
    from tl3d import synth
    w, h = wh
    scene = synth.object_scene(with_room=True)
    rng = np.random.default_rng(w * 1000 + h)
    cam = dict(width=w, height=h, fx=0.9 * w, fy=0.9 * w, cx=0.5 * w - 0.5, cy=0.5 * h - 0.5)
    poses = synth.orbit_poses(5, 1.0, 7.0)
    frames = [synth.render(scene, p, **cam) for p in poses]
    ctx, orc = make_pair(cam=cam, dims=(96, 96, 96), voxel=0.03, centre=(0.0, -0.1, 0.0), n_slots=5, channels=tl3d.CH_TSDF)
    with ctx:
        for i, ((depth, bgr), pose) in enumerate(zip(frames, poses)):
            d = depth.copy()
            holes = rng.random(d.shape)
            d[holes < 0.03] = 0.0
            d[(holes > 0.03) & (holes < 0.05)] = 80.0                      # beyond max_depth
            if i == 1:
                d[:32, :32] = 0.0                                          # a whole region without a valid pixel
            if kind == "u16":
                mm = np.clip(np.rint(d * 1000.0), 0, 65535).astype(np.uint16)
                ctx.upload(i, mm, bgr)
                d = mm.astype(np.float32) / np.float32(1000.0)
            else:
                ctx.upload(i, d, bgr)
            ctx.integrate(i, pose)
            orc.tsdf_integrate(d, pose[0], pose[1])
        g = ctx.download_grid(tl3d.CH_TSDF)
    assert orc.tsdf[:, 1].sum() > 1000, (w, h, kind)
    assert np.array_equal(g, orc.tsdf), (w, h, kind)
