"""GPU: FusionContext.icp_evaluate (tl3d_icp_evaluate_pairs) -- one point-to-plane pass per pair at a given pose -- against the
C oracle's icp_sums, its determinism, its error codes, and its agreement with the statistics a registration reports."""
import numpy as np
import pytest

import tl3d
from tl3d import _cabi as abi
from tl3d import synth
from oracle import c_oracle

from loop_closure_common import sym6

pytestmark = pytest.mark.gpu

W, H = 320, 240
CAM = dict(fx=300.0, fy=300.0, cx=160.0, cy=120.0)
EPS = 2.0 ** -52


def _frames(n=4, deg=3.0, sigma=0.001):
    scene = synth.object_scene(True)
    poses = synth.orbit_poses(n, 1.0, deg)
    frames = [synth.render(scene, p, W, H, **CAM, noise_sigma=sigma, seed=40 + i) for i, p in enumerate(poses)]
    return poses, frames


def _rel(poses, i, j):
    r, t = synth.relative_pose(poses[i], poses[j])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = r, np.asarray(t).reshape(3)
    return T


def _context(frames, radius):
    ctx = tl3d.FusionContext(W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], n_slots=len(frames) + 1, grid=None)
    ctx.set_normal_smoothing(radius)
    for i, (d, c) in enumerate(frames):
        ctx.upload(i, d, c)
        ctx.build_normals(i)
    return ctx


def _oracle():
    return c_oracle.Oracle(W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], 0.1, 50.0, dims=(8, 8, 8), origin=(0.0, 0.0, 0.0),
                           voxel_size=0.02, sdf_trunc=0.08)


def _check_against_oracle(res, sums, cnt, nsrc, what):
    A, b, e = sym6(sums), sums[21:27], sums[27]
    d_a = np.abs(res["A"] - A) / np.maximum(np.sqrt(np.outer(np.diag(A), np.diag(A))), 1e-300)
    d_b = np.abs(res["b"] - b) / np.maximum(np.sqrt(np.diag(A) * e), 1e-300)
    d_e = abs(res["e"] - e) / max(e, 1e-300)
    print(f"{what}: n_corr {res['n_corr']} / {cnt}, n_src {res['n_src']} / {nsrc}; |dA| {d_a.max() / EPS:.1f}, |db| {d_b.max() / EPS:.1f}, "
          f"|de| {d_e / EPS:.1f} (units of 2^-52; bound n_corr = {cnt})")
    assert res["n_corr"] == cnt and res["n_src"] == nsrc, what
    assert np.array_equal(res["A"], res["A"].T)
    # the reordering bound of an fp64 sum of n_corr terms
    assert d_a.max() <= cnt * EPS and d_b.max() <= cnt * EPS and d_e <= cnt * EPS, what
    assert res["fitness"] == (cnt / nsrc if nsrc else 0.0)
    assert res["rmse"] == pytest.approx(np.sqrt(e / cnt) if cnt else 0.0, rel=max(1e-12, cnt * EPS))


@pytest.mark.parametrize("radius", [0, 1])
def test_evaluate_matches_oracle_sums(radius):
    poses, frames = _frames(n=4, deg=3.0)
    far_pose = synth.orbit_poses(2, 1.0, 50.0)[1]                         # little overlap with frame 0
    frames.append(synth.render(synth.object_scene(True), far_pose, W, H, **CAM, noise_sigma=0.001, seed=77))
    poses = list(poses) + [far_pose]
    orc = _oracle()
    if radius:
        maps = [orc.normals_smooth(d, radius=radius) for d, _ in frames]
    else:
        maps = [(d, orc.normals(d)) for d, _ in frames]
    with _context(frames, radius) as ctx:
        cases = [(0, 1, _rel(poses, 0, 1)), (2, 1, _rel(poses, 2, 1)), (0, 3, np.eye(4)), (0, 4, _rel(poses, 0, 4)), (4, 0, np.eye(4))]
        for stride in (1, 2, 3, 4):
            for gate in (0.02, 0.05, 0.2):
                got = ctx.icp_evaluate([(i, j) for i, j, _ in cases], [T for _, _, T in cases], stride=stride, max_dist=gate)
                assert len(got) == len(cases)
                for (i, j, T), res in zip(cases, got):
                    sums, cnt, nsrc = orc.icp_sums(maps[i][0], maps[j][1], T, stride=stride, max_dist=gate)
                    _check_against_oracle(res, sums, cnt, nsrc, f"radius {radius} stride {stride} gate {gate} pair ({i}, {j})")
        low = ctx.icp_evaluate([(0, 4)], [_rel(poses, 0, 4)], stride=2, max_dist=0.05)[0]
        full = ctx.icp_evaluate([(0, 1)], [_rel(poses, 0, 1)], stride=2, max_dist=0.05)[0]
        assert 0 < low["n_corr"] < 0.6 * full["n_corr"]                      # the pair with little overlap is one
        # a source scale: the oracle's scale_src
        res = ctx.icp_evaluate([(0, 1)], [_rel(poses, 0, 1)], stride=2, max_dist=0.05, scales=[1.001])[0]
        sums, cnt, nsrc = orc.icp_sums(maps[0][0], maps[1][1], _rel(poses, 0, 1), stride=2, max_dist=0.05, scale_src=1.001)
        _check_against_oracle(res, sums, cnt, nsrc, "scaled source")


def _same(a, b):
    return (np.array_equal(a["A"], b["A"]) and np.array_equal(a["b"], b["b"]) and a["e"] == b["e"] and a["n_corr"] == b["n_corr"]
            and a["n_src"] == b["n_src"])


def test_result_does_not_depend_on_the_batch_or_the_run():
    poses, frames = _frames(n=4, deg=3.0)
    with _context(frames, 1) as ctx:
        T = _rel(poses, 0, 1)
        alone = ctx.icp_evaluate([(0, 1)], [T], stride=2, max_dist=0.05)[0]
        assert alone["n_corr"] > 1000
        rng = np.random.default_rng(5)
        pairs = [(int(a), int(b)) for a, b in rng.integers(0, 4, (200, 2))]
        Ts = [_rel(poses, a, b) for a, b in pairs]
        for pos in (0, 57, 199):
            pairs[pos], Ts[pos] = (0, 1), T
        batch = ctx.icp_evaluate(pairs, Ts, stride=2, max_dist=0.05)
        again = ctx.icp_evaluate(pairs, Ts, stride=2, max_dist=0.05)
        for pos in (0, 57, 199):
            assert _same(alone, batch[pos]), pos
        assert all(_same(a, b) for a, b in zip(batch, again))
        assert _same(alone, ctx.icp_evaluate([(0, 1)], [T], stride=2, max_dist=0.05)[0])
        assert ctx.icp_evaluate([], [], stride=2, max_dist=0.05) == []      # n_pairs = 0 is accepted


def test_error_codes():
    poses, frames = _frames(n=3, deg=3.0)
    with _context(frames, 0) as ctx:
        lib = abi.load()

        def fails(code, *a, **k):
            with pytest.raises(tl3d.Tl3dError) as ei:
                ctx.icp_evaluate(*a, **k)
            assert ei.value.code == code, ei.value
            assert lib.tl3d_last_error()                                     # ... with a message
        fails(abi.E_INVALID, [(0, 9)], None)                                 # slots out of range (n_slots = 4)
        fails(abi.E_INVALID, [(-1, 0)], None)
        fails(abi.E_INVALID, [(0, 1)], None, stride=0)
        fails(abi.E_INVALID, [(0, 1)], None, max_dist=0.0)
        fails(abi.E_INVALID, [(0, 1)], None, max_dist=-1.0)
        fails(abi.E_STATE, [(0, 3)], None)                                   # slot 3 holds no frame
        ctx.upload(3, *frames[0])
        fails(abi.E_STATE, [(0, 3)], None)                                   # ... and then no normal map
        assert ctx.icp_evaluate([(3, 0)], None)[0]["n_corr"] > 0             # as a SOURCE it needs none
        ctx.icp_batch_enqueue([(0, 1)], [dict(iters=2, stride=4, max_dist=0.05)])
        fails(abi.E_STATE, [(0, 1)], None)                                   # a batch is in flight
        ctx.icp_batch_collect()
        assert ctx.icp_evaluate([(0, 1)], None)[0]["n_corr"] > 0


@pytest.mark.parametrize("radius", [0, 1])
def test_registration_statistics_are_the_evaluation_at_its_pose(radius):
    poses, frames = _frames(n=4, deg=3.0)
    with _context(frames, radius) as ctx:
        levels = [dict(iters=10, stride=4, max_dist=0.20), dict(iters=15, stride=2, max_dist=0.05)]
        pairs = [(0, 1), (1, 2), (2, 3), (0, 3)]
        reg = ctx.icp_batch(pairs, levels)
        ev = ctx.icp_evaluate(pairs, [r["T"] for r in reg], stride=2, max_dist=0.05)
        for p, r, e in zip(pairs, reg, ev):
            print(p, r["n_corr"], e["n_corr"], r["n_src"], e["n_src"], r["rmse"], e["rmse"])
            assert r["status"] != 2
            assert r["n_corr"] == e["n_corr"] and r["n_src"] == e["n_src"]
            assert e["rmse"] == pytest.approx(r["rmse"], rel=1e-12)
            assert e["fitness"] == pytest.approx(r["fitness"], rel=1e-15)
