"""GPU: the crafted ICP pairs of icp_edges_common through normals_kernel / smooth_depth_kernel and through all three kernels that
share icp_accumulate_core -- icp_eval_kernel (icp_evaluate), icp_iter_kernel (icp with iters = 0: the final pass alone) and
icp_batch_kernel (icp_batch, one level with iters = 0) -- against the C oracle and the numpy formulation: maps bit for bit, counts
exactly, sums within the reordering bound of test_gpu_icp_eval (equal on the dyadic cases, whose sums are exact:
test_icp_edges_reference_cpu.py).  Every test has its own small context."""
import functools

import numpy as np
import pytest

import tl3d
from loop_closure_common import sym6
from oracle import second_numpy as sn

import icp_edges_common as ic
from test_gpu_icp_eval import _check_against_oracle

pytestmark = pytest.mark.gpu

CASES = ic.cases()
BY_NAME = {c.name: c for c in CASES}


def _ids(cases):
    return [c.name for c in cases]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """maps of both references and the C oracle's sums, once per case"""
    case = BY_NAME[name]
    mc, mn = ic.maps_c(case), ic.maps_numpy(case)
    sums, cnt, nsrc = ic.c_oracle_for(case).icp_sums(mc[0], mc[2], case.T, stride=case.stride, max_dist=case.max_dist, scale_src=case.scale)
    _, _, _, cnt_n, nsrc_n = sn.icp_sums(ic.geometry(case), mn[0], mn[2], case.T, stride=case.stride, max_dist=case.max_dist,
                                         scale_src=case.scale)
    assert (cnt, nsrc) == (cnt_n, nsrc_n)
    return dict(maps_c=mc, maps_n=mn, sums=sums, cnt=cnt, nsrc=nsrc)


def _context(width, height, radius, n_slots=2):
    ctx = tl3d.FusionContext(width, height, ic.FX, ic.FY, ic.CX, ic.CY, min_depth=ic.MIN_DEPTH, max_depth=ic.MAX_DEPTH, n_slots=n_slots,
                             grid=None)
    ctx.set_normal_smoothing(radius)
    return ctx


def _load(ctx, case):
    """source in slot 0 (its window-averaged depth is built with its normals when smoothing is on; a raw source needs no map),
    target in slot 1"""
    ctx.upload(0, case.src)
    ctx.upload(1, case.tgt)
    if case.radius > 0:
        ctx.build_normals(0, scale=case.scale, depth_jump=case.jump)
    ctx.build_normals(1, depth_jump=case.jump)


def _check_map(ctx, slot, want_c, want_n, what):
    import torch
    got = ctx.download_normals(slot)
    assert ic.same_bits(got, want_c), f"{what}: host destination differs from the C oracle"
    assert ic.same_bits(got, want_n), f"{what}: host destination differs from the numpy formulation"
    dev = torch.full(got.shape, -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                                               # the fill runs on torch's stream, the download on the context's
    ctx.download_normals(slot, out=dev)
    assert ic.same_bits(dev.cpu().numpy(), want_c), f"{what}: device destination"


# one map per distinct (target image, radius, jump)
_MAP_CASES = list({(id(c.tgt), c.radius, c.jump): c for c in CASES}.values())


@pytest.mark.parametrize("case", _MAP_CASES, ids=_ids(_MAP_CASES))
def test_normal_maps_equal_both_references(case):
    ref = _reference(case.name)
    with _context(case.width, case.height, case.radius) as ctx:
        ctx.upload(1, case.tgt)
        ctx.build_normals(1, depth_jump=case.jump)
        _check_map(ctx, 1, ref["maps_c"][2], ref["maps_n"][2], case.name)


def _check_statistics(res, ev, ref, what):
    """a registration's final pass against the reference's counts and the evaluation's statistics (the tolerances of
    test_gpu_icp_eval.test_registration_statistics_are_the_evaluation_at_its_pose)"""
    assert res["n_corr"] == ref["cnt"] and res["n_src"] == ref["nsrc"], (what, res["n_corr"], ref["cnt"], res["n_src"], ref["nsrc"])
    assert res["n_corr"] == ev["n_corr"] and res["n_src"] == ev["n_src"], what
    assert ev["rmse"] == pytest.approx(res["rmse"], rel=1e-12), what
    assert ev["fitness"] == pytest.approx(res["fitness"], rel=1e-15), what


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_one_pass_through_all_three_kernels(case):
    ref = _reference(case.name)
    sums, cnt, nsrc = ref["sums"], ref["cnt"], ref["nsrc"]
    level = dict(iters=0, stride=case.stride, max_dist=case.max_dist)
    with _context(case.width, case.height, case.radius, n_slots=3) as ctx:
        _load(ctx, case)
        ctx.upload(2, np.ascontiguousarray(case.tgt[::-1, ::-1]))          # a different frame, for the other pairs of the batch
        if case.radius > 0:                                                  # the source's own map, built at the source's scale
            nm_c = ic.c_oracle_for(case).normals_smooth(case.src, case.radius, case.scale, case.jump)[1]
            nm_n = sn.normals(ic.geometry(case), ref["maps_n"][0], case.scale, case.jump, step=case.radius)
            _check_map(ctx, 0, nm_c, nm_n, f"{case.name}: source map")
        # icp_eval_kernel
        ev = ctx.icp_evaluate([(0, 1)], [case.T], stride=case.stride, max_dist=case.max_dist, scales=[case.scale])[0]
        _check_against_oracle(ev, sums, cnt, nsrc, f"{case.name}: icp_evaluate")
        if case.exact:
            assert np.array_equal(ev["A"], sym6(sums)) and np.array_equal(ev["b"], sums[21:27]) and ev["e"] == sums[27], case.name
        # icp_iter_kernel: the final pass alone
        reg = ctx.icp(0, 1, T_init=case.T, scale_src=case.scale, **level)
        _check_statistics(reg, ev, ref, f"{case.name}: icp")
        # icp_batch_kernel: the case first and last among different pairs
        tie = ic.pose((1 / 64, 0.0, 0.0))
        pairs = [(0, 1), (2, 1), (1, 1), (2, 1), (0, 1)]
        poses = [case.T, None, tie, tie, case.T]
        scales = [case.scale, 1.0, 1.0, 1.0, case.scale]
        batch = ctx.icp_batch(pairs, [level], T_init=poses, scales=scales)
        others = ctx.icp_evaluate(pairs, poses, stride=case.stride, max_dist=case.max_dist, scales=scales)
        for pos in (0, 4):
            _check_statistics(batch[pos], ev, ref, f"{case.name}: icp_batch pair {pos}")
            assert others[pos]["n_corr"] == ev["n_corr"] and others[pos]["e"] == ev["e"] and np.array_equal(others[pos]["A"], ev["A"])
        for pos in (1, 2, 3):                                                # the kernels agree on the other pairs too
            assert batch[pos]["n_corr"] == others[pos]["n_corr"] and batch[pos]["n_src"] == others[pos]["n_src"], (case.name, pos)
            assert others[pos]["rmse"] == pytest.approx(batch[pos]["rmse"], rel=1e-12), (case.name, pos)


def _oracle_pass(case, src_map, nmap):
    return ic.c_oracle_for(case).icp_sums(src_map, nmap, case.T, stride=case.stride, max_dist=case.max_dist, scale_src=case.scale)


def test_radius_two_then_radius_zero_on_the_same_slot():
    """the slot's map is rebuilt unsmoothed, and as a source the slot is read as the raw frame again"""
    case = BY_NAME["smooth_r0_s1"]
    orc = ic.c_oracle_for(case)
    g = ic.geometry(case)
    with _context(case.width, case.height, 2) as ctx:
        ctx.upload(0, case.src)
        ctx.build_normals(0, depth_jump=case.jump)
        sd_c, nm_c = orc.normals_smooth(case.src, 2, 1.0, case.jump)
        sd_n = sn.smooth_depth(g, case.src, 1.0, case.jump, 2)
        _check_map(ctx, 0, nm_c, sn.normals(g, sd_n, 1.0, case.jump, step=2), "radius 2")
        ctx.set_normal_smoothing(0)
        ctx.build_normals(0, depth_jump=case.jump)
        _check_map(ctx, 0, orc.normals(case.src, 1.0, case.jump), sn.normals(g, case.src, 1.0, case.jump), "radius 0 after radius 2")
        ctx.upload(1, case.tgt)
        ctx.build_normals(1, depth_jump=case.jump)
        nmap = orc.normals(case.tgt, 1.0, case.jump)
        sums, cnt, nsrc = _oracle_pass(case, case.src, nmap)                 # slot 0 as the source: the raw frame, row-major
        stale = _oracle_pass(case, sd_c, nmap)
        assert cnt > 0 and not np.allclose(sums, stale[0], rtol=1e-9, atol=0.0)        # the averaged depth would show
        ev = ctx.icp_evaluate([(0, 1)], [case.T], stride=case.stride, max_dist=case.max_dist)[0]
        _check_against_oracle(ev, sums, cnt, nsrc, "slot rebuilt at radius 0 as a source")
        level = dict(iters=0, stride=case.stride, max_dist=case.max_dist)
        ref = dict(cnt=cnt, nsrc=nsrc)
        _check_statistics(ctx.icp(0, 1, T_init=case.T, **level), ev, ref, "icp")
        _check_statistics(ctx.icp_batch([(0, 1)], [level], T_init=[case.T])[0], ev, ref, "icp_batch")


def test_an_upload_into_a_smoothed_slot_is_read_raw_until_it_is_rebuilt():
    """slot 0 held a window-averaged map; a new frame is uploaded into it and used as a source without a rebuild: all three kernels
    read the new raw frame, not the old averaged depth"""
    case = BY_NAME["smooth_r1_s1"]
    orc = ic.c_oracle_for(case)
    old = ic.tgt_ramp()
    with _context(case.width, case.height, 1) as ctx:
        ctx.upload(0, old)
        ctx.build_normals(0, depth_jump=case.jump)
        ctx.upload(1, case.tgt)
        ctx.build_normals(1, depth_jump=case.jump)
        ctx.upload(0, case.src)
        _, nmap = orc.normals_smooth(case.tgt, 1, 1.0, case.jump)
        sums, cnt, nsrc = _oracle_pass(case, case.src, nmap)
        averaged = _oracle_pass(case, orc.normals_smooth(case.src, 1, 1.0, case.jump)[0], nmap)
        stale = _oracle_pass(case, orc.normals_smooth(old, 1, 1.0, case.jump)[0], nmap)
        assert cnt > 0 and (cnt, nsrc) != stale[1:] and not np.allclose(sums, averaged[0], rtol=1e-9, atol=0.0)      # told apart
        ref = dict(cnt=cnt, nsrc=nsrc)
        ev = ctx.icp_evaluate([(0, 1)], [case.T], stride=case.stride, max_dist=case.max_dist)[0]
        _check_against_oracle(ev, sums, cnt, nsrc, "raw source after a new upload")
        level = dict(iters=0, stride=case.stride, max_dist=case.max_dist)
        _check_statistics(ctx.icp(0, 1, T_init=case.T, **level), ev, ref, "icp")
        _check_statistics(ctx.icp_batch([(0, 1)], [level], T_init=[case.T])[0], ev, ref, "icp_batch")
