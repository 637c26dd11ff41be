"""GPU: the joint point-to-plane + photometric registration (csrc/kernels_rgbd.hip; build_intensity, download_intensity, rgbd_evaluate,
rgbd_register) against the numpy reference of tests/rgbd_reference.py: intensity maps bit for bit, one pass with exact counts and sums
inside the reordering bound, the registration inside the project's ICP bar, the known answers of the degenerate scenes, batch
independence, and every error of the C ABI.  Every comparison prints what it measured."""
import ctypes as C

import numpy as np
import pytest

import icp_degenerate_common as idc
import rgbd_common as rc
import rgbd_reference as ref
import tl3d
from tl3d import _cabi as abi

pytestmark = pytest.mark.gpu

SLOT = {name: (2 * i, 2 * i + 1) for i, name in enumerate(rc.NAMES)}               # (source, target)
SMALL = dict(width=24, height=18, fx=20.0, fy=20.0, cx=11.5, cy=8.5)


@pytest.fixture(scope="module")
def orc():
    return idc.oracle()


@pytest.fixture(scope="module")
def ctxs():
    """normal-smoothing radius -> a context with every pair's frames, normal maps and intensity maps"""
    out = {}
    for radius in (0, 1):
        ctx = tl3d.FusionContext(rc.W, rc.H, rc.CAM["fx"], rc.CAM["fy"], rc.CAM["cx"], rc.CAM["cy"], n_slots=2 * len(rc.NAMES), grid=None)
        ctx.set_normal_smoothing(radius)
        for name, (s, t) in SLOT.items():
            f = rc.pairs()[name]
            ctx.upload(s, f["src"], f["src_bgr"])
            ctx.upload(t, f["tgt"], f["tgt_bgr"])
        ctx.build_normals_many(list(range(2 * len(rc.NAMES))))
        ctx.build_intensity(list(range(2 * len(rc.NAMES))), rc.RADIUS, rc.JUMP)
        out[radius] = ctx
    yield out
    for ctx in out.values():
        ctx.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- intensity maps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_intensity_map_is_the_reference_bit_for_bit(kind):
    d, bgr = rc.crafted()
    if kind == "u16":
        with np.errstate(invalid="ignore"):
            d = np.where(np.isfinite(d) & (d > 0), d * 1000.0, 0.0).round().astype(np.uint16)
    with tl3d.FusionContext(**SMALL, n_slots=2, grid=None) as ctx:
        ctx.upload(0, d, bgr)
        ctx.upload(1, d, bgr)
        depth = ctx.download_depth(0)                       # the slot's f32 depth: what the map is defined on
        if kind == "f32":
            assert np.array_equal(_bits(depth), _bits(d))
        for radius in (0, 1, 2):
            ctx.build_intensity([0, 1] if radius == 1 else 0, radius, rc.JUMP)
            got, want = ctx.download_intensity(0), ref.intensity_map(depth, bgr, radius, rc.JUMP)
            assert np.array_equal(_bits(got), _bits(want)), f"{kind} radius {radius}"
            assert {0.0, 1.0, 2.0} <= set(np.unique(got[..., 3]))
        ctx.build_intensity([0, 1], rc.RADIUS, rc.JUMP)
        ctx.build_normals_many([0, 1])
        ev = ctx.rgbd_evaluate([(0, 1)], [np.eye(4)], stride=1, max_dist=0.1)[0]
        assert ev["n_photo"] > 0
        # a rewrite of the depth voids the map: E_STATE until it is rebuilt
        ctx.filter_depth_slots([0])
        for rebuild in (lambda: None, lambda: ctx.build_normals(0)):
            rebuild()
            with pytest.raises(tl3d.Tl3dError) as e:
                ctx.rgbd_evaluate([(1, 0)], [np.eye(4)], stride=1, max_dist=0.1)
            assert e.value.code == abi.E_STATE
        assert "intensity" in str(e.value)
        with pytest.raises(tl3d.Tl3dError) as e:
            ctx.download_intensity(0)
        assert e.value.code == abi.E_STATE
        ctx.build_intensity(0, rc.RADIUS, rc.JUMP)
        assert ctx.rgbd_evaluate([(1, 0)], [np.eye(4)], stride=1, max_dist=0.1)[0]["n_src"] > 0
        assert np.array_equal(_bits(ctx.download_intensity(0)), _bits(ref.intensity_map(ctx.download_depth(0), bgr, rc.RADIUS, rc.JUMP)))


# ---- one pass --------------------------------------------------------------------------------------------------------------------
def _vec(d, p=""):
    return np.concatenate([d["A" + p][np.triu_indices(6)] if d["A" + p].ndim == 2 else d["A" + p], d["b" + p], [d["e" + p]]])


@pytest.mark.parametrize("radius", [0, 1])
def test_evaluate_against_the_reference(ctxs, orc, radius):
    ctx = ctxs[radius]
    worst = 0.0
    for name in rc.NAMES:
        f = rc.pairs()[name]
        m = rc.maps(orc, name, radius)
        for stride in (1, 2, 3):
            for pose in ("T_true", "T_init"):
                what = f"{name} stride {stride} radius {radius} {pose}"
                want = ref.sums(rc.CAM, *m, f[pose], stride=stride, max_dist=0.1, photo_gate=rc.GATE)
                got = ctx.rgbd_evaluate([SLOT[name]], [f[pose]], stride=stride, max_dist=0.1, photo_gate=rc.GATE)[0]
                geo = ctx.icp_evaluate([SLOT[name]], [f[pose]], stride=stride, max_dist=0.1)[0]
                counts = tuple(got[k] for k in ("n_corr", "n_src", "n_qualified", "n_photo"))
                assert counts == tuple(want[k] for k in ("n_corr", "n_src", "n_qualified", "n_photo")), what
                assert want["n_photo"] > 500, what
                bg, bp = want["n_corr"] * idc.EPS * want["abs"], want["n_photo"] * idc.EPS * want["abs_p"]
                dg = np.abs(_vec(got) - _vec(want))
                dp = np.abs(_vec(got, "_p") - _vec(want, "_p"))
                assert (dg <= bg).all() and (dp <= bp).all(), what
                assert (geo["n_corr"], geo["n_src"]) == (got["n_corr"], got["n_src"]), what
                assert (np.abs(_vec(got) - _vec(geo)) <= bg).all(), what
                ratio = max(float((dg[bg > 0] / bg[bg > 0]).max()), float((dp[bp > 0] / bp[bp > 0]).max()))       # (a sum of zeros has bound 0)
                worst = max(worst, ratio)
                print(f"{what}: counts {counts}, worst |sum - ref| / bound {ratio:.3e}")
    print(f"radius {radius}: worst measured / bound {worst:.3e}")


def test_a_pair_does_not_depend_on_its_batch(ctxs):
    ctx = ctxs[0]
    f = rc.pairs()
    me, others = SLOT["tube"], [SLOT["control"], SLOT["plane"], SLOT["control"], SLOT["plane"]]
    T_me, T_others = f["tube"]["T_init"], [f[n]["T_init"] for n in ("control", "plane", "control", "plane")]

    def runs(pairs, T, k):
        ev = ctx.rgbd_evaluate(pairs, T, stride=2, max_dist=0.1)[k]
        rg = ctx.rgbd_register(pairs, rc.levels(), T_init=T)[k]
        return np.concatenate([_vec(ev), _vec(ev, "_p"), rg["T"].ravel(), [rg["rmse"], rg["photo_rmse"], rg["n_photo"], rg["iters_run"]]])
    alone = runs([me], [T_me], 0)
    for what, got in (("again", runs([me], [T_me], 0)), ("first of 5", runs([me] + others, [T_me] + T_others, 0)),
                      ("last of 5", runs(others + [me], T_others + [T_me], 4)), ("last of 5, again", runs(others + [me], T_others + [T_me], 4))):
        assert np.array_equal(alone.view(np.uint64), got.view(np.uint64)), what


# ---- the registration ---------------------------------------------------------------------------------------------------------------
def test_register_matches_the_reference(ctxs, orc):
    res = ctxs[0].rgbd_register([SLOT[n] for n in rc.NAMES], rc.levels(), T_init=[rc.pairs()[n]["T_init"] for n in rc.NAMES])
    for name, got in zip(rc.NAMES, res):
        want = rc.reference_run(orc, name)
        d = float(np.linalg.norm(got["T"] - want["T"]))
        print(f"{name}: |T - T_ref|_F {d:.3e} (bar 1e-4); status {got['status']} / {want['status']}, iterations {got['iters_run']} / {want['iters_run']}, "
              f"n_corr {got['n_corr']} / {want['n_corr']}, n_photo {got['n_photo']} / {want['n_photo']}, rmse {got['rmse']:.3e} / {want['rmse']:.3e}, "
              f"photometric rmse {got['photo_rmse']:.3e} / {want['photo_rmse']:.3e}")
        assert d <= 1e-4, name
        assert got["n_src"] == want["n_src"] and abs(got["n_corr"] - want["n_corr"]) <= 0.01 * want["n_corr"], name
        assert got["n_photo"] > 500 and got["photo_rmse"] > 0 and got["fitness"] == got["n_corr"] / got["n_src"], name


def test_weight_zero_is_the_batched_icp(ctxs):
    ctx = ctxs[0]
    T0 = [rc.pairs()["control"]["T_init"]]
    got = ctx.rgbd_register([SLOT["control"]], rc.levels(0.0), T_init=T0)[0]
    want = ctx.icp_batch([SLOT["control"]], rc.levels(0.0), T_init=T0)[0]
    d = float(np.linalg.norm(got["T"] - want["T"]))
    print(f"photo_weight 0 against icp_batch on control: |dT|_F {d:.3e} (bar 1e-9)")
    assert d <= 1e-9
    assert (got["n_corr"], got["n_src"], got["status"]) == (want["n_corr"], want["n_src"], want["status"])


def test_known_answers_hold_on_the_device(ctxs):
    """the planted slide of the tube and the in-plane motion of the wall: recovered with colour, left by icp_batch"""
    ctx = ctxs[0]
    names = ("tube", "plane")
    T0 = [rc.pairs()[n]["T_init"] for n in names]
    joint = ctx.rgbd_register([SLOT[n] for n in names], rc.levels(), T_init=T0)
    geo = ctx.icp_batch([SLOT[n] for n in names], rc.levels(), T_init=T0)
    err_j = {n: rc.trans_err(r["T"], rc.pairs()[n]) for n, r in zip(names, joint)}
    err_g = {n: rc.trans_err(r["T"], rc.pairs()[n]) for n, r in zip(names, geo)}
    print(f"joint: tube {err_j['tube'][0] * 1e3:.3f} mm, plane {err_j['plane'][0] * 1e3:.3f} mm; icp_batch: tube {err_g['tube'][1] * 1e3:.2f} mm along the "
          f"axis, plane {err_g['plane'][0] * 1e3:.2f} mm")
    assert err_j["tube"][0] <= rc.JOINT_BAR["tube"] and err_j["plane"][0] <= rc.JOINT_BAR["plane"]
    assert err_g["tube"][1] >= rc.TUBE_GEO_AXIS_MIN and err_g["plane"][0] > rc.PLANE_GEO_MIN


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_of_the_c_abi():
    lib = abi.load()
    d, bgr = rc.crafted()
    with tl3d.FusionContext(**SMALL, n_slots=4, grid=None) as ctx:
        h = ctx._h
        ctx.upload(0, d, bgr)
        ctx.upload(1, d, bgr)
        ctx.upload(2, d, None)                              # no colour; slot 3 stays empty
        ctx.build_normals_many([0, 1, 2])

        def build(slots, radius=1, jump=0.05):
            sl = np.asarray(slots, np.int32)
            return lib.tl3d_build_intensity_many(h, len(sl), abi.ptr(sl), radius, jump)

        def pair_arr(pairs):
            arr = np.zeros(len(pairs), [("slot_src", "<i4"), ("slot_tgt", "<i4"), ("scale_src", "<f8"), ("T_init", "<f8", (16,))])
            for i, (s, t) in enumerate(pairs):
                arr[i] = (s, t, 1.0, np.eye(4).ravel())
            return arr

        def evaluate(pairs=((0, 1),), stride=1, max_dist=0.1, gate=0.2, n=None):
            arr, out = pair_arr(pairs), (abi.RgbdEval * max(1, len(pairs)))()
            return lib.tl3d_rgbd_evaluate_pairs(h, arr.ctypes.data_as(C.POINTER(abi.IcpPair)), len(pairs) if n is None else n, stride, max_dist, gate, out)

        def register(pairs=((0, 1),), n_levels=1, n=None, **kw):
            prm = dict(iters=2, stride=1, max_dist=0.1, photo_weight=0.1, photo_gate=0.2, estimate_scale=False)
            prm.update(kw)
            lv = (abi.RgbdLevel * abi.ICP_MAX_LEVELS)()
            for i in range(abi.ICP_MAX_LEVELS):
                lv[i] = abi.RgbdLevel(abi.IcpParams(prm["iters"], prm["stride"], prm["max_dist"], 1e-6, 1e-9, 1e-4, int(prm["estimate_scale"]), 0),
                                      prm["photo_weight"], prm["photo_gate"])
            arr, out, info = pair_arr(pairs), (abi.IcpResult * max(1, len(pairs)))(), (abi.RgbdInfo * max(1, len(pairs)))()
            return lib.tl3d_rgbd_register_pairs(h, arr.ctypes.data_as(C.POINTER(abi.IcpPair)), len(pairs) if n is None else n, lv, n_levels, out, info)
        # intensity maps
        assert build([3]) == abi.E_STATE and build([2]) == abi.E_STATE                       # no frame; no colour
        assert b"colour" in lib.tl3d_last_error()
        assert build([4]) == abi.E_INVALID and build([-1]) == abi.E_INVALID
        assert build([0], radius=-1) == abi.E_INVALID and build([0], radius=8) == abi.E_INVALID
        assert build([0], jump=0.0) == abi.E_INVALID and build([0], jump=float("nan")) == abi.E_INVALID
        assert build([]) == abi.OK
        out = np.zeros((SMALL["height"], SMALL["width"], 4), np.float32)
        assert lib.tl3d_download_intensity(h, 0, abi.ptr(out)) == abi.E_STATE                # no map yet
        assert lib.tl3d_download_intensity(h, 4, abi.ptr(out)) == abi.E_INVALID
        # no intensity map on either side
        assert evaluate() == abi.E_STATE and register() == abi.E_STATE
        assert build([0]) == abi.OK
        assert evaluate() == abi.E_STATE and register() == abi.E_STATE
        assert build([0, 1], radius=7) == abi.OK and build([0, 1]) == abi.OK
        assert lib.tl3d_download_intensity(h, 0, None) == abi.E_INVALID
        assert evaluate() == abi.OK and register() == abi.OK
        # zero pairs
        assert evaluate(n=0) == abi.OK and register(n=0) == abi.OK
        assert lib.tl3d_rgbd_evaluate_pairs(h, None, 0, 1, 0.1, 0.2, None) == abi.OK
        assert evaluate(n=-1) == abi.E_INVALID and register(n=-1) == abi.E_INVALID
        # slots: out of range, empty, without colour
        for bad in ((0, 4), (-1, 1)):
            assert evaluate([bad]) == abi.E_INVALID and register([bad]) == abi.E_INVALID
        for bad in ((0, 3), (3, 1), (2, 1), (0, 2)):
            assert evaluate([bad]) == abi.E_STATE and register([bad]) == abi.E_STATE
        # parameters
        assert evaluate(stride=0) == abi.E_INVALID and register(stride=0) == abi.E_INVALID
        for g in (0.0, -1.0, float("nan")):
            assert evaluate(max_dist=g) == abi.E_INVALID and register(max_dist=g) == abi.E_INVALID
            assert evaluate(gate=g) == abi.E_INVALID and register(photo_gate=g) == abi.E_INVALID
        assert register(photo_weight=-0.1) == abi.E_INVALID and register(photo_weight=0.0) == abi.OK
        assert register(n_levels=0) == abi.E_INVALID and register(n_levels=abi.ICP_MAX_LEVELS + 1) == abi.E_INVALID
        assert register(n_levels=abi.ICP_MAX_LEVELS) == abi.OK
        assert register(estimate_scale=True) == abi.E_INVALID and b"scale" in lib.tl3d_last_error()
        # a target without a normal map; an uncollected ICP batch
        ctx.icp_batch_enqueue([(0, 1)], [dict(iters=1, stride=1, max_dist=0.1)])
        assert evaluate() == abi.E_STATE and register() == abi.E_STATE
        ctx.icp_batch_collect()
        ctx.upload(1, d, bgr)
        ctx.build_intensity(1)
        assert evaluate() == abi.E_STATE and register() == abi.E_STATE
        assert b"normal map" in lib.tl3d_last_error()
        ctx.build_normals(1)
        assert evaluate() == abi.OK and register() == abi.OK
