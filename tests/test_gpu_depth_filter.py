"""GPU: tl3d_filter_depth / tl3d_filter_depth_slots against the numpy formulations of depth_filter_reference.py: the output's BITS
and the four counts are equal on every crafted image of depth_filter_common.py (shapes, tile seams at every radius, support and
link decisions at their boundaries, invalid bit patterns, region sizes and topologies, stage A feeding stage B); the array call on
host and on device memory, in place and out of place, and the slot call give the same bytes in every run; refusals write nothing."""
import ctypes as C

import numpy as np
import pytest

import depth_filter_common as dc
import depth_filter_reference as dr
import tl3d
from tl3d import _cabi as abi

pytestmark = pytest.mark.gpu

CASES = dc.crafted_cases()
SHAPES = dc.by_shape(CASES)


def make_ctx(h, w, n_slots=2):
    return tl3d.FusionContext(w, h, 50.0, 50.0, 0.5 * (w - 1), 0.5 * (h - 1), n_slots=n_slots, grid=None)


@pytest.fixture(scope="module")
def reference():
    """name -> (filtered, counts) by the shifted-array formulation, computed once and never written to"""
    out = {}
    for name, img, prm in CASES:
        f, c = dr.filter_shifted(img, **prm)
        f.setflags(write=False)
        out[name] = (f, c)
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(dr.bits(a), dr.bits(b))


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_crafted_images_equal_the_reference(shape, reference):
    bad = []
    with make_ctx(*shape) as ctx:
        for name, img, prm in SHAPES[shape]:
            want, want_counts = reference[name]
            before = img.copy()
            got, counts = ctx.filter_depth(img, **prm)
            assert same_bits(img, before), name                          # the input is not written
            if not same_bits(got, want):
                bad.append((name, "image", int((dr.bits(got) != dr.bits(want)).sum())))
            if [counts[k] for k in ctx.DEPTH_FILTER_COUNTS] != want_counts.tolist():
                bad.append((name, "counts", counts, want_counts.tolist()))
    assert not bad, bad[:10]


def _to_device(img):
    import torch
    return torch.from_numpy(img.view(np.int16) if img.dtype == np.uint16 else img).cuda()


def _from_device(t, dtype):
    a = t.cpu().numpy()
    return a.view(np.uint16) if dtype == np.uint16 else a


@pytest.mark.parametrize("name", ["noise_f32_big", "noise_u16_big", "noise_f32_big_r3", "noise_u16_big_r3", "spiral_f32_keep", "comb_u16_drop",
                                  "mixed_invalid"])
def test_array_call_and_slot_call_give_the_same_bytes(name, reference):
    import torch
    _n, img, prm = next(c for c in CASES if c[0] == name)
    want, want_counts = reference[name]
    h, w = img.shape
    with make_ctx(h, w, n_slots=2) as ctx:
        for run in range(3):                                             # every run the same bytes
            got, counts = ctx.filter_depth(img, **prm)
            assert same_bits(got, want) and list(counts.values()) == want_counts.tolist(), run
        # in place, host
        buf = img.copy()
        got, counts = ctx.filter_depth(buf, out=buf, **prm)
        assert got is buf and same_bits(buf, want) and list(counts.values()) == want_counts.tolist()
        # device pointers, out of place and in place
        d_in = _to_device(img)
        d_out, counts = ctx.filter_depth(d_in, **prm)
        torch.cuda.synchronize()
        assert same_bits(_from_device(d_out, img.dtype), want) and list(counts.values()) == want_counts.tolist()
        assert same_bits(_from_device(d_in, img.dtype), img)
        d_same, counts = ctx.filter_depth(d_in, out=d_in, **prm)
        torch.cuda.synchronize()
        assert same_bits(_from_device(d_in, img.dtype), want) and list(counts.values()) == want_counts.tolist()
        # device in, host out and the other way round
        host_out = np.empty_like(img)
        ctx.filter_depth(_to_device(img), out=host_out, **prm)
        assert same_bits(host_out, want)
        d_out2 = torch.empty_like(d_in)
        ctx.filter_depth(img, out=d_out2, **prm)
        torch.cuda.synchronize()
        assert same_bits(_from_device(d_out2, img.dtype), want)
        # the slot call, then download_depth: the f32 image a fresh upload of the reference's answer gives
        for run in range(2):
            ctx.upload(0, img)
            ctx.upload(1, np.array(want))
            cnt = ctx.filter_depth_slots([0], **prm)
            assert cnt.dtype == np.int64 and cnt.shape == (1, 4) and cnt[0].tolist() == want_counts.tolist()
            assert same_bits(ctx.download_depth(0), ctx.download_depth(1)), run
        # a filtered slot filtered again: the reference's answer on the reference's answer
        again, _c = dr.filter_shifted(np.array(want), **prm)
        ctx.filter_depth_slots([1], **prm)
        ctx.upload(0, again)
        assert same_bits(ctx.download_depth(1), ctx.download_depth(0))


def test_slots_of_both_kinds_share_launches_without_mixing(reference):
    """more slots than one launch takes (16), f32 and u16 frames interleaved: every slot gets its own image's answer and counts"""
    h, w = 13, 37
    prm = dc.prm(radius=2, min_support=3, min_region=4)
    imgs = [dc.noise_image(h, w, 500 + i, np.uint16 if i % 3 == 1 else np.float32) for i in range(37)]
    want = [dr.filter_shifted(im, **prm) for im in imgs]
    with make_ctx(h, w, n_slots=len(imgs) + 1) as ctx:
        for order in (list(range(len(imgs))), list(range(len(imgs)))[::-1], [5], [4, 36, 1]):
            for i, im in enumerate(imgs):
                ctx.upload(i, im)
            cnt = ctx.filter_depth_slots(order, **prm)
            assert cnt.tolist() == [want[i][1].tolist() for i in order]
            for i in range(len(imgs)):
                ctx.upload(len(imgs), np.array(want[i][0]) if i in order else imgs[i])
                assert same_bits(ctx.download_depth(i), ctx.download_depth(len(imgs))), (order, i)
        assert ctx.filter_depth_slots([], **prm).shape == (0, 4)         # n == 0 is fine
        assert ctx.filter_depth_slots([2, 3], counts=False, **prm) is None


def test_refusals_write_nothing():
    h, w = 9, 33
    img = dc.noise_image(h, w, 3)
    img16 = dc.noise_image(h, w, 4, np.uint16)
    with make_ctx(h, w, n_slots=3) as ctx:
        lib, hnd = ctx._lib, ctx._h
        good = abi.DepthFilterParams(jump_rel=0.05, radius=1, min_support=4, min_region=0, reserved=0)

        def params(**kw):
            p = abi.DepthFilterParams(jump_rel=0.05, radius=1, min_support=4, min_region=0, reserved=0)
            for k, v in kw.items():
                setattr(p, k, v)
            return p
        bad_params = [params(jump_rel=0.0), params(jump_rel=-1.0), params(jump_rel=float("nan")), params(jump_rel=float("inf")),
                      params(radius=0), params(radius=4), params(min_support=-1), params(min_support=9), params(radius=2, min_support=25),
                      params(radius=3, min_support=49), params(min_region=-1), params(reserved=1)]
        out = np.full((h, w), 7.0, np.float32)
        cnt = (C.c_int64 * 4)(-5, -5, -5, -5)

        def untouched():
            return (out == 7.0).all() and list(cnt) == [-5] * 4
        for p in bad_params:
            assert lib.tl3d_filter_depth(hnd, abi.ptr(img), abi.DEPTH_F32_M, C.byref(p), abi.ptr(out), cnt) == abi.E_INVALID
            assert untouched()
        for args in ((None, abi.ptr(img), abi.DEPTH_F32_M, C.byref(good), abi.ptr(out), cnt),
                     (hnd, None, abi.DEPTH_F32_M, C.byref(good), abi.ptr(out), cnt),
                     (hnd, abi.ptr(img), abi.DEPTH_F32_M, None, abi.ptr(out), cnt),
                     (hnd, abi.ptr(img), abi.DEPTH_F32_M, C.byref(good), None, cnt),
                     (hnd, abi.ptr(img), abi.DEPTH_F32_M, C.byref(good), abi.ptr(out), None),
                     (hnd, abi.ptr(img), 7, C.byref(good), abi.ptr(out), cnt),
                     (hnd, abi.ptr(img), -1, C.byref(good), abi.ptr(out), cnt)):
            assert lib.tl3d_filter_depth(*args) == abi.E_INVALID
            assert untouched()
        # an output that overlaps the input without being it: one row down in the same buffer
        big = np.full((h + 1, w), 7.0, np.float32)
        big[:h] = img
        snap = big.copy()
        for a, b in ((big[:h], big[1:]), (big[1:], big[:h])):
            assert lib.tl3d_filter_depth(hnd, abi.ptr(a), abi.DEPTH_F32_M, C.byref(good), abi.ptr(b), cnt) == abi.E_INVALID
            assert same_bits(big, snap) and list(cnt) == [-5] * 4
        # the slot call
        ctx.upload(0, img)
        ctx.upload(1, img16)
        d0, d1 = ctx.download_depth(0), ctx.download_depth(1)
        cn = np.full((3, 4), -5, np.int64)

        def slots_call(sl, p=good, n=None, c=cn):
            a = np.ascontiguousarray(sl, np.int32)
            return lib.tl3d_filter_depth_slots(hnd, len(a) if n is None else n, abi.ptr(a), C.byref(p) if p is not None else None, abi.ptr(c))
        for p in bad_params:
            assert slots_call([0, 1], p) == abi.E_INVALID
        assert slots_call([0, 1], None) == abi.E_INVALID
        assert slots_call([0, 1], n=-1) == abi.E_INVALID
        assert slots_call([0, 3]) == abi.E_INVALID and slots_call([-1]) == abi.E_INVALID          # out of range
        assert slots_call([0, 1, 0]) == abi.E_INVALID                                             # named twice
        assert lib.tl3d_filter_depth_slots(hnd, 2, None, C.byref(good), abi.ptr(cn)) == abi.E_INVALID
        assert lib.tl3d_filter_depth_slots(None, 1, abi.ptr(np.zeros(1, np.int32)), C.byref(good), abi.ptr(cn)) == abi.E_INVALID
        assert slots_call([0, 2]) == abi.E_STATE and b"holds no frame" in lib.tl3d_last_error()   # slot 2 holds no frame
        assert (cn == -5).all()
        assert same_bits(ctx.download_depth(0), d0) and same_bits(ctx.download_depth(1), d1)
        assert slots_call([], n=0) == abi.OK and (cn == -5).all()
        # and the good call still works afterwards, NULL counts too
        assert slots_call([1, 0], c=None) == abi.OK
        ctx.upload(2, dr.filter_shifted(img)[0])
        assert same_bits(ctx.download_depth(0), ctx.download_depth(2))
        ctx.upload(2, dr.filter_shifted(img16)[0])
        assert same_bits(ctx.download_depth(1), ctx.download_depth(2))
