"""GPU: the warp calls of the C ABI (mxd_resize_crop_batch_warp and its
host-source / JPEG counterparts).  The expectation is always the CPU statement
(mxd_warp_apply_u8), and Pillow itself, applied to the u8 result of the same
call without warps; then, where the call has them, the NumPy restatements of
the tone table, the colour map and the format table in that order.  Every
comparison is of integer bits, and every byte of a destination buffer outside
the image's elements must keep the 0xff it was filled with."""
import os

import numpy as np
import pytest

import color_ref as C
import tone_ref as T
import warp_ref as W
from gpu_util import synth
from mlx_data_amd import capi
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expect, expected_table
from test_gpu_color import F32, FORMATTED, U8, Dsts, Sources, _plan_entry

pytestmark = pytest.mark.gpu

BF16_CHW = FORMATTED[5]
MODES = [W.NEAREST, W.BILINEAR]
MODE_IDS = ["nearest", "bilinear"]
KINDS = ["shear", "translate", "rotate", "outside"]
NO_WARP = (W.NONE, 0, None)


def _matrix(kind, w, h):
    return {"shear": W.shear(0.3, -0.1), "translate": W.translate(2.5, -1.25), "rotate": W.rotate_matrix(w, h, 30.0),
            "outside": W.OUTSIDE}[kind]


def _warped(q, warp):
    """The CPU statement's bytes, which must be Pillow's."""
    got = capi.warp_apply_u8(q, warp)
    assert np.array_equal(got, W.pillow_apply(q, warp))
    return got


def _expected(mode, q, warp, tone=None, m=None):
    p = _warped(q, warp)
    if tone is not None:
        p = T.apply(p, tone)
    if m is not None:
        p = C.apply_ref(p, m)
    if mode[1] is None:
        return p
    mean, std = (IMAGENET_MEAN, IMAGENET_STD) if mode[3] else (None, None)
    return expect(expected_table(mode[1], 3, mean, std), p)


def _launch(src, dsts, warps, tones=None, mats=None, stream=None):
    arr, n = capi.make_images(src.entries(dsts.pairs()))
    capi.resize_crop_batch_warp(arr, capi.make_warps(warps), capi.make_tones(tones) if tones is not None else None,
                                capi.make_colors(mats) if mats is not None else None, n, dsts.dtype(), dsts.fmt(), 0,
                                stream.handle if stream else None)
    if stream:
        stream.synchronize()


def _compare(outs, clean, plain, warps, tones, mats, mode, tag):
    for k, (o, q, wp, ok) in enumerate(zip(outs, plain, warps, clean)):
        e = _expected(mode, q, wp, tones[k] if tones is not None else None, mats[k] if mats is not None else None)
        assert o.shape == e.shape and o.dtype == e.dtype, (tag, mode[0], k)
        bad = int((o != e).sum())
        assert bad == 0, (tag, mode[0], k, wp, bad, np.argwhere(o != e)[:3])
        assert ok, (tag, mode[0], k, "bytes outside the image were written")


def _check(src, plain, warps, mode, tag, tones=None, mats=None, **kw):
    dsts = Dsts(src.geoms, mode, **kw)
    try:
        dsts.clear()
        _launch(src, dsts, warps, tones, mats)
        capi.check(capi.lib().mxd_device_synchronize(0))
        outs, clean = dsts.read()
    finally:
        dsts.free()
    _compare(outs, clean, plain, warps, tones, mats, mode, tag)
    return outs


def _warps(src, mode, kind, fill=(10, 200, 90)):
    return [(mode, fill, _matrix(kind, g[4], g[5])) for g in src.geoms]


# ---- the smallest windows that can go wrong -------------------------------------------

@pytest.fixture(scope="module")
def windows():
    """Crop windows 1x1, 3x2 (mirrored) and 5x7 (lane tails, rows shorter than
    a lane's four pixels) and 65x17 (a second tile in both directions)."""
    imgs = [synth(61, 97, 3, 800 + k) for k in range(4)]
    geoms = [(40, 36, 3, 5, 1, 1, 0), (40, 36, 1, 3, 3, 2, 1), (40, 36, 3, 5, 5, 7, 0), (90, 60, 7, 2, 65, 17, 0)]
    src = Sources(imgs, geoms)
    plain = src.plain_u8()
    yield src, plain
    src.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_small_windows_in_u8(windows, mode, kind):
    src, plain = windows
    warps = _warps(src, mode, kind)
    outs = _check(src, plain, warps, U8, kind)
    if kind == "outside":
        assert all((o == np.array([10, 200, 90], np.uint8)).all() for o in outs)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_none_mixed_into_a_batch_and_the_identity(windows, mode):
    src, plain = windows
    g = src.geoms
    warps = [NO_WARP, (mode, 7, _matrix("rotate", g[1][4], g[1][5])), (mode, 255, W.IDENTITY), NO_WARP]
    outs = _check(src, plain, warps, U8, "mixed")
    assert all(np.array_equal(outs[k], plain[k]) for k in (0, 2, 3))
    outs = _check(src, plain, warps, BF16_CHW, "mixed")


@pytest.mark.parametrize("kind", ["shear", "translate", "rotate"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_a_destination_one_byte_past_alignment_with_padded_rows(windows, mode, kind):
    src, plain = windows
    _check(src, plain, _warps(src, mode, kind), U8, "odd", dst_pad=2, dst_shift=1)
    _check(src, plain, _warps(src, mode, kind), U8, "padded", dst_pad=4)


# ---- every resize route -----------------------------------------------------------------

def test_224_from_a_wave_kernel_source():
    imgs = [synth(300, 400, 3, 21), synth(300, 400, 3, 22)]
    geoms = [(341, 256, 58, 16, 224, 224, 0), (341, 256, 58, 16, 224, 224, 1)]
    src = Sources(imgs, geoms)
    try:
        plan = capi.describe_plan(_plan_entry(imgs[0], geoms[0], src.pitches[0]))
        assert plan["wave"] == 1, plan
        plain = src.plain_u8()
        m = W.rotate_matrix(224, 224, 30.0)
        _check(src, plain, [(W.BILINEAR, (124, 116, 104), m), (W.NEAREST, (124, 116, 104), m)], U8, "224")
    finally:
        src.free()


@pytest.mark.parametrize("policy", [capi.MXD_POLICY_AUTO, capi.MXD_POLICY_PREFER_BAND], ids=["auto", "prefer-band"])
def test_band_and_general_kernel_sources(policy):
    """test_gpu_color.py's routes: 680x680 -> 40x40 and unaligned source rows
    (the general kernel), 600x600 -> 40x40 (the band kernel under
    MXD_POLICY_PREFER_BAND), each with its own warp."""
    imgs = [synth(680, 680, 3, 3), synth(99, 101, 3, 4), synth(600, 600, 3, 5)]
    geoms = [(40, 40, 0, 0, 40, 40, 0), (75, 70, 3, 2, 61, 33, 1), (40, 40, 0, 0, 40, 40, 0)]
    src = Sources(imgs, geoms, src_align=[16, 1, 16])
    prev = capi.set_kernel_policy(policy)
    try:
        plans = [capi.describe_plan(_plan_entry(i, g, p)) for i, g, p in zip(imgs, geoms, src.pitches)]
        assert plans[0]["wave"] == 0 and plans[1]["wave"] == 0, plans
        assert capi.describe_band_plan(_plan_entry(imgs[2], geoms[2], src.pitches[2]))["band"] == 1
        plain = src.plain_u8()
        warps = [(W.BILINEAR, 3, W.shear(0.3, 0.0)), (W.NEAREST, (1, 2, 3), W.rotate_matrix(61, 33, 30.0)),
                 (W.NEAREST, 128, W.translate(2.5, -1.25))]
        _check(src, plain, warps, U8, "routes")
        _check(src, plain, warps, F32, "routes")
    finally:
        capi.set_kernel_policy(prev)
        src.free()


# ---- what follows the warp in the launch ---------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_warp_then_equalize_then_colour_then_bf16_chw(windows, mode):
    """EQUALIZE counts the fill pixels: its statistics are the warped image's."""
    src, plain = windows
    warps = _warps(src, mode, "rotate", fill=(255, 0, 30))
    tones = [(T.EQUALIZE, 0, 0.0)] * 4
    mats = C.eight_matrices()[1:5]
    _check(src, plain, warps, BF16_CHW, "chain", tones, mats)
    _check(src, plain, warps, U8, "tone only", tones)
    _check(src, plain, warps, U8, "colour only", None, mats, dst_pad=2, dst_shift=1)
    _check(src, plain, warps, BF16_CHW, "format only")
    q = plain[3]
    assert not np.array_equal(T.apply(_warped(q, warps[3]), tones[3]), _warped(T.apply(q, tones[3]), warps[3]))


def test_two_calls_on_one_stream_with_other_matrices(windows):
    """The same shapes and destinations: the uploads differ in the matrices only."""
    src, plain = windows
    dsts = Dsts(src.geoms, U8)
    stream = capi.Stream(0)
    try:
        a = _warps(src, W.BILINEAR, "rotate")
        b = _warps(src, W.BILINEAR, "shear")
        c = _warps(src, W.NEAREST, "translate")
        for tag, warps in (("a", a), ("b", b), ("c", c), ("a again", a)):
            dsts.clear()
            _launch(src, dsts, warps, None, None, stream)
            _compare(*dsts.read(), plain, warps, None, None, U8, tag)
    finally:
        stream.close()
        dsts.free()


# ---- host and JPEG sources ----------------------------------------------------------------

def test_host_sources():
    imgs = [synth(120, 160, 3, 40 + k) for k in range(3)]
    geoms = [(80, 60, 5, 3, 70, 41, k % 2) for k in range(3)]
    warps = [(W.BILINEAR, 9, W.rotate_matrix(70, 41, 30.0)), NO_WARP, (W.NEAREST, (4, 5, 6), W.translate(2.5, -1.25))]
    tones = [(T.EQUALIZE, 0, 0.0), (T.CONTRAST, 0, 1.3), (T.NONE, 0, 0.0)]

    def entries(pairs):
        return [dict(src=imgs[k].ctypes.data, src_stride=160 * 3, src_w=160, src_h=120, channels=3, resize_w=80,
                     resize_h=60, crop_x=5, crop_y=3, crop_w=70, crop_h=41, flip=geoms[k][6], dst=p, dst_stride=dp)
                for k, (p, dp) in enumerate(pairs)]

    plain_d, dsts, dsts8 = Dsts(geoms, U8), Dsts(geoms, BF16_CHW), Dsts(geoms, U8)
    try:
        arr, n = capi.make_images(entries(plain_d.pairs()))
        capi.resize_crop_to_device(arr, n, capi.MXD_U8, 0)
        plain = plain_d.read()[0]
        dsts.clear()
        arr, n = capi.make_images(entries(dsts.pairs()))
        capi.resize_crop_to_device_warp(arr, capi.make_warps(warps), capi.make_tones(tones), None, n, dsts.dtype(),
                                        dsts.fmt(), 0)
        _compare(*dsts.read(), plain, warps, tones, None, BF16_CHW, "host")
        dsts8.clear()
        arr, n = capi.make_images(entries(dsts8.pairs()))
        capi.resize_crop_to_device_warp(arr, capi.make_warps(warps), None, None, n, capi.MXD_U8, None, 0)
        _compare(*dsts8.read(), plain, warps, None, None, U8, "host u8")
    finally:
        plain_d.free()
        dsts.free()
        dsts8.free()


def test_jpeg_sources():
    """A 4:2:0 fixture (83x61) and the 300x200 4:2:0 photograph."""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz"))
    names = ["sub2_prog0_jpg", "caltech_300x200_jpg"]
    geoms = [(60, 44, 3, 1, 53, 41, 1), (341 * 3 // 4, 171, 11, 5, 224, 160, 0)]
    coefs = [capi.JpegCoefs(gold[k]) for k in names]
    warps = [(W.NEAREST, (0, 255, 0), W.shear(0.3, -0.1)), (W.BILINEAR, 77, W.rotate_matrix(224, 160, 30.0))]
    plain_d, dsts = Dsts(geoms, U8), Dsts(geoms, U8)

    def entries(pairs):
        return [dict(coefs=c, resize_w=g[0], resize_h=g[1], crop_x=g[2], crop_y=g[3], crop_w=g[4], crop_h=g[5],
                     flip=g[6], dst=p, dst_stride=dp) for c, g, (p, dp) in zip(coefs, geoms, pairs)]

    try:
        arr, n = capi.make_jpeg_images(entries(plain_d.pairs()))
        capi.jpeg_resize_crop_to_device(arr, n, capi.MXD_U8, 0)
        plain = plain_d.read()[0]
        assert all(p.any() for p in plain)
        dsts.clear()
        arr, n = capi.make_jpeg_images(entries(dsts.pairs()))
        capi.jpeg_resize_crop_to_device_warp(arr, capi.make_warps(warps), None, None, n, capi.MXD_U8, None, 0)
        _compare(*dsts.read(), plain, warps, None, None, U8, "jpeg")
    finally:
        plain_d.free()
        dsts.free()
        for c in coefs:
            c.close()
