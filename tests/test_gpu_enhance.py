"""GPU: the enhance calls of the C ABI (mxd_resize_crop_batch_enhance and its
host-source / JPEG counterparts).  The expectation is always the CPU statement
(mxd_enhance_apply_u8), asserted equal to Pillow itself and to the NumPy
restatement, applied to the u8 result of the same call without enhance ops
(after the CPU statement of the warp, where the call has one); then, where the
call has them, the NumPy restatements of the tone table, the colour map and
the format table in that order.  Every comparison is of integer bits, and
every byte of a destination buffer outside the image's elements must keep the
0xff it was filled with."""
import os

import numpy as np
import pytest

import color_ref as C
import enhance_ref as E
import tone_ref as T
import warp_ref as W
from gpu_util import synth
from mlx_data_amd import capi
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expect, expected_table
from test_gpu_color import FORMATTED, U8, Dsts, Sources

pytestmark = pytest.mark.gpu

BF16_CHW = FORMATTED[5]
FACTORS = [0.0, 0.3, 1.0, 1.9, 5.0]
NO_ENHANCE = (E.NONE, 0.0)


def _enhanced(q, enh):
    """The CPU statement's bytes, which must be Pillow's and the restatement's."""
    got = capi.enhance_apply_u8(q, enh)
    assert np.array_equal(got, E.pillow_apply(q, enh)), enh
    assert np.array_equal(got, E.apply(q, enh)), enh
    return got


def _expected(mode, q, enh, warp=None, tone=None, m=None):
    p = q
    if warp is not None:
        p = capi.warp_apply_u8(p, warp)
    p = _enhanced(p, enh)
    if tone is not None:
        p = T.apply(p, tone)
    if m is not None:
        p = C.apply_ref(p, m)
    if mode[1] is None:
        return p
    mean, std = (IMAGENET_MEAN, IMAGENET_STD) if mode[3] else (None, None)
    return expect(expected_table(mode[1], 3, mean, std), p)


def _launch(src, dsts, enhs, warps=None, tones=None, mats=None, stream=None):
    arr, n = capi.make_images(src.entries(dsts.pairs()))
    capi.resize_crop_batch_enhance(arr, capi.make_warps(warps) if warps is not None else None, capi.make_enhances(enhs),
                                   capi.make_tones(tones) if tones is not None else None,
                                   capi.make_colors(mats) if mats is not None else None, n, dsts.dtype(), dsts.fmt(), 0,
                                   stream.handle if stream else None)
    if stream:
        stream.synchronize()


def _compare(outs, clean, plain, enhs, warps, tones, mats, mode, tag):
    for k, (o, q, en, ok) in enumerate(zip(outs, plain, enhs, clean)):
        e = _expected(mode, q, en, warps[k] if warps is not None else None, tones[k] if tones is not None else None,
                      mats[k] if mats is not None else None)
        assert o.shape == e.shape and o.dtype == e.dtype, (tag, mode[0], k)
        bad = int((o != e).sum())
        assert bad == 0, (tag, mode[0], k, en, bad, np.argwhere(o != e)[:3])
        assert ok, (tag, mode[0], k, "bytes outside the image were written")


def _check(src, plain, enhs, mode, tag, warps=None, tones=None, mats=None, **kw):
    dsts = Dsts(src.geoms, mode, **kw)
    try:
        dsts.clear()
        _launch(src, dsts, enhs, warps, tones, mats)
        capi.check(capi.lib().mxd_device_synchronize(0))
        outs, clean = dsts.read()
    finally:
        dsts.free()
    _compare(outs, clean, plain, enhs, warps, tones, mats, mode, tag)
    return outs


# ---- the smallest windows that can go wrong -------------------------------------------

@pytest.fixture(scope="module")
def windows():
    """Crop windows 1x1 (no interior), 3x2 mirrored (no interior, the mirror
    path), 3x3 (one interior pixel), 5x7 (lane tails), 65x17 (the interior
    crosses a tile edge in both directions: the halo comes from the neighbour
    tile) and 130x33 (a tile with tiles on every side)."""
    imgs = [synth(61, 97, 3, 900 + k) for k in range(5)] + [synth(80, 300, 3, 905)]
    geoms = [(40, 36, 3, 5, 1, 1, 0), (40, 36, 1, 3, 3, 2, 1), (40, 36, 2, 4, 3, 3, 0), (40, 36, 3, 5, 5, 7, 0),
             (90, 60, 7, 2, 65, 17, 0), (150, 40, 9, 3, 130, 33, 0)]
    src = Sources(imgs, geoms)
    plain = src.plain_u8()
    yield src, plain
    src.free()


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("op", E.OPS, ids=E.OP_IDS)
def test_small_windows_in_u8_and_bf16_chw(windows, op, factor):
    src, plain = windows
    enhs = [(op, factor)] * len(plain)
    outs = _check(src, plain, enhs, U8, "u8")
    if factor == 1.0:
        assert all(np.array_equal(o, q) for o, q in zip(outs, plain))
    if op == E.SHARPNESS:
        # the windows without an interior come back as they are, whatever the factor
        assert all(np.array_equal(outs[k], plain[k]) for k in (0, 1))
    _check(src, plain, enhs, BF16_CHW, "bf16 chw")


def test_none_mixed_into_a_batch(windows):
    src, plain = windows
    enhs = [NO_ENHANCE, (E.SHARPNESS, 1.9), (E.COLOR, 0.3), NO_ENHANCE, (E.BRIGHTNESS, 1.9), (E.SHARPNESS, 0.3)]
    outs = _check(src, plain, enhs, U8, "mixed")
    assert all(np.array_equal(outs[k], plain[k]) for k in (0, 3))
    assert not np.array_equal(outs[5], plain[5])
    _check(src, plain, enhs, BF16_CHW, "mixed")


@pytest.mark.parametrize("op", E.OPS, ids=E.OP_IDS)
def test_a_destination_one_byte_past_alignment_with_padded_rows(windows, op):
    src, plain = windows
    enhs = [(op, 1.9)] * len(plain)
    _check(src, plain, enhs, U8, "odd", dst_pad=2, dst_shift=1)
    _check(src, plain, enhs, U8, "padded", dst_pad=4)


# ---- what stands before and behind the stage in the launch ------------------------------

@pytest.mark.parametrize("op", E.OPS, ids=E.OP_IDS)
def test_rotation_then_enhance_then_equalize_then_colour_then_bf16_chw(windows, op):
    """With a warp the stage reads the warp's rows and writes the resize
    kernels' (dead by then); EQUALIZE's statistics are the enhanced bytes'."""
    src, plain = windows
    n = len(plain)
    warps = [(W.BILINEAR, (255, 0, 30), W.rotate_matrix(g[4], g[5], 30.0)) for g in src.geoms]
    enhs = [(op, 1.9)] * n
    tones = [(T.EQUALIZE, 0, 0.0)] * n
    mats = (C.eight_matrices() * 2)[1:1 + n]
    _check(src, plain, enhs, BF16_CHW, "chain", warps, tones, mats)
    _check(src, plain, enhs, U8, "warp only", warps)
    _check(src, plain, enhs, U8, "tone only", None, tones)
    _check(src, plain, enhs, U8, "colour only", None, None, mats, dst_pad=2, dst_shift=1)
    _check(src, plain, enhs, BF16_CHW, "warp and format", warps)
    q = capi.warp_apply_u8(plain[5], warps[5])
    assert not np.array_equal(T.apply(_enhanced(q, enhs[5]), tones[5]), _enhanced(T.apply(q, tones[5]), enhs[5]))


def test_two_calls_on_one_stream_with_other_factors(windows):
    """The same shapes and destinations: the uploads differ in ops and factors only."""
    src, plain = windows
    n = len(plain)
    dsts = Dsts(src.geoms, U8)
    stream = capi.Stream(0)
    try:
        a = [(E.SHARPNESS, 1.9)] * n
        b = [(E.SHARPNESS, 0.3)] * n
        c = [(E.COLOR, 0.3)] * n
        for tag, enhs in (("a", a), ("b", b), ("c", c), ("a again", a)):
            dsts.clear()
            _launch(src, dsts, enhs, None, None, None, stream)
            _compare(*dsts.read(), plain, enhs, None, None, None, U8, tag)
    finally:
        stream.close()
        dsts.free()


# ---- host and JPEG sources ----------------------------------------------------------------

def test_host_sources():
    imgs = [synth(120, 160, 3, 60 + k) for k in range(3)]
    geoms = [(80, 60, 5, 3, 70, 41, k % 2) for k in range(3)]
    enhs = [(E.SHARPNESS, 1.9), NO_ENHANCE, (E.COLOR, 0.3)]
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
        capi.resize_crop_to_device_enhance(arr, None, capi.make_enhances(enhs), capi.make_tones(tones), None, n,
                                           dsts.dtype(), dsts.fmt(), 0)
        _compare(*dsts.read(), plain, enhs, None, tones, None, BF16_CHW, "host")
        dsts8.clear()
        arr, n = capi.make_images(entries(dsts8.pairs()))
        capi.resize_crop_to_device_enhance(arr, None, capi.make_enhances(enhs), None, None, n, capi.MXD_U8, None, 0)
        _compare(*dsts8.read(), plain, enhs, None, None, None, U8, "host u8")
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
    enhs = [(E.BRIGHTNESS, 1.9), (E.SHARPNESS, 1.9)]
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
        capi.jpeg_resize_crop_to_device_enhance(arr, None, capi.make_enhances(enhs), None, None, n, capi.MXD_U8, None, 0)
        _compare(*dsts.read(), plain, enhs, None, None, None, U8, "jpeg")
    finally:
        plain_d.free()
        dsts.free()
        for c in coefs:
            c.close()
