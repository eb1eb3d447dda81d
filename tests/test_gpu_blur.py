"""GPU: MXD_ENHANCE_GAUSSIAN_BLUR in the enhance calls of the C ABI (blur_rows).
Every case is bit-equal to the float32 restatement (tests/blur_ref.py) applied
to the u8 result of the same chain in front of the op, followed by the
statements of what the chain runs behind it; bytes outside the images must
keep the 0xff they were filled with."""
import os

import numpy as np
import pytest

import blur_ref as B
import color_ref as C
import enhance_ref as E
import mix_ref as M
import tone_ref as T
import warp_ref as W
from gpu_util import synth
from mlx_data_amd import capi
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expect, expected_table
from test_gpu_color import FORMATTED, U8, Dsts, Sources

pytestmark = pytest.mark.gpu

BLUR = capi.MXD_ENHANCE_GAUSSIAN_BLUR
BF16_CHW = FORMATTED[5]
# w x h: radius >= size (repeated reflection), one strip, 64 +- 1, several strips; heights on
# both sides of a segment boundary (112 rows: the last one has a second segment of three rows)
SIZES = [(1, 1), (2, 5), (17, 3), (63, 70), (65, 33), (130, 67), (20, 115)]
# a near-delta kernel, flushed tail weights, the widest ring
KERNELS = [(3, 0.1), (3, 2.0), (23, 2.0), (33, 0.5), (33, 5.0)]


def _op(q, enh):
    if enh[0] == BLUR:
        return B.blur_f32(q, enh[2], enh[1])
    return capi.enhance_apply_u8(q, enh)


def _expected(mode, q, enh, warp=None, tone=None, m=None):
    p = _op(capi.warp_apply_u8(q, warp) if warp is not None else q, enh)
    if tone is not None:
        p = T.apply(p, tone)
    if m is not None:
        p = C.apply_ref(p, m)
    if mode[1] is None:
        return p
    return expect(expected_table(mode[1], 3, IMAGENET_MEAN, IMAGENET_STD), p)


def _run(src, enhs, mode, warps=None, tones=None, mats=None, mixes=None, stream=None, **kw):
    dsts = Dsts(src.geoms, mode, **kw)
    try:
        dsts.clear()
        arr, n = capi.make_images(src.entries(dsts.pairs()))
        members = (capi.make_warps(warps) if warps else None, capi.make_enhances(enhs),
                   capi.make_tones(tones) if tones else None, capi.make_colors(mats) if mats else None)
        tail = (n, dsts.dtype(), dsts.fmt(), 0, stream.handle if stream else None)
        if mixes:
            capi.resize_crop_batch_mix(arr, *members, capi.make_mixes(mixes), *tail)
        else:
            capi.resize_crop_batch_enhance(arr, *members, *tail)
        capi.check(capi.lib().mxd_device_synchronize(0))
        outs, clean = dsts.read()
    finally:
        dsts.free()
    assert all(clean), "bytes outside the images were written"
    return outs


def _same(outs, wants, tag):
    for k, (o, e) in enumerate(zip(outs, wants)):
        assert o.shape == e.shape and o.dtype == e.dtype, (tag, k)
        assert np.array_equal(o, e), (tag, k, int((o != e).sum()), np.argwhere(o != e)[:3])


@pytest.fixture(scope="module")
def windows():
    imgs = [synth(90, 150, 3, 700 + k) for k in range(len(SIZES))]
    geoms = [(140, 125, 3 + k, 5, w, h, k % 2) for k, (w, h) in enumerate(SIZES)]
    src = Sources(imgs, geoms)
    yield src, src.plain_u8()
    src.free()


@pytest.mark.parametrize("k,sigma", KERNELS)
def test_every_size_in_u8_with_aligned_and_misaligned_destinations(windows, k, sigma):
    src, plain = windows
    enhs = [(BLUR, sigma, k)] * len(plain)
    want = [_expected(U8, q, e) for q, e in zip(plain, enhs)]
    _same(_run(src, enhs, U8), want, "u8")
    _same(_run(src, enhs, U8, dst_pad=2, dst_shift=1), want, "misaligned")
    if (k, sigma) == (3, 0.1):  # a near-delta kernel returns the image
        _same(want, plain, "delta")


def test_blur_sharpness_color_and_none_in_one_call(windows):
    src, plain = windows
    enhs = [(BLUR, 2.0, 23), (E.SHARPNESS, 1.9), (BLUR, 0.7, 5), (E.NONE, 0.0), (E.COLOR, 0.3), (BLUR, 5.0, 33),
            (BLUR, 1.0, 9)]
    _same(_run(src, enhs, U8), [_expected(U8, q, e) for q, e in zip(plain, enhs)], "mixed")
    # reversed: an unblurred image last in the entries, and the output form behind the stage
    enhs = enhs[::-1]
    _same(_run(src, enhs, BF16_CHW), [_expected(BF16_CHW, q, e) for q, e in zip(plain, enhs)], "mixed bf16")


def test_behind_a_warp_and_in_front_of_tone_colour_and_bf16_chw(windows):
    src, plain = windows
    n = len(plain)
    warps = [(W.BILINEAR, (255, 0, 30), W.rotate_matrix(g[4], g[5], 30.0)) for g in src.geoms]
    enhs = [(BLUR, 2.0, 23)] * n
    tones = [(T.EQUALIZE, 0, 0.0)] * n
    mats = (C.eight_matrices() * 2)[1:1 + n]
    want = [_expected(BF16_CHW, q, e, w, t, m) for q, e, w, t, m in zip(plain, enhs, warps, tones, mats)]
    _same(_run(src, enhs, BF16_CHW, warps, tones, mats), want, "chain")


def test_with_a_mix_stage_last(windows):
    src, plain = windows
    enhs = [(BLUR, 2.0, 23)] * len(plain)
    blurred = [_expected(U8, q, e) for q, e in zip(plain, enhs)]
    mixes = [M.entry_mixup(k, 0.3) for k in range(len(plain))]  # (each its own partner: sizes differ)
    want = [expect(expected_table("bfloat16", 3, IMAGENET_MEAN, IMAGENET_STD), M.apply(blurred, k, mixes[k]))
            for k in range(len(plain))]
    _same(_run(src, enhs, BF16_CHW, mixes=mixes), want, "mix")


def test_two_calls_on_one_stream_that_differ_in_sigma_only(windows):
    src, plain = windows
    stream = capi.Stream(0)
    try:
        outs = {}
        for sigma in (2.0, 1.0, 2.0):
            enhs = [(BLUR, sigma, 23)] * len(plain)
            outs[sigma] = _run(src, enhs, U8, stream=stream)
            _same(outs[sigma], [_expected(U8, q, e) for q, e in zip(plain, enhs)], sigma)
        assert not np.array_equal(outs[2.0][5], outs[1.0][5])
    finally:
        stream.close()


def test_jpeg_sources():
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz"))
    geoms = [(60, 44, 3, 1, 53, 41, 1), (341 * 3 // 4, 171, 11, 5, 224, 160, 0)]
    coefs = [capi.JpegCoefs(gold[k]) for k in ("sub2_prog0_jpg", "caltech_300x200_jpg")]
    enhs = [(BLUR, 0.5, 33), (BLUR, 2.0, 23)]
    plain_d, dsts = Dsts(geoms, U8), Dsts(geoms, U8)

    def entries(pairs):
        return [dict(coefs=c, resize_w=g[0], resize_h=g[1], crop_x=g[2], crop_y=g[3], crop_w=g[4], crop_h=g[5],
                     flip=g[6], dst=p, dst_stride=dp) for c, g, (p, dp) in zip(coefs, geoms, pairs)]

    try:
        arr, n = capi.make_jpeg_images(entries(plain_d.pairs()))
        capi.jpeg_resize_crop_to_device(arr, n, capi.MXD_U8, 0)
        plain = plain_d.read()[0]
        dsts.clear()
        arr, n = capi.make_jpeg_images(entries(dsts.pairs()))
        capi.jpeg_resize_crop_to_device_enhance(arr, None, capi.make_enhances(enhs), None, None, n, capi.MXD_U8, None, 0)
        outs, clean = dsts.read()
        assert all(clean)
        _same(outs, [_expected(U8, q, e) for q, e in zip(plain, enhs)], "jpeg")
    finally:
        plain_d.free()
        dsts.free()
        for c in coefs:
            c.close()
