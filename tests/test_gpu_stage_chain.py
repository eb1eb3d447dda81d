"""GPU: the stage chain behind the resize, end to end.  One call for every
null / non-null combination of {fmt, colors, tones, warps, enhances}, each
through the C entry point that combination maps to, over one batch that mixes
wave and non-wave images.  The expectation starts from the u8 result of the
plain mxd_resize_crop_batch of the same images; on it the CPU statements of
the warp and the enhance op, then the NumPy restatements of the tone table,
the colour map and the format table, in that order.  A stage that reads the
wrong rows, or runs in place, changes bytes; every comparison is of integer
bits, and every byte of a destination buffer outside the image's elements
must keep the 0xff it was filled with."""
import itertools

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
FILL = (124, 116, 104)

# test_gpu_enhance.py's six windows (1x1, 3x2 mirrored, 3x3, 5x7, 65x17,
# 130x33), then 500x375 -> 341x256, crop 224x224: a wave image.
GEOMS = [(40, 36, 3, 5, 1, 1, 0), (40, 36, 1, 3, 3, 2, 1), (40, 36, 2, 4, 3, 3, 0), (40, 36, 3, 5, 5, 7, 0),
         (90, 60, 7, 2, 65, 17, 0), (150, 40, 9, 3, 130, 33, 0), (341, 256, 58, 16, 224, 224, 0)]
# Per image; every array holds one NONE (the colours: the identity).
ENHANCES = [(E.NONE, 0.0), (E.COLOR, 0.3), (E.BRIGHTNESS, 1.9), (E.SHARPNESS, 0.3), (E.SHARPNESS, 1.9),
            (E.SHARPNESS, 1.9), (E.COLOR, 1.9)]
WARPS = [(W.NONE, FILL, W.IDENTITY),
         (W.NEAREST, FILL, W.translate(1.0, 0.0)),             # table path
         (W.NEAREST, FILL, W.shear(0.3, -0.1)),                # fixed point
         (W.BILINEAR, FILL, W.rotate_matrix(5, 7, 30.0)),
         (W.NEAREST, FILL, (0.7, 0.0, 1.3, 0.0, 1.4, -0.6)),   # table path
         (W.BILINEAR, FILL, W.rotate_matrix(130, 33, 30.0)),
         (W.NEAREST, FILL, W.rotate_matrix(224, 224, -20.0))]  # fixed point
TONES = [(T.EQUALIZE, 0, 0.0), (T.POSTERIZE, 3, 0.0), (T.NONE, 0, 0.0), (T.AUTOCONTRAST, 0, 0.0), (T.EQUALIZE, 0, 0.0),
         (T.CONTRAST, 0, 1.3), (T.EQUALIZE, 0, 0.0)]
COMBOS = list(itertools.product((False, True), repeat=5))  # (fmt, colors, tones, warps, enhances)


@pytest.fixture(scope="module")
def batch():
    imgs = [synth(61, 97, 3, 900 + k) for k in range(5)] + [synth(80, 300, 3, 905), synth(375, 500, 3, 906)]
    # (windows 0 and 2 from packed rows of 291 bytes: no wave kernel reads a stride that is no multiple of 4)
    src = Sources(imgs, GEOMS, src_align=[1, 16, 1, 16, 16, 16, 16])
    plain = src.plain_u8()
    assert all(p.any() for p in plain)
    yield src, plain
    src.free()


def test_the_batch_mixes_wave_and_other_images(batch):
    """So the format-alone call mixes images the resize launch formats with
    images the second pass formats."""
    src, _ = batch
    plans = [capi.describe_plan(e) for e in src.entries([(256, g[4] * 3) for g in GEOMS])]
    assert plans[6]["wave"] == 1
    assert any(p["wave"] == 0 for p in plans[:6])


def _expected(q, k, fmt, colors, tones, warps, enhances):
    p = q
    if warps:
        p = capi.warp_apply_u8(p, WARPS[k])
    if enhances:
        p = capi.enhance_apply_u8(p, ENHANCES[k])
    if tones:
        p = T.apply(p, TONES[k])
    if colors:
        p = C.apply_ref(p, C.eight_matrices()[k])
    if not fmt:
        return p
    return expect(expected_table(BF16_CHW[1], 3, IMAGENET_MEAN, IMAGENET_STD), p)


def _launch(src, dsts, fmt, colors, tones, warps, enhances):
    """The C entry point the combination maps to, every absent member null."""
    arr, n = capi.make_images(src.entries(dsts.pairs()))
    c = capi.make_colors(C.eight_matrices()[:n]) if colors else None
    t = capi.make_tones(TONES) if tones else None
    w = capi.make_warps(WARPS) if warps else None
    e = capi.make_enhances(ENHANCES) if enhances else None
    if enhances:
        capi.resize_crop_batch_enhance(arr, w, e, t, c, n, dsts.dtype(), dsts.fmt(), 0, None)
    elif warps:
        capi.resize_crop_batch_warp(arr, w, t, c, n, dsts.dtype(), dsts.fmt(), 0, None)
    elif tones:
        capi.resize_crop_batch_tone(arr, t, c, n, dsts.dtype(), dsts.fmt(), 0, None)
    elif colors:
        capi.resize_crop_batch_color(arr, c, n, dsts.dtype(), dsts.fmt(), 0, None)
    elif fmt:
        capi.resize_crop_batch_fmt(arr, n, dsts.fmt(), 0, None)
    else:
        capi.resize_crop_batch(arr, n, capi.MXD_U8, 0, None)


@pytest.mark.parametrize("combo", COMBOS, ids=["".join(c for c, on in zip("fctwe", combo) if on) or "plain" for combo in COMBOS])
def test_every_combination_of_the_five_members(batch, combo):
    src, plain = batch
    dsts = Dsts(GEOMS, BF16_CHW if combo[0] else U8)
    try:
        dsts.clear()
        _launch(src, dsts, *combo)
        capi.check(capi.lib().mxd_device_synchronize(0))
        outs, clean = dsts.read()
    finally:
        dsts.free()
    for k, (o, q, ok) in enumerate(zip(outs, plain, clean)):
        e = _expected(q, k, *combo)
        assert o.shape == e.shape and o.dtype == e.dtype, (combo, k)
        bad = int((o != e).sum())
        assert bad == 0, (combo, k, bad, np.argwhere(o != e)[:3])
        assert ok, (combo, k, "bytes outside the image were written")
    if combo[4] and not (combo[1] or combo[2] or combo[3]):
        # the stage did something: SHARPNESS 1.9 on the windows with an interior
        for k in (4, 5):
            assert not np.array_equal(_expected(plain[k], k, combo[0], False, False, False, False), outs[k])
