"""GPU: the arithmetic-domain sweeps of tests/stage_domains.py through the device
calls of the C ABI, on crop-only plans (resize to the source size), so the bytes
that reach a stage are the bytes the builder chose: plain_u8() is asserted equal
to the input first.  The expectation is Pillow itself for the tone, warp and
enhance stages and the NumPy statements (tests/*_ref.py) for colour, Gaussian
blur and mix; everything is compared as integer bits, and every byte of a
destination buffer outside the image's elements must keep the 0xff it was filled
with.  Every builder property relied on here is asserted, without a device, by
tests/test_stage_domains.py.  Sources / Dsts are test_gpu_color.py's."""
import numpy as np
import pytest

import blur_ref as B
import color_ref as C
import enhance_ref as E
import mix_ref as M
import stage_domains as S
import tone_ref as T
import warp_ref as W
from mlx_data_amd import capi
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expect, expected_table
from test_gpu_color import FORMATTED, U8, Dsts, Sources

pytestmark = pytest.mark.gpu

BF16_CHW = FORMATTED[5]
ODD = dict(dst_pad=2, plane_pad=2, dst_shift=1)  # destinations that force element stores


def _device(images, launch, mode=U8, **kw):
    """The results of launch(arr, n, dsts) on the crop-only plans of `images`."""
    images = list(images)
    src = Sources(images, S.geoms(images))
    try:
        plain = src.plain_u8()
        assert all(np.array_equal(p, i) for p, i in zip(plain, images)), "a crop-only plan changed its bytes"
        dsts = Dsts(src.geoms, mode, **kw)
        try:
            dsts.clear()
            arr, n = capi.make_images(src.entries(dsts.pairs()))
            launch(arr, n, dsts)
            capi.check(capi.lib().mxd_device_synchronize(0))
            outs, clean = dsts.read()
        finally:
            dsts.free()
    finally:
        src.free()
    assert all(clean), "bytes outside the images were written"
    return outs


def _same(outs, wants, tags):
    assert len(outs) == len(wants)
    for o, e, tag in zip(outs, wants, tags):
        assert o.shape == e.shape and o.dtype == e.dtype, tag
        assert np.array_equal(o, e), (tag, int((o != e).sum()), np.argwhere(o != e)[:3])


def _formatted(mode, p):
    return p if mode[1] is None else expect(expected_table(mode[1], 3, IMAGENET_MEAN, IMAGENET_STD), p)


def _tone(images, tones, tags):
    outs = _device(images, lambda arr, n, d: capi.resize_crop_batch_tone(arr, capi.make_tones(tones), None, n, d.dtype(), d.fmt(), 0, None))
    _same(outs, [T.pillow_apply(i, t) for i, t in zip(images, tones)], tags)
    return outs


# ---- 1. tone tables over their whole domain ----------------------------------------------------

@pytest.mark.parametrize("chunk", S.autocontrast_chunks(), ids=lambda c: f"{c[0]}-{c[1]}")
def test_autocontrast_every_lo_hi(chunk):
    """One call per chunk of at most 1,024 16 x 16 images, three (lo, hi) pairs an image."""
    imgs, pairs = S.autocontrast_images()
    a, b = chunk
    _tone(imgs[a:b], [(T.AUTOCONTRAST, 0, 0.0)] * (b - a), [(n, pairs[n].tolist()) for n in range(a, b)])


@pytest.mark.parametrize("factor", S.contrast_factors())
def test_contrast_every_rounded_mean_and_the_rounding_boundary(factor):
    means = S.contrast_mean_images()
    imgs, tags = [means[m][0] for m in range(256)], [("mean", m) for m in range(256)]
    for k, on, below in S.contrast_tie_images():
        imgs += [on, below]
        tags += [("tie", k, on.shape), ("below the tie", k, on.shape)]
    _tone(imgs, [(T.CONTRAST, 0, factor)] * len(imgs), tags)


def test_equalize_histograms():
    cases = S.equalize_cases()
    outs = _tone([v[0] for v in cases.values()], [(T.EQUALIZE, 0, 0.0)] * len(cases), list(cases))
    for (name, (img, steps)), o in zip(cases.items(), outs):
        for c, (step, bins) in enumerate(steps):
            if step == 0 or bins <= 1:
                assert np.array_equal(o[..., c], img[..., c]), (name, c)


def test_every_posterize_and_solarize_argument():
    tones = S.poster_solar_tones()
    _tone([S.all_bytes_image()] * len(tones), tones, tones)


# ---- 2. encode ties and saturation of the colour map -----------------------------------------

@pytest.mark.parametrize("kw", [{}, ODD], ids=["aligned", "element-stores"])
@pytest.mark.parametrize("mode", [U8, BF16_CHW], ids=["u8", "bfloat16-chw"])
def test_encode_ties_and_saturation(mode, kw):
    mats = S.tie_matrices()
    img = S.all_bytes_image()
    outs = _device([img] * len(mats), lambda arr, n, d: capi.resize_crop_batch_color(arr, capi.make_colors(mats), n, d.dtype(), d.fmt(), 0, None),
                   mode, **kw)
    _same(outs, [_formatted(mode, C.apply_ref(img, m)) for m in mats], range(len(mats)))


# ---- 3. contraction witnesses ---------------------------------------------------------------------

def test_colour_witnesses():
    """The triples of every row of the three twists and NEGATIVE at which a fused multiply-add
    changes a byte."""
    images, mats, tags = [], [], []
    for name, imgs in S.color_witness_images().items():
        for img in imgs:
            images.append(img), mats.append(S.color_matrices()[name]), tags.append(name)
    outs = _device(images, lambda arr, n, d: capi.resize_crop_batch_color(arr, capi.make_colors(mats), n, d.dtype(), d.fmt(), 0, None))
    _same(outs, [C.apply_ref(i, m) for i, m in zip(images, mats)], tags)


def test_mixup_witnesses():
    lam = next(lam for lam in S.MIX_LAMS if len(S.mix_witnesses()[(lam, "FULL")][1]))
    own, partner = S.mix_witness_images(lam)
    mixes = [M.entry_mixup(1, lam), M.entry_mixup(0, lam)]
    outs = _device([own, partner], lambda arr, n, d: capi.resize_crop_batch_mix(arr, None, None, None, None, capi.make_mixes(mixes), n, d.dtype(),
                                                                                 d.fmt(), 0, None))
    _same(outs, [M.mixup(own, partner, lam), M.mixup(partner, own, lam)], ["own", "partner"])


def _enhance(images, enhs, wants, tags):
    outs = _device(images, lambda arr, n, d: capi.resize_crop_batch_enhance(arr, None, capi.make_enhances(enhs), None, None, n, d.dtype(),
                                                                           d.fmt(), 0, None))
    _same(outs, wants, tags)


def test_blend_witnesses():
    found = S.blend_witnesses()
    images, enhs = [v[0] for v in found.values()], list(found)
    _enhance(images, enhs, [E.pillow_apply(i, e) for i, e in zip(images, enhs)], enhs)


@pytest.mark.parametrize("mode", [W.BILINEAR, S.CUBIC], ids=["bilinear", "bicubic"])
def test_warp_witnesses(mode):
    found = S.bilinear_witnesses() if mode == W.BILINEAR else S.bicubic_witnesses()
    images, warps, tags = [], [], []
    for name, cases in found.items():
        for img, x, y, names in cases:
            images.append(img), warps.append((mode, S.FILL, S.warp_matrices()[name])), tags.append((name, x, y))
    outs = _device(images, lambda arr, n, d: capi.resize_crop_batch_warp(arr, capi.make_warps(warps), None, None, n, d.dtype(), d.fmt(), 0, None))
    _same(outs, [S._pillow_warp(i, mode, w[2]) for i, w in zip(images, warps)], tags)


@pytest.mark.parametrize("k,sigma", S.BLUR_KERNELS)
def test_blur_witnesses(k, sigma):
    cases, _ = S.blur_witnesses(capi.gaussian_weights(sigma, k), 5)
    images = [c[0] for c in cases]
    _enhance(images, [(capi.MXD_ENHANCE_GAUSSIAN_BLUR, sigma, k)] * len(images), [B.blur_f32(i, k, sigma) for i in images],
             [c[1:] for c in cases])
