"""GPU: the tone calls of the C ABI (mxd_resize_crop_batch_tone and its
host-source / JPEG counterparts).  The expectation is always the NumPy
restatement of the tone tables (tests/tone_ref.py) applied to the u8 result of
the same call without tone, then the NumPy expression of the colour map
(tests/color_ref.py) when the call has matrices, then the format table
(out_format_util.expected_table).  Everything is compared as integer bits, and
every byte of a destination buffer outside the image's elements must keep the
0xff it was filled with.  Sources / Dsts are test_gpu_color.py's."""
import os

import numpy as np
import pytest

import color_ref as C
import tone_ref as T
from gpu_util import synth
from mlx_data_amd import capi
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expect, expected_table
from test_gpu_color import F32, FORMATTED, MODES, U8, Dsts, Sources

pytestmark = pytest.mark.gpu

BF16_CHW = FORMATTED[5]
# one of every op, with parameters (op, arg, factor)
SIX = [(T.NONE, 0, 0.0), (T.POSTERIZE, 3, 0.0), (T.SOLARIZE, 100, 0.0), (T.AUTOCONTRAST, 0, 0.0), (T.EQUALIZE, 0, 0.0),
       (T.CONTRAST, 0, 1.3)]


def _tid(t):
    return f"{T.NAMES[t[0]]}-{t[1] if t[0] in (T.POSTERIZE, T.SOLARIZE) else t[2]}"


def _expected(mode, q, tone, m=None):
    """What the call must write for u8 result bytes q under tone, then matrix m."""
    p = T.apply(q, tone)
    if m is not None:
        p = C.apply_ref(p, m)
    if mode[1] is None:
        return p
    mean, std = (IMAGENET_MEAN, IMAGENET_STD) if mode[3] else (None, None)
    return expect(expected_table(mode[1], 3, mean, std), p)


def _launch(src, dsts, tones, mats=None, stream=None):
    arr, n = capi.make_images(src.entries(dsts.pairs()))
    capi.resize_crop_batch_tone(arr, capi.make_tones(tones), capi.make_colors(mats) if mats is not None else None, n,
                                dsts.dtype(), dsts.fmt(), 0, stream.handle if stream else None)
    if stream:
        stream.synchronize()


def _compare(outs, clean, plain, tones, mats, mode, tag):
    for k, (o, q, t, ok) in enumerate(zip(outs, plain, tones, clean)):
        e = _expected(mode, q, t, mats[k] if mats is not None else None)
        assert o.shape == e.shape and o.dtype == e.dtype, (tag, mode[0], k)
        bad = int((o != e).sum())
        assert bad == 0, (tag, mode[0], k, _tid(t), bad, np.argwhere(o != e)[:3])
        assert ok, (tag, mode[0], k, "bytes outside the image were written")


def _check(src, plain, tones, mode, tag, mats=None, **kw):
    dsts = Dsts(src.geoms, mode, **kw)
    try:
        dsts.clear()
        _launch(src, dsts, tones, mats)
        capi.check(capi.lib().mxd_device_synchronize(0))
        outs, clean = dsts.read()
    finally:
        dsts.free()
    _compare(outs, clean, plain, tones, mats, mode, tag)
    return outs


# ---- the smallest windows that can go wrong -------------------------------------------

@pytest.fixture(scope="module")
def windows():
    """Crop windows 5x7, 31x29 (w mod 4 != 0, rows that are no 16-byte
    multiple), 64x8 (one row group of every kernel) and 70x41 (three tone_hist
    workgroups add into one statistics block, six pixel_rows workgroups), the
    second mirrored."""
    imgs = [synth(61, 97, 3, 700 + k) for k in range(4)]
    geoms = [(40, 36, 3, 5, 5, 7, 0), (40, 36, 1, 3, 31, 29, 1), (80, 50, 9, 11, 64, 8, 0), (90, 60, 7, 2, 70, 41, 0)]
    src = Sources(imgs, geoms)
    plain = src.plain_u8()
    assert all(p.any() for p in plain)
    yield src, plain
    src.free()


ALL_OPS = ([(T.NONE, 0, 0.0)] + [(T.POSTERIZE, b, 0.0) for b in (1, 4, 8)] +
           [(T.SOLARIZE, t, 0.0) for t in (0, 128, 256)] + [(T.AUTOCONTRAST, 0, 0.0), (T.EQUALIZE, 0, 0.0)] +
           [(T.CONTRAST, 0, f) for f in (0.0, 0.5, 1.0, 1.9)])


@pytest.mark.parametrize("tone", ALL_OPS, ids=[_tid(t) for t in ALL_OPS])
def test_every_op_in_u8(windows, tone):
    src, plain = windows
    outs = _check(src, plain, [tone] * 4, U8, "windows")
    if tone[0] == T.NONE or tone == (T.POSTERIZE, 8, 0.0) or tone == (T.SOLARIZE, 256, 0.0) or tone == (T.CONTRAST, 0, 1.0):
        assert all(np.array_equal(o, q) for o, q in zip(outs, plain))  # the identities
    else:
        assert not all(np.array_equal(o, q) for o, q in zip(outs, plain))


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("tone", [SIX[4], SIX[5]], ids=["equalize", "contrast"])
def test_every_output_form_with_destinations_that_force_element_stores(windows, tone, mode):
    """Bases one element past a 256-byte boundary, padded rows and planes, and
    a matrix per image behind the table; the same destinations without a
    matrix (the kernel that skips the map, on its element stores)."""
    src, plain = windows
    mats = C.eight_matrices()[1:5]
    _check(src, plain, [tone] * 4, mode, "odd", mats, dst_pad=2, plane_pad=2, dst_shift=1)
    _check(src, plain, [tone] * 4, mode, "aligned")
    _check(src, plain, [tone] * 4, mode, "odd, no matrix", None, dst_pad=2, plane_pad=2, dst_shift=1)


def test_one_image(windows):
    src, plain = windows
    one = Sources(src.images[3:], src.geoms[3:])
    try:
        _check(one, plain[3:], [SIX[4]], U8, "n=1")
        _check(one, plain[3:], [SIX[5]], BF16_CHW, "n=1", [C.NEGATIVE])
    finally:
        one.free()


# ---- the images every lane of which hits one bin, and the min(255) ------------------

def test_constant_two_level_and_sparse_images_through_crop_only_plans():
    """Resize to the source size is the identity, so the result bytes are the
    source's: a constant image (one bin: the identity branches), two levels
    (every lane of a wave adds to one of two bins) and zeros with five pixels
    of 255 (EQUALIZE overshoots 255 without the min)."""
    imgs = [np.full((24, 40, 3), 77, np.uint8), T.two_level(16, 16), T.zeros_five(), T.two_level(40, 36)]
    geoms = [(40, 24, 0, 0, 40, 24, 0), (16, 16, 0, 0, 16, 16, 0), (20, 20, 0, 0, 20, 20, 0), (36, 40, 3, 2, 30, 35, 1)]
    src = Sources(imgs, geoms)
    try:
        plain = src.plain_u8()
        assert np.array_equal(plain[0], imgs[0]) and np.array_equal(plain[1], imgs[1]) and np.array_equal(plain[2], imgs[2])
        for tone in (SIX[3], SIX[4], SIX[5], (T.CONTRAST, 0, 0.5)):
            outs = _check(src, plain, [tone] * 4, U8, "edge")
            if tone[0] in (T.AUTOCONTRAST, T.EQUALIZE):
                assert np.array_equal(outs[0], imgs[0])  # one bin: the identity
        eq = _check(src, plain, [SIX[4]] * 4, U8, "edge")
        assert T.table(imgs[2], SIX[4])[0, 255] == 255 and (eq[2] == 255).sum() == 15 and (eq[2] == 0).sum() == 1185
        ac = _check(src, plain, [SIX[3]] * 4, U8, "edge")
        assert set(np.unique(ac[1])) == {0, 255}
    finally:
        src.free()


# ---- nine images mixing all six ops ---------------------------------------------------

@pytest.mark.parametrize("colored", [False, True], ids=["no-matrix", "matrices"])
@pytest.mark.parametrize("mode", [U8, BF16_CHW], ids=["u8", "bfloat16-chw"])
def test_nine_images_mixing_all_six_ops(mode, colored):
    """A triangle wave image, a Catmull-Rom wave image, general-kernel images
    and small ones, each with its own op and parameters: the launch reorders
    the images by kernel, and op, statistics and table must follow the image."""
    imgs = [synth(150, 200, 3, 1), synth(150, 200, 3, 2), synth(99, 101, 3, 3)] + [synth(61, 97, 3, 10 + k) for k in range(6)]
    geoms = [(120, 90, 7, 3, 101, 80, 0), (120, 90, 7, 3, 101, 80, 1), (75, 70, 3, 2, 61, 33, 1)] + [
        (40, 36, 1 + k, 2, 33 - k, 29 + (k % 2), k % 2) for k in range(6)]
    filters = [0, 1, 0] + [0] * 6
    tones = [SIX[4], SIX[5], SIX[3], SIX[0], SIX[1], (T.SOLARIZE, 60, 0.0), (T.CONTRAST, 0, 0.4), SIX[4], (T.POSTERIZE, 1, 0.0)]
    assert {t[0] for t in tones} == set(range(6))
    mats = (C.eight_matrices() + [C.NEGATIVE]) if colored else None
    src = Sources(imgs, geoms, filters, src_align=[16, 16, 1] + [16] * 6)
    try:
        plain = src.plain_u8()
        outs = _check(src, plain, tones, mode, "nine", mats)
        if mode is U8 and not colored:
            assert np.array_equal(outs[3], plain[3])  # MXD_TONE_NONE
    finally:
        src.free()


# ---- two calls on one stream; the cached descriptor slot -------------------------------

def test_the_second_call_on_a_stream_does_not_see_the_first_call_s_counts(windows):
    """The same shapes, destinations and ops (the same upload: a cache hit and
    the same statistics blocks) over other images."""
    src, plain = windows
    tones = [SIX[4], SIX[5], SIX[3], SIX[4]]
    dsts = Dsts(src.geoms, U8)
    stream = capi.Stream(0)
    try:
        dsts.clear()
        _launch(src, dsts, tones, None, stream)
        _compare(*dsts.read(), plain, tones, None, U8, "first")
        other = [synth(61, 97, 3, 900 + k) for k in range(4)]
        src.upload(other)
        plain2 = src.plain_u8()
        assert not np.array_equal(plain2[3], plain[3])
        for tag in ("second", "third"):
            dsts.clear()
            _launch(src, dsts, tones, None, stream)
            _compare(*dsts.read(), plain2, tones, None, U8, tag)
    finally:
        src.upload(src.images)
        stream.close()
        dsts.free()


def test_cached_descriptors_follow_the_ops_and_parameters(windows):
    """The same images and destinations with other ops, other parameters and
    the first ones again: the uploads differ in the tone fields only."""
    src, plain = windows
    dsts = Dsts(src.geoms, FORMATTED[4])
    stream = capi.Stream(0)
    try:
        a = [SIX[4], SIX[5], SIX[1], SIX[2]]
        b = [SIX[5], SIX[4], (T.POSTERIZE, 5, 0.0), (T.SOLARIZE, 101, 0.0)]
        c = [SIX[3], (T.CONTRAST, 0, 1.4), SIX[0], SIX[4]]
        for tag, tones in (("a", a), ("b", b), ("c", c), ("a again", a)):
            dsts.clear()
            _launch(src, dsts, tones, None, stream)
            _compare(*dsts.read(), plain, tones, None, FORMATTED[4], tag)
    finally:
        stream.close()
        dsts.free()


# ---- host and JPEG sources ----------------------------------------------------------------

def test_host_sources():
    imgs = [synth(120, 160, 3, 40 + k) for k in range(3)]
    geoms = [(80, 60, 5, 3, 70, 41, k % 2) for k in range(3)]
    tones = [SIX[4], SIX[5], SIX[1]]
    mats = [C.NEGATIVE, C.IDENTITY, C.SWAP]

    def entries(pairs):
        return [dict(src=imgs[k].ctypes.data, src_stride=160 * 3, src_w=160, src_h=120, channels=3, resize_w=80,
                     resize_h=60, crop_x=5, crop_y=3, crop_w=70, crop_h=41, flip=geoms[k][6], dst=p, dst_stride=dp)
                for k, (p, dp) in enumerate(pairs)]

    plain_d, dsts = Dsts(geoms, U8), Dsts(geoms, BF16_CHW)
    try:
        arr, n = capi.make_images(entries(plain_d.pairs()))
        capi.resize_crop_to_device(arr, n, capi.MXD_U8, 0)
        plain = plain_d.read()[0]
        dsts.clear()
        arr, n = capi.make_images(entries(dsts.pairs()))
        capi.resize_crop_to_device_tone(arr, capi.make_tones(tones), capi.make_colors(mats), n, dsts.dtype(), dsts.fmt(), 0)
        _compare(*dsts.read(), plain, tones, mats, BF16_CHW, "host")
    finally:
        plain_d.free()
        dsts.free()


def test_jpeg_sources():
    """A 4:2:0 fixture (83x61) and the 300x200 4:2:0 photograph."""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz"))
    names = ["sub2_prog0_jpg", "caltech_300x200_jpg"]
    geoms = [(60, 44, 3, 1, 53, 41, 1), (341 * 3 // 4, 171, 11, 5, 224, 160, 0)]
    coefs = [capi.JpegCoefs(gold[k]) for k in names]
    tones = [SIX[5], SIX[4]]
    plain_d, dsts = Dsts(geoms, U8), Dsts(geoms, F32)

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
        capi.jpeg_resize_crop_to_device_tone(arr, capi.make_tones(tones), None, n, dsts.dtype(), dsts.fmt(), 0)
        _compare(*dsts.read(), plain, tones, None, F32, "jpeg")
    finally:
        plain_d.free()
        dsts.free()
        for c in coefs:
            c.close()
