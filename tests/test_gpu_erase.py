"""GPU: the erase calls of the C ABI (mxd_resize_crop_batch_erase and its
host-source / JPEG counterparts).  The expectation is always the same call
without erases (every count 0, itself asserted equal to the call that has no
erases member) with the boxes replaced by the CPU statement's elements
(mxd_erase_apply, held to tests/erase_ref.py by tests/test_erase.py).  Every
comparison is of integer bits, and every byte of a destination buffer outside
the image's elements must keep the 0xff it was filled with."""
import os

import numpy as np
import pytest

import erase_ref as R
import mix_ref as M
from gpu_util import synth
from mlx_data_amd import capi
from test_gpu_color import F32, FORMATTED, U8, Dsts, Sources

pytestmark = pytest.mark.gpu

F16_HWC, BF16_CHW = FORMATTED[2], FORMATTED[5]
FORMS = [U8, F32, F16_HWC, BF16_CHW]
ELEM = {U8[0]: capi.MXD_ERASE_U8, F32[0]: capi.MXD_ERASE_F32, F16_HWC[0]: capi.MXD_ERASE_F16, BF16_CHW[0]: capi.MXD_ERASE_BF16}

# Crop windows: 1x1; 5x7; 65x17 (17 quads a row: a unit of 256 items ends inside
# a row); 130x33 (several units a box); a second 65x17 that is never erased.
GEOMS = [(40, 36, 3, 5, 1, 1, 0), (40, 36, 3, 5, 5, 7, 0), (90, 60, 7, 2, 65, 17, 0), (90, 60, 2, 9, 65, 17, 1),
         (150, 40, 9, 3, 130, 33, 0)]


def boxes_of(w, h, which):
    if which == "window":  # the box equal to the window
        return [(0, 0, w, h)]
    if which == "inner":  # x 1..4 of the 5x7: partial quads on both sides, no interior quad
        return [(min(1, w), min(1, h), min(4, w), h)]
    if which == "empty":
        return [(min(3, w), 0, min(3, w), h)]
    if which == "two":  # overlapping, edges inside quads
        return [(0, 0, max(1, w - 3), max(1, h - 2)), (w // 3, h // 3, w, h)]
    return [(0, 0, w - w // 4, h - h // 4), (w // 5, h // 4, w, h - 1), (w // 2, 0, w // 2 + max(1, w // 7), h),
            (max(0, w // 2 - 2), h // 2, min(w, w // 2 + 6), h // 2 + 1)]  # four


def erases_of(mode, which, seed=(11, 12)):
    """One entry per image of GEOMS; image 3 (between erased ones) has count 0."""
    return [None if k == 3 else (mode, boxes_of(g[4], g[5], which), seed, (3.0, 250.0, 17.0))
            for k, g in enumerate(GEOMS)]


@pytest.fixture(scope="module")
def windows():
    imgs = [synth(80, 300, 3, 800 + k) if g[4] == 130 else synth(61, 97, 3, 800 + k) for k, g in enumerate(GEOMS)]
    src = Sources(imgs, GEOMS)
    yield src
    src.free()


def _launch(src, dsts, erases, mixes=None, stream=None):
    arr, n = capi.make_images(src.entries(dsts.pairs()))
    capi.resize_crop_batch_erase(arr, None, None, None, None, capi.make_mixes(mixes) if mixes else None,
                                 capi.make_erases(erases), n, dsts.dtype(), dsts.fmt(), 0,
                                 stream.handle if stream else None)
    capi.check(capi.lib().mxd_device_synchronize(0))


def _expected(base, erases, mode):
    out = [b.copy() for b in base]
    for o, e in zip(out, erases):
        if e is not None:
            capi.erase_apply(o, e, ELEM[mode[0]])
    return out


def _check(src, erases, mode, tag, base=None, mixes=None, **kw):
    dsts = Dsts(src.geoms, mode, **kw)
    try:
        if base is None:
            dsts.clear()
            _launch(src, dsts, [None] * len(erases), mixes)
            base = dsts.read()[0]
        dsts.clear()
        _launch(src, dsts, erases, mixes)
        outs, clean = dsts.read()
    finally:
        dsts.free()
    for k, (o, e, ok) in enumerate(zip(outs, _expected(base, erases, mode), clean)):
        bad = int((o != e).sum())
        assert bad == 0, (tag, mode[0], k, erases[k], bad, np.argwhere(o != e)[:3])
        assert ok, (tag, mode[0], k, "bytes outside the image were written")
    return outs, base


@pytest.mark.parametrize("which", ["window", "inner", "empty", "two", "four"])
@pytest.mark.parametrize("emode", [R.CONST, R.COLOR, R.PIXEL], ids=["const", "color", "pixel"])
@pytest.mark.parametrize("mode", FORMS, ids=[m[0] for m in FORMS])
def test_boxes_in_every_output_form(windows, mode, emode, which):
    if mode is U8 and emode != R.CONST:
        with pytest.raises(capi.MxdError, match="needs a float element type"):
            _check(windows, erases_of(emode, which), mode, which, base=[])
        return
    outs, base = _check(windows, erases_of(emode, which), mode, which)
    assert np.array_equal(outs[3], base[3])  # count 0
    if which == "empty":
        assert all(np.array_equal(o, b) for o, b in zip(outs, base))
    if which == "window":
        assert all((o != b).any() for o, b in zip(outs[:3], base))


def test_a_call_without_erased_images_is_the_formatted_call(windows):
    for mode in (U8, BF16_CHW):
        dsts = Dsts(GEOMS, mode)
        try:
            dsts.clear()
            _launch(windows, dsts, [None] * len(GEOMS))
            ours = dsts.read()[0]
            dsts.clear()
            arr, n = capi.make_images(windows.entries(dsts.pairs()))
            if mode is U8:
                capi.resize_crop_batch(arr, n, capi.MXD_U8, 0, None)
            else:
                capi.resize_crop_batch_fmt(arr, n, dsts.fmt(), 0, None)
            capi.check(capi.lib().mxd_device_synchronize(0))
            assert all(np.array_equal(a, b) for a, b in zip(ours, dsts.read()[0]))
        finally:
            dsts.free()


@pytest.mark.parametrize("mode,kw", [(U8, dict(dst_pad=2, dst_shift=1)), (F32, dict(dst_pad=1, dst_shift=1)),
                                     (F16_HWC, dict(dst_pad=1, dst_shift=1)), (BF16_CHW, dict(dst_pad=1, dst_shift=1)),
                                     (BF16_CHW, dict(plane_pad=3))],
                         ids=["u8", "f32", "f16", "bf16 chw", "bf16 chw odd planes"])
def test_misaligned_destinations_take_the_element_stores(windows, mode, kw):
    _check(windows, erases_of(R.CONST if mode is U8 else R.PIXEL, "four"), mode, "misaligned", **kw)


def test_erase_behind_a_mixup(windows):
    n = len(GEOMS)
    mixes = [M.entry_mixup(3 if k == 2 else 2 if k == 3 else k, 0.3) for k in range(n)]
    outs, base = _check(windows, erases_of(R.PIXEL, "two"), BF16_CHW, "mix", mixes=mixes)
    plain = _check(windows, [None] * n, BF16_CHW, "no mix")[1]
    assert not np.array_equal(base[2], plain[2])  # (the mix did something)


def test_two_calls_on_one_stream_that_differ_in_seed_only(windows):
    dsts = Dsts(GEOMS, F32)
    stream = capi.Stream(0)
    try:
        dsts.clear()
        _launch(windows, dsts, [None] * len(GEOMS), stream=stream)
        base, seen = dsts.read()[0], []
        for seed in ((1, 2), (1, 3), (1, 2)):
            erases = erases_of(R.PIXEL, "two", seed)
            _launch(windows, dsts, erases, stream=stream)
            outs = dsts.read()[0]
            assert all(np.array_equal(o, e) for o, e in zip(outs, _expected(base, erases, F32))), seed
            seen.append(outs[4].tobytes())
        assert seen[0] == seen[2] != seen[1]
    finally:
        stream.close()
        dsts.free()


def test_host_and_jpeg_sources():
    imgs = [synth(120, 160, 3, 60 + k) for k in range(2)]
    geoms = [(80, 60, 5, 3, 70, 41, k) for k in range(2)]
    erases = [(R.PIXEL, [(3, 2, 66, 40), (30, 0, 41, 41)], (8, 9)), (R.COLOR, [(0, 0, 70, 41)], (8, 9))]
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz"))
    coefs = [capi.JpegCoefs(gold[k]) for k in ("sub2_prog0_jpg", "caltech_300x200_jpg")]
    jgeoms = [(60, 44, 3, 1, 53, 41, 1), (120, 80, 11, 5, 53, 41, 0)]
    jerases = [(R.PIXEL, [(1, 1, 52, 40)], (8, 9)), None]
    host_d, jpeg_d = Dsts(geoms, BF16_CHW), Dsts(jgeoms, BF16_CHW)
    try:
        for dsts, er, make, call, ents in (
                (host_d, erases, capi.make_images, capi.resize_crop_to_device_erase,
                 lambda pairs: [dict(src=imgs[k].ctypes.data, src_stride=160 * 3, src_w=160, src_h=120, channels=3,
                                     resize_w=80, resize_h=60, crop_x=5, crop_y=3, crop_w=70, crop_h=41, flip=k, dst=p,
                                     dst_stride=dp) for k, (p, dp) in enumerate(pairs)]),
                (jpeg_d, jerases, capi.make_jpeg_images, capi.jpeg_resize_crop_to_device_erase,
                 lambda pairs: [dict(coefs=c, resize_w=g[0], resize_h=g[1], crop_x=g[2], crop_y=g[3], crop_w=g[4],
                                     crop_h=g[5], flip=g[6], dst=p, dst_stride=dp)
                                for c, g, (p, dp) in zip(coefs, jgeoms, pairs)])):
            got = []
            for e in ([None] * 2, er):
                dsts.clear()
                arr, n = make(ents(dsts.pairs()))
                call(arr, None, None, None, None, None, capi.make_erases(e), n, dsts.dtype(), dsts.fmt(), 0)
                got.append(dsts.read())
            (base, _), (outs, clean) = got
            assert all(np.array_equal(o, x) for o, x in zip(outs, _expected(base, er, BF16_CHW))) and all(clean)
            assert not np.array_equal(outs[0], base[0])
    finally:
        host_d.free(), jpeg_d.free()
        for c in coefs:
            c.close()
