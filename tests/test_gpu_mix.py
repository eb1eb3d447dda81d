"""GPU: the mix calls of the C ABI (mxd_resize_crop_batch_mix and its
host-source / JPEG counterparts).  The expectation is always the CPU statement
(mxd_mix_apply_u8, asserted equal to timm's NumPy expression of
tests/mix_ref.py) applied to the u8 results of the same call without mixes --
each image's own and its partner's -- then the format table.  Every comparison
is of integer bits, and every byte of a destination buffer outside the image's
elements must keep the 0xff it was filled with."""
import os

import numpy as np
import pytest

import color_ref as C
import enhance_ref as E
import mix_ref as M
import tone_ref as T
import warp_ref as W
from gpu_util import synth
from mlx_data_amd import capi
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expect, expected_table
from test_gpu_color import F32, FORMATTED, U8, Dsts, Sources

pytestmark = pytest.mark.gpu

F16_HWC, BF16_CHW = FORMATTED[2], FORMATTED[5]
FORMS = [U8, F32, F16_HWC, BF16_CHW]
NONE = (M.NONE,)


def _mixed(unmixed, i, entry):
    """The CPU statement's bytes for image i, which must be the NumPy expression's."""
    partner = unmixed[entry[1]] if entry[0] != M.NONE else None
    got = capi.mix_apply_u8(unmixed[i], partner, entry)
    assert np.array_equal(got, M.apply(unmixed, i, entry)), (i, entry)
    return got


def _expected(mode, unmixed, i, entry):
    p = _mixed(unmixed, i, entry)
    if mode[1] is None:
        return p
    mean, std = (IMAGENET_MEAN, IMAGENET_STD) if mode[3] else (None, None)
    return expect(expected_table(mode[1], 3, mean, std), p)


def _members(warps, enhs, tones, mats):
    return (capi.make_warps(warps) if warps is not None else None, capi.make_enhances(enhs) if enhs is not None else None,
            capi.make_tones(tones) if tones is not None else None, capi.make_colors(mats) if mats is not None else None)


def _launch(src, dsts, mixes, warps=None, enhs=None, tones=None, mats=None, stream=None):
    arr, n = capi.make_images(src.entries(dsts.pairs()))
    w, e, t, c = _members(warps, enhs, tones, mats)
    capi.resize_crop_batch_mix(arr, w, e, t, c, capi.make_mixes(mixes), n, dsts.dtype(), dsts.fmt(), 0,
                               stream.handle if stream else None)
    if stream:
        stream.synchronize()


def _unmixed(src, warps=None, enhs=None, tones=None, mats=None):
    """The u8 results of the same call without mixes (the entry point its other members map to)."""
    if warps is None and enhs is None and tones is None and mats is None:
        return src.plain_u8()
    dsts = Dsts(src.geoms, U8)
    try:
        arr, n = capi.make_images(src.entries(dsts.pairs()))
        w, e, t, c = _members(warps, enhs, tones, mats)
        if enhs is not None:
            capi.resize_crop_batch_enhance(arr, w, e, t, c, n, capi.MXD_U8, None, 0, None)
        elif warps is not None:
            capi.resize_crop_batch_warp(arr, w, t, c, n, capi.MXD_U8, None, 0, None)
        elif tones is not None:
            capi.resize_crop_batch_tone(arr, t, c, n, capi.MXD_U8, None, 0, None)
        else:
            capi.resize_crop_batch_color(arr, c, n, capi.MXD_U8, None, 0, None)
        capi.check(capi.lib().mxd_device_synchronize(0))
        return dsts.read()[0]
    finally:
        dsts.free()


def _compare(outs, clean, unmixed, mixes, mode, tag):
    for k, (o, ok) in enumerate(zip(outs, clean)):
        e = _expected(mode, unmixed, k, mixes[k])
        assert o.shape == e.shape and o.dtype == e.dtype, (tag, mode[0], k)
        bad = int((o != e).sum())
        assert bad == 0, (tag, mode[0], k, mixes[k], bad, np.argwhere(o != e)[:3])
        assert ok, (tag, mode[0], k, "bytes outside the image were written")


def _check(src, unmixed, mixes, mode, tag, members=(), **kw):
    dsts = Dsts(src.geoms, mode, **kw)
    try:
        dsts.clear()
        _launch(src, dsts, mixes, *members)
        capi.check(capi.lib().mxd_device_synchronize(0))
        outs, clean = dsts.read()
    finally:
        dsts.free()
    _compare(outs, clean, unmixed, mixes, mode, tag)
    return outs


# ---- the smallest windows that can go wrong -------------------------------------------

# Crop windows 1x1, 3x2 mirrored, 5x7 (lane tails), 65x17 and 130x33 (several
# workgroups per image: 17 and 33 rows, 8 rows a workgroup), each twice and in
# mirror order, so that the partner of i is n - 1 - i; then a third 65x17.
HALF = [(40, 36, 3, 5, 1, 1, 0), (40, 36, 1, 3, 3, 2, 1), (40, 36, 3, 5, 5, 7, 0), (90, 60, 7, 2, 65, 17, 0),
        (150, 40, 9, 3, 130, 33, 0)]
# the second of each pair from another origin (and the 3x2 one not mirrored)
OTHER = [(40, 36, 7, 9, 1, 1, 0), (40, 36, 5, 1, 3, 2, 0), (40, 36, 11, 4, 5, 7, 0), (90, 60, 2, 9, 65, 17, 1),
         (150, 40, 4, 1, 130, 33, 0)]
GEOMS = HALF + OTHER[::-1] + [(90, 60, 11, 20, 65, 17, 0)]
N = len(GEOMS)
REVERSED = [N - 2 - i for i in range(N - 1)] + [N - 1]  # (the eleventh is its own partner)


@pytest.fixture(scope="module")
def windows():
    def source(g, k):
        return synth(80, 300, 3, 700 + k) if g[4] == 130 else synth(61, 97, 3, 700 + k)

    imgs = [source(g, k) for k, g in enumerate(GEOMS)]
    src = Sources(imgs, GEOMS)
    plain = src.plain_u8()
    assert all(plain[i].shape == plain[REVERSED[i]].shape for i in range(N))
    yield src, plain
    src.free()


@pytest.mark.parametrize("mode", FORMS, ids=[m[0] for m in FORMS])
def test_small_windows_with_reversed_partners_in_every_output_form(windows, mode):
    src, plain = windows
    for lam in (0.3, 0.5):
        mixes = [M.entry_mixup(REVERSED[i], lam) for i in range(N)]
        outs = _check(src, plain, mixes, mode, f"mixup {lam}")
    if mode is U8:
        assert not np.array_equal(outs[4], plain[4]) and not np.array_equal(outs[4], plain[5])
    # a box whose edges fall inside a lane's four pixels (clipped to the small windows)
    mixes = [M.entry_cutmix(REVERSED[i], min(1, g[4]), 0, min(7, g[4]), min(5, g[5])) for i, g in enumerate(GEOMS)]
    outs = _check(src, plain, mixes, mode, "cutmix")
    if mode is U8:
        assert np.array_equal(outs[4][:5, 1:7], plain[5][:5, 1:7]) and np.array_equal(outs[4][5:], plain[4][5:])


def test_self_partners_a_chain_and_none_among_them(windows):
    """3 -> 6 -> 10 -> 3 is a chain over the three 65x17 images: each reads
    its partner's unmixed rows, whichever workgroup runs first."""
    src, plain = windows
    mixes = [M.entry_mixup(0, 0.3), NONE, M.entry_cutmix(2, 1, 2, 4, 6), M.entry_mixup(6, 0.3), M.entry_mixup(4, 0.5), NONE,
             M.entry_cutmix(10, 3, 1, 62, 16), M.entry_mixup(2, 0.7), NONE, M.entry_mixup(0, 1.0), M.entry_mixup(3, 0.25)]
    for mode in (U8, BF16_CHW):
        outs = _check(src, plain, mixes, mode, "mixed")
    outs = _check(src, plain, mixes, U8, "mixed")
    assert all(np.array_equal(outs[k], plain[k]) for k in (1, 5, 8, 9))  # NONE, and lam 1
    assert np.array_equal(outs[2], plain[2])  # CutMix with itself
    every_none = _check(src, plain, [NONE] * N, BF16_CHW, "all none")
    table = expected_table(BF16_CHW[1], 3, IMAGENET_MEAN, IMAGENET_STD)
    assert all(np.array_equal(o, expect(table, q)) for o, q in zip(every_none, plain))


BOXES = {  # on the 65x17 and 130x33 windows (indices 3, 4, 5, 6, 10): x0, y0, x1, y1 by (w, h)
    "edges inside quads": lambda w, h: (5, 3, w - 6, h - 2), "from 0": lambda w, h: (0, 0, 7, h),
    "to w": lambda w, h: (w - 9, 1, w, h - 1), "one pixel": lambda w, h: (w - 1, h - 1, w, h),
    "one column in a quad": lambda w, h: (6, 0, 7, h), "full": lambda w, h: (0, 0, w, h),
    "empty columns": lambda w, h: (13, 2, 13, h), "empty rows": lambda w, h: (3, 9, w - 3, 9),
    "a workgroup's last row": lambda w, h: (2, 7, w - 2, 8),
}


@pytest.mark.parametrize("name", list(BOXES))
def test_cutmix_boxes(windows, name):
    src, plain = windows
    mixes = [M.entry_cutmix(REVERSED[i], *BOXES[name](g[4], g[5])) if g[4] >= 65 else NONE for i, g in enumerate(GEOMS)]
    outs = _check(src, plain, mixes, U8, name)
    if name == "full":
        assert np.array_equal(outs[4], plain[5]) and np.array_equal(outs[3], plain[6])
    if name.startswith("empty"):
        assert all(np.array_equal(o, q) for o, q in zip(outs, plain))
    _check(src, plain, mixes, BF16_CHW, name)


@pytest.mark.parametrize("mode,kw", [(U8, dict(dst_pad=2, dst_shift=1)), (U8, dict(dst_pad=4)), (F32, dict(dst_pad=1, dst_shift=1)),
                                     (F16_HWC, dict(dst_pad=1, dst_shift=1)), (BF16_CHW, dict(dst_pad=1, dst_shift=1)),
                                     (BF16_CHW, dict(plane_pad=3))],
                         ids=["u8 odd", "u8 padded", "f32 shifted", "f16 shifted", "bf16 chw shifted", "bf16 chw odd planes"])
def test_misaligned_destinations_take_the_element_stores(windows, mode, kw):
    src, plain = windows
    mixes = [M.entry_mixup(REVERSED[i], 0.3) if i % 3 else M.entry_cutmix(REVERSED[i], 0, 0, min(3, g[4]), g[5])
             for i, g in enumerate(GEOMS)]
    _check(src, plain, mixes, mode, "misaligned", **kw)


# ---- every byte pair ---------------------------------------------------------------------------

@pytest.mark.parametrize("lam", [0.3, 0.5])
def test_every_byte_pair_on_the_device(lam):
    """Two 256 x 256 crop-only images hold every (own, partner) pair; at 0.3 a
    fused multiply-add, at 0.5 rounding half up would differ (tests/test_mix.py)."""
    q, r = M.byte_pair_grid()
    src = Sources([q, r], [(256, 256, 0, 0, 256, 256, 0)] * 2)
    try:
        plain = src.plain_u8()
        assert np.array_equal(plain[0], q) and np.array_equal(plain[1], r)  # crop-only plans are exact copies
        mixes = [M.entry_mixup(1, lam), M.entry_mixup(0, lam)]
        outs = _check(src, plain, mixes, U8, "grid")
        assert np.array_equal(outs[0], M.mixup(q, r, lam)) and np.array_equal(outs[1], M.mixup(r, q, lam))
    finally:
        src.free()


def test_weights_that_do_not_sum_to_one_saturate_at_255_on_the_device():
    """The header's min(rint(x), 255), as the CPU statement (tests/test_mix.py)."""
    q, r = M.byte_pair_grid()
    src = Sources([q, r], [(256, 256, 0, 0, 256, 256, 0)] * 2)
    try:
        plain = src.plain_u8()
        mixes = [(M.MIXUP, 1, 1.0, 1.0), (M.MIXUP, 0, 1.0, 0.5)]
        outs = _check(src, plain, mixes, U8, "saturate")
        assert np.array_equal(outs[0], np.minimum(q.astype(np.int32) + r, 255).astype(np.uint8))
    finally:
        src.free()


# ---- chains of one to four stages: the mix stage reads rows A, B, A, B ---------------------------

def test_chains_of_one_to_four_stages(windows):
    src, plain = windows
    geoms = src.geoms
    warps = [(W.BILINEAR, (255, 0, 30), W.rotate_matrix(g[4], g[5], 30.0)) for g in geoms]
    enhs = [(E.SHARPNESS, 1.9) if k % 2 else (E.COLOR, 0.3) for k in range(N)]
    tones = [(T.EQUALIZE, 0, 0.0) if k % 3 else (T.POSTERIZE, 3, 0.0) for k in range(N)]
    mats = (C.eight_matrices() * 2)[1:1 + N]
    mixes = [M.entry_mixup(REVERSED[i], 0.3) if i % 2 else M.entry_cutmix(REVERSED[i], 0, 0, (g[4] + 1) // 2, g[5])
             for i, g in enumerate(geoms)]
    seen = []
    for tag, members in (("mix alone", (None, None, None, None)), ("colour", (None, None, None, mats)),
                         ("enhance and tone", (None, enhs, tones, None)), ("all four", (warps, enhs, tones, mats))):
        unmixed = _unmixed(src, *members)
        for mode in (U8, BF16_CHW):
            outs = _check(src, unmixed, mixes, mode, tag, members)
        seen.append(unmixed[4].tobytes())
    assert len(set(seen)) == 4  # (the members did something)
    # a format with a warp alone: no second pass, the mix stage writes the format
    unmixed = _unmixed(src, warps)
    _check(src, unmixed, mixes, F16_HWC, "warp and format", (warps, None, None, None))


# ---- partners whose rows come from different resize kernels ----------------------------------------

ROUTE_GEOMS = [(341, 256, 58, 16, 224, 224, 0), (341, 256, 57, 15, 224, 224, 1), (40, 40, 0, 0, 40, 40, 0),
               (40, 40, 0, 0, 40, 40, 0)]


@pytest.mark.parametrize("policy", [capi.MXD_POLICY_AUTO, capi.MXD_POLICY_PREFER_BAND], ids=["auto", "prefer band"])
def test_partners_from_the_wave_band_and_general_kernels(policy):
    """tests/test_gpu_stage_chain.py's wave image (500x375 -> 341x256, crop
    224x224) beside the same window from packed rows of 1503 bytes (no wave
    or band kernel reads a stride that is no multiple of 4: the general
    kernel), and 600 -> 40 (wave; band when preferred) beside 680 -> 40
    (general)."""
    imgs = [synth(375, 500, 3, 906), synth(375, 501, 3, 907), synth(600, 600, 3, 908), synth(680, 680, 3, 909)]
    src = Sources(imgs, ROUTE_GEOMS, src_align=[16, 1, 16, 16])
    old = capi.set_kernel_policy(policy)
    try:
        entries = src.entries([(256, g[4] * 3) for g in ROUTE_GEOMS])
        waves = [capi.describe_plan(e)["wave"] for e in entries]
        bands = [capi.describe_band_plan(e)["band"] for e in entries]
        assert waves[0] == 1 and waves[2] == 1 and bands[0] == 1 and bands[2] == 1  # band first when preferred
        assert (waves[1], bands[1], waves[3], bands[3]) == (0, 0, 0, 0)
        plain = src.plain_u8()
        mixes = [M.entry_mixup(1, 0.3), M.entry_cutmix(0, 30, 50, 190, 170), M.entry_cutmix(3, 3, 3, 37, 37),
                 M.entry_mixup(2, 0.5)]
        _check(src, plain, mixes, U8, "routes")
        _check(src, plain, mixes, BF16_CHW, "routes")
    finally:
        capi.set_kernel_policy(old)
        src.free()


# ---- two calls on a stream of its own ----------------------------------------------------------------

def test_two_calls_on_one_stream_with_other_mixes(windows):
    """The same shapes and destinations: the uploads differ in the mixes only,
    so a cached descriptor slot must not serve the other call."""
    src, plain = windows
    dsts = Dsts(src.geoms, U8)
    stream = capi.Stream(0)
    try:
        a = [M.entry_mixup(REVERSED[i], 0.3) for i in range(N)]
        b = [M.entry_mixup(REVERSED[i], 0.5) for i in range(N)]
        c = [M.entry_mixup(i, 0.3) for i in range(N)]
        d = [M.entry_cutmix(REVERSED[i], 0, 0, 1, 1) for i in range(N)]
        for tag, mixes in (("a", a), ("b", b), ("c", c), ("d", d), ("a again", a)):
            dsts.clear()
            _launch(src, dsts, mixes, stream=stream)
            _compare(*dsts.read(), plain, mixes, U8, tag)
    finally:
        stream.close()
        dsts.free()


# ---- host and JPEG sources ----------------------------------------------------------------

def test_host_sources():
    imgs = [synth(120, 160, 3, 60 + k) for k in range(3)]
    geoms = [(80, 60, 5, 3, 70, 41, k % 2) for k in range(3)]
    mixes = [M.entry_mixup(2, 0.3), NONE, M.entry_cutmix(0, 9, 4, 50, 33)]
    tones = [(T.EQUALIZE, 0, 0.0), (T.CONTRAST, 0, 1.3), (T.NONE, 0, 0.0)]

    def entries(pairs):
        return [dict(src=imgs[k].ctypes.data, src_stride=160 * 3, src_w=160, src_h=120, channels=3, resize_w=80,
                     resize_h=60, crop_x=5, crop_y=3, crop_w=70, crop_h=41, flip=geoms[k][6], dst=p, dst_stride=dp)
                for k, (p, dp) in enumerate(pairs)]

    plain_d, toned_d, dsts, dsts8 = Dsts(geoms, U8), Dsts(geoms, U8), Dsts(geoms, BF16_CHW), Dsts(geoms, U8)
    try:
        arr, n = capi.make_images(entries(plain_d.pairs()))
        capi.resize_crop_to_device(arr, n, capi.MXD_U8, 0)
        plain = plain_d.read()[0]
        arr, n = capi.make_images(entries(toned_d.pairs()))
        capi.resize_crop_to_device_tone(arr, capi.make_tones(tones), None, n, capi.MXD_U8, None, 0)
        toned = toned_d.read()[0]
        dsts.clear()
        arr, n = capi.make_images(entries(dsts.pairs()))
        capi.resize_crop_to_device_mix(arr, None, None, capi.make_tones(tones), None, capi.make_mixes(mixes), n, dsts.dtype(),
                                       dsts.fmt(), 0)
        _compare(*dsts.read(), toned, mixes, BF16_CHW, "host")
        dsts8.clear()
        arr, n = capi.make_images(entries(dsts8.pairs()))
        capi.resize_crop_to_device_mix(arr, None, None, None, None, capi.make_mixes(mixes), n, capi.MXD_U8, None, 0)
        _compare(*dsts8.read(), plain, mixes, U8, "host u8")
    finally:
        for d in (plain_d, toned_d, dsts, dsts8):
            d.free()


def test_jpeg_sources():
    """A 4:2:0 fixture (83x61) and the 300x200 4:2:0 photograph, to one 53x41 window each."""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz"))
    names = ["sub2_prog0_jpg", "caltech_300x200_jpg"]
    geoms = [(60, 44, 3, 1, 53, 41, 1), (120, 80, 11, 5, 53, 41, 0)]
    coefs = [capi.JpegCoefs(gold[k]) for k in names]
    mixes = [M.entry_mixup(1, 0.3), M.entry_cutmix(0, 5, 6, 31, 40)]
    plain_d, dsts, dstsf = Dsts(geoms, U8), Dsts(geoms, U8), Dsts(geoms, BF16_CHW)

    def entries(pairs):
        return [dict(coefs=c, resize_w=g[0], resize_h=g[1], crop_x=g[2], crop_y=g[3], crop_w=g[4], crop_h=g[5],
                     flip=g[6], dst=p, dst_stride=dp) for c, g, (p, dp) in zip(coefs, geoms, pairs)]

    try:
        arr, n = capi.make_jpeg_images(entries(plain_d.pairs()))
        capi.jpeg_resize_crop_to_device(arr, n, capi.MXD_U8, 0)
        plain = plain_d.read()[0]
        assert all(p.any() for p in plain)
        for d, mode in ((dsts, U8), (dstsf, BF16_CHW)):
            d.clear()
            arr, n = capi.make_jpeg_images(entries(d.pairs()))
            capi.jpeg_resize_crop_to_device_mix(arr, None, None, None, None, capi.make_mixes(mixes), n, d.dtype(), d.fmt(), 0)
            _compare(*d.read(), plain, mixes, mode, "jpeg")
    finally:
        for d in (plain_d, dsts, dstsf):
            d.free()
        for c in coefs:
            c.close()
