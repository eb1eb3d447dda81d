"""GPU: MXD_ENHANCE_PIL_GAUSSIAN_BLUR / PIL_BOX_BLUR in the enhance calls of the
C ABI (pilblur_rows).  Every case is byte-equal to the NumPy restatement of
Pillow's filter (tests/pilblur_ref.py, itself pinned on Pillow by
tests/test_pilblur.py) applied to the u8 result of the same chain in front of
the op, followed by the statements of what the chain runs behind it; bytes
outside the images must keep the 0xff they were filled with."""
import numpy as np
import pytest

import blur_ref as B
import color_ref as C
import enhance_ref as E
import mix_ref as M
import pilblur_ref as P
import tone_ref as T
import warp_ref as W
from gpu_util import synth
from mlx_data_amd import capi
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expect, expected_table
from test_gpu_blur import _run, _same
from test_gpu_color import FORMATTED, U8, Sources
from test_pilblur import BOX, CASES, GAUSS

pytestmark = pytest.mark.gpu

BF16_CHW = FORMATTED[5]
# w x h: radius larger than the image, one strip, 64 +- 1, several strips sharing halos; the last
# one is three rows higher than a segment (112 rows): a second segment
SIZES = [(1, 1), (2, 5), (17, 3), (63, 70), (65, 33), (130, 67), (20, 115)]


def _op(q, enh):
    if enh[0] in (GAUSS, BOX):
        return P.blur(q, enh[1], enh[0] == GAUSS)
    if enh[0] == capi.MXD_ENHANCE_GAUSSIAN_BLUR:
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


@pytest.fixture(scope="module")
def windows():
    imgs = [synth(90, 150, 3, 900 + k) for k in range(len(SIZES))]
    geoms = [(140, 125, 3 + k, 5, w, h, k % 2) for k, (w, h) in enumerate(SIZES)]
    src = Sources(imgs, geoms)
    yield src, src.plain_u8()
    src.free()


@pytest.mark.parametrize("op,r", CASES)
def test_every_size_in_u8_with_aligned_and_misaligned_destinations(windows, op, r):
    src, plain = windows
    enhs = [(op, r)] * len(plain)
    want = [_expected(U8, q, e) for q, e in zip(plain, enhs)]
    _same(_run(src, enhs, U8), want, "u8")
    _same(_run(src, enhs, U8, dst_pad=2, dst_shift=1), want, "misaligned")


def test_every_enhance_op_in_one_call(windows):
    src, plain = windows
    enhs = [(GAUSS, 2.0), (E.SHARPNESS, 1.9), (BOX, 3), (E.NONE, 0.0), (capi.MXD_ENHANCE_GAUSSIAN_BLUR, 2.0, 23),
            (GAUSS, 0.0), (GAUSS, 0.7)]
    _same(_run(src, enhs, U8), [_expected(U8, q, e) for q, e in zip(plain, enhs)], "mixed")
    # reversed: another image last in each table, and the output form behind the stage
    enhs = enhs[::-1]
    _same(_run(src, enhs, BF16_CHW), [_expected(BF16_CHW, q, e) for q, e in zip(plain, enhs)], "mixed bf16")


def test_behind_a_warp_and_in_front_of_tone_colour_and_bf16_chw(windows):
    src, plain = windows
    n = len(plain)
    warps = [(W.BILINEAR, (255, 0, 30), W.rotate_matrix(g[4], g[5], 30.0)) for g in src.geoms]
    enhs = [(GAUSS, 2.0)] * n
    tones = [(T.EQUALIZE, 0, 0.0)] * n
    mats = (C.eight_matrices() * 2)[1:1 + n]
    want = [_expected(BF16_CHW, q, e, w, t, m) for q, e, w, t, m in zip(plain, enhs, warps, tones, mats)]
    _same(_run(src, enhs, BF16_CHW, warps, tones, mats), want, "chain")


def test_with_a_mix_stage_last(windows):
    src, plain = windows
    enhs = [(GAUSS, 2.0)] * len(plain)
    blurred = [_expected(U8, q, e) for q, e in zip(plain, enhs)]
    mixes = [M.entry_mixup(k, 0.3) for k in range(len(plain))]  # (each its own partner: sizes differ)
    want = [expect(expected_table("bfloat16", 3, IMAGENET_MEAN, IMAGENET_STD), M.apply(blurred, k, mixes[k]))
            for k in range(len(plain))]
    _same(_run(src, enhs, BF16_CHW, mixes=mixes), want, "mix")
