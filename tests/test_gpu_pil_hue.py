"""GPU: MXD_ENHANCE_PIL_HUE in the enhance calls of the C ABI (hue_rows) and image_pil_hue of the
surface.  A C ABI case is byte-equal to the CPU statement (pinned on Pillow by tests/test_pil_hue.py)
applied to the u8 result of the same chain in front of the op, then the statements of what runs
behind it; a surface case is byte-equal to Pillow itself.  Bytes outside the images keep their 0xff."""
import numpy as np
import pytest

import mix_ref as M
import tone_ref as T
import warp_ref as W
from gpu_util import synth
from mlx_data_amd import capi
from mlx_data_amd import data as dx
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expect, expected_table
from test_gpu_blur import _run, _same
from test_gpu_color import FORMATTED, U8, Sources
from test_gpu_tone_surface import chain, one_device, plan, samples  # noqa: F401  (one_device: autouse)
from test_pil_hue import HUE, colours, pillow_hue  # noqa: F401  (colours: the cube fixture)

pytestmark = pytest.mark.gpu

BF16_CHW = FORMATTED[5]
# w x h: a lane's tail, a full lane, a lane and a tail, 64 +- 1; one row, two, one more than a workgroup's 8
SIZES = [(w, h) for h in (1, 2, 9) for w in (1, 3, 4, 5, 63, 64, 65)]
_hue = capi.enhance_apply_u8


@pytest.fixture(scope="module")
def windows():
    imgs = [synth(24, 80, 3, 1200 + k) for k in range(len(SIZES))]
    geoms = [(70, 12, 2 + k % 3, 1, w, h, k % 2) for k, (w, h) in enumerate(SIZES)]
    src = Sources(imgs, geoms)
    yield src, src.plain_u8()
    src.free()


@pytest.mark.parametrize("dst", [{}, dict(dst_pad=2, dst_shift=1)], ids=["aligned", "misaligned"])
def test_every_size_in_u8(windows, dst):
    src, plain = windows
    enhs = [(HUE, 0.0, 25)] * len(plain)
    _same(_run(src, enhs, U8, **dst), [_hue(q, e) for q, e in zip(plain, enhs)], "u8")


def test_four_shifts_and_none_in_one_call(windows):
    src, plain = windows
    enhs = [[(HUE, 0.0, 1), (HUE, 0.0, 127), (capi.MXD_ENHANCE_NONE, 0.0), (HUE, 0.0, 128), (HUE, 0.0, 231)][k % 5] for k in range(len(plain))]
    outs = _run(src, enhs, U8)
    _same(outs, [_hue(q, e) for q, e in zip(plain, enhs)], "mixed")
    _same(outs[2::5], plain[2::5], "none")


def test_every_colour_at_identity_geometry(colours):
    """The device's float32 divisions and double roundings on all 2^24 inputs."""
    src = Sources([colours], [(4096, 4096, 0, 0, 4096, 4096, 0)])
    try:
        plain = src.plain_u8()
        assert np.array_equal(plain[0], colours)
        got = _run(src, [(HUE, 0.0, 25)], U8)[0]
    finally:
        src.free()
    assert int((got != _hue(colours, (HUE, 0.0, 25))).sum()) == 0


@pytest.mark.parametrize("case", ["warp", "tone", "bf16_chw", "mix"])
def test_behind_a_warp_and_in_front_of_tone_format_and_mix(windows, case):
    src, plain = windows
    n = len(plain)
    enhs = [(HUE, 0.0, 25 + k) for k in range(n)]
    table = expected_table("bfloat16", 3, IMAGENET_MEAN, IMAGENET_STD)
    if case == "warp":
        warps = [(W.BILINEAR, (255, 0, 30), W.rotate_matrix(g[4], g[5], 30.0)) for g in src.geoms]
        want = [_hue(capi.warp_apply_u8(q, w), e) for q, w, e in zip(plain, warps, enhs)]
        _same(_run(src, enhs, U8, warps), want, case)
    elif case == "tone":
        tones = [(T.EQUALIZE, 0, 0.0)] * n
        _same(_run(src, enhs, U8, None, tones), [T.apply(_hue(q, e), t) for q, e, t in zip(plain, enhs, tones)], case)
    elif case == "bf16_chw":
        _same(_run(src, enhs, BF16_CHW), [expect(table, _hue(q, e)) for q, e in zip(plain, enhs)], case)
    else:
        shifted = [_hue(q, e) for q, e in zip(plain, enhs)]
        mixes = [M.entry_mixup(k, 0.3) for k in range(n)]  # (each its own partner: sizes differ)
        _same(_run(src, enhs, BF16_CHW, mixes=mixes), [expect(table, M.apply(shifted, k, mixes[k])) for k in range(n)], case)


@pytest.mark.parametrize("after", ["plain", "flipped", "cropped"])
def test_the_surface_op_on_a_device_batch_equals_pillow(after):
    b = chain(dx.buffer_from_vector(samples(6, 3)))
    u8 = b.batch(6)[0]["image"]
    want = np.stack([pillow_hue(x, int(np.array(-0.1 * 255).astype("uint8"))) for x in u8])
    t = b.image_pil_hue("image", -0.1)
    if after == "flipped":
        t, want = t.image_random_h_flip("image", 1.0), want[:, :, ::-1]
    if after == "cropped":
        t, want = t.image_center_crop("image", 21, 17), want[:, 6:23, 6:27]
    assert plan(t)["enhance"] == ("pil_hue", 0.0, 231) and plan(t)["src_shape"] == plan(b)["src_shape"]
    got = t.batch(6, device=0)[0]["image"].numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want)
