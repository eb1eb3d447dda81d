"""CPU: MXD_ENHANCE_PIL_HUE -- the CPU statement against Pillow's own HSV round trip on every RGB
colour; the refusals; the header; the surface's arguments, marked plan and composition rules."""
import ctypes
import os

import numpy as np
import pytest
from PIL import Image

from mlx_data_amd import capi
from test_enhance import _buf, _calls, _entry, _materialised, _plan

HUE = capi.MXD_ENHANCE_PIL_HUE
SHIFTS = [0, 1, 25, 127, 128, 231, 255]


def pillow_hue(img, shift):
    """torchvision's adjust_hue on a PIL image, the shift already a byte."""
    h, s, v = Image.fromarray(np.ascontiguousarray(img)).convert("HSV").split()
    h = Image.fromarray(np.asarray(h) + np.uint8(shift))  # uint8: wraps
    return np.asarray(Image.merge("HSV", (h, s, v)).convert("RGB"))


@pytest.fixture(scope="module")
def colours():
    """Every RGB colour once, as one 4096 x 4096 image."""
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([c & 255, (c >> 8) & 255, c >> 16], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.mark.parametrize("shift", SHIFTS)
def test_every_colour_equals_pillow(colours, shift):
    got, want = capi.enhance_apply_u8(colours, (HUE, 0.0, shift)), pillow_hue(colours, shift)
    assert int((got != want).sum()) == 0
    grey = (colours[..., 0] == colours[..., 1]) & (colours[..., 1] == colours[..., 2])
    assert np.array_equal(got[grey], colours[grey]) and not np.array_equal(got, colours)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (3, 5)])
def test_small_sizes_with_strided_input_and_output(w, h):
    img = np.random.default_rng(10 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = pillow_hue(img, 25)
    assert np.array_equal(capi.enhance_apply_u8(img, (HUE, 0.0, 25)), want)
    wide = np.full((h, w + 3, 3), 0xEE, np.uint8)
    wide[:, 1:w + 1] = img
    out = np.full((h, w + 5, 3), 0xDD, np.uint8)
    capi.enhance_apply_u8(wide[:, 1:w + 1], (HUE, 0.0, 25), out[:, 2:w + 2])
    assert np.array_equal(out[:, 2:w + 2], want) and (out[:, :2] == 0xDD).all() and (out[:, w + 2:] == 0xDD).all()


@pytest.mark.parametrize("e,what", [
    ((HUE, 0.0, -1), "hue shift must be in 0..255"), ((HUE, 0.0, 256), "hue shift must be in 0..255"),
    ((HUE, 0.5, 25), "factor must be 0"), (capi.MxdEnhance(HUE, 0.0, (ctypes.c_int32 * 2)(25, 1)), "reserved must be 0"), ((13, 0.0), "unknown op 13")])
def test_refusals_name_the_image_and_the_field(e, what):
    arr, n = capi.make_images([_entry(), _entry()])
    rcs, msg = _calls(arr, None, capi.make_enhances([(HUE, 0.0, 255), e]), None, None, n, capi.MXD_U8, None)
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and msg == f"mxd_enhance: {what} (image 1)", (rcs, msg)
    with pytest.raises(RuntimeError):
        capi.enhance_apply_u8(np.zeros((4, 4, 3), np.uint8), e)


def test_the_header_defines_the_op_and_keeps_the_abi():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mxd_amd.h")).read()
    assert "#define MXD_HAS_PIL_HUE 1" in text and "MXD_ENHANCE_PIL_HUE = 12" in text and HUE == 12
    assert "#define MXD_ABI_VERSION 7" in text and ctypes.sizeof(capi.MxdEnhance) == 16


@pytest.mark.parametrize("make,word", [
    (lambda b: b.image_pil_hue("image", 0.7), "hue_factor (0.7) is not in [-0.5, 0.5]."),
    (lambda b: b.to_stream().image_pil_hue("image", -0.51), "hue_factor (-0.51) is not in [-0.5, 0.5]."),
    (lambda b: b.image_pil_hue("image", float("nan")), "hue_factor (nan) is not in [-0.5, 0.5]."),
    (lambda b: b.image_random_pil_hue("image", hue=(-0.1, 1.0)), "hue_factor (1.0) is not in [-0.5, 0.5]."),
    (lambda b: b.image_random_pil_hue("image", hue=(0.1, -0.1)), "image_random_pil_hue: hue range has lo > hi"),
    (lambda b: b.image_random_pil_hue("image", hue=0.1), "image_random_pil_hue: hue must be a (lo, hi) pair"),
])
def test_surface_refuses_bad_arguments_when_the_op_is_made(make, word):
    with pytest.raises(ValueError) as err:
        make(_buf())
    assert str(err.value) == word


@pytest.mark.parametrize("h", [-0.5, -0.1, -0.004, 0.0, 0.003, 0.1, 0.3, 0.5])
def test_the_marked_shift_is_numpys_uint8_cast_of_the_drawn_factor(h):
    want = ("pil_hue", 0.0, int(np.array(h * 255).astype("uint8")))  # torchvision's own expression
    assert _plan(_buf().image_pil_hue("image", h))["enhance"] == want
    assert _plan(_buf().image_random_pil_hue("image", hue=(h, h)))["enhance"] == want  # (a range of one point: the draw is h)


def test_the_op_marks_the_plan_and_composes_as_image_color_does():
    b = _buf().image_resize("image", 30, 20)
    q, t = _plan(b), b.image_pil_hue("image", 0.1)
    p = _plan(t)
    assert {k: p[k] for k in p if k != "enhance"} == {k: q[k] for k in q if k != "enhance"}
    # a flip, a crop, a tone op and an output form compose
    e = _plan(t.image_random_h_flip("image", 1.0).image_center_crop("image", 10, 8).image_equalize("image")
              .image_normalize("image", mean=0.5, std=0.5, dtype="bfloat16", layout="chw"))
    assert e["enhance"] == p["enhance"] and e["tone"] == ("equalize", None) and e["flip"] and e["shape"] == [3, 8, 10]
    assert e["src_shape"] == q["src_shape"]
    assert _plan(t.image_to_float("image"))["enhance"] == p["enhance"]
    assert _plan(t.image_color_twist("image", 1.2, 0.8, 1.5, 20.0))["enhance"] == p["enhance"]
    # a second enhance op, a resize and a warp run the hue shift first (without a device the attempt is the evidence)
    for after in (lambda: t.image_brightness("image", 1.2), lambda: t.image_resize("image", 15, 10),
                  lambda: t.image_affine_rotate("image", 30.0)):
        a = _materialised(after)
        assert a is None or a["enhance"] != p["enhance"]
    assert _plan(b.image_pil_hue_if(False, "image", 0.1))["enhance"] is None
    assert _plan(b.image_random_pil_hue_if(True, "image", hue=(0.1, 0.1)))["enhance"] == p["enhance"]
