"""CPU: MXD_ENHANCE_PIL_GAUSSIAN_BLUR / PIL_BOX_BLUR -- the CPU statement and
the NumPy restatement (tests/pilblur_ref.py) against Pillow's own
ImageFilter.GaussianBlur / BoxBlur, byte for byte; mxd_pil_blur_params; the
refusals; the operator surface's arguments and marked plan."""
import numpy as np
import pytest
from PIL import Image, ImageFilter

import pilblur_ref as P
from mlx_data_amd import capi
from test_enhance import _buf, _calls, _entry, _plan

GAUSS, BOX = capi.MXD_ENHANCE_PIL_GAUSSIAN_BLUR, capi.MXD_ENHANCE_PIL_BOX_BLUR
# 0.3 and 1.0 are the radii at which a double division for ww gives other bytes
CASES = [(GAUSS, r) for r in (0, 0.1, 0.3, 1.0, 2.0, 5.0, 16.0)] + [(BOX, r) for r in (0.5, 3, 15)]
SIZES = [(1, 1), (2, 5), (17, 3), (63, 70), (130, 67)]  # w x h


@pytest.mark.parametrize("op,r", CASES)
@pytest.mark.parametrize("w,h", SIZES)
def test_cpu_statement_and_restatement_equal_pillow(w, h, op, r):
    img = np.random.default_rng(1000 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    flt = ImageFilter.GaussianBlur(r) if op == GAUSS else ImageFilter.BoxBlur(r)
    want = np.asarray(Image.fromarray(img).filter(flt))
    assert np.array_equal(P.blur(img, r, op == GAUSS), want)
    assert np.array_equal(capi.enhance_apply_u8(img, (op, r)), want)
    assert r != 0 or np.array_equal(want, img)


@pytest.mark.parametrize("op,r", CASES)
def test_params_match_the_formula(op, r):
    fr, ww, fw, passes = capi.pil_blur_params(op, r)
    want = P.params(r, op == GAUSS)
    assert (np.float32(fr), ww, fw, passes) == want, (fr, ww, fw, passes, want)
    assert int(fr) + 1 <= 16 and (2 * int(fr) + 1) * ww + 2 * fw in ((1 << 24) - 1, 1 << 24)


@pytest.mark.parametrize("e,what", [
    ((GAUSS, -1.0), "factor (the radius) must be finite and not negative"),
    ((BOX, float("nan")), "factor (the radius) must be finite and not negative"),
    ((GAUSS, 17.0), "factor (the radius) is too large: its box radius must stay below 16"),
    ((BOX, 16.0), "factor (the radius) is too large: its box radius must stay below 16"),
    ((GAUSS, 1.0, 3), "reserved must be 0"), ((11, 1.0), "unknown op 11")])
def test_refusals_name_the_image_and_the_limit(e, what):
    arr, n = capi.make_images([_entry(), _entry()])
    rcs, msg = _calls(arr, None, capi.make_enhances([(GAUSS, 16.0), e]), None, None, n, capi.MXD_U8, None)
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and msg == f"mxd_enhance: {what} (image 1)", (rcs, msg)
    with pytest.raises(RuntimeError):
        capi.enhance_apply_u8(np.zeros((4, 4, 3), np.uint8), e)
    if len(e) == 2:  # (the radius alone: what mxd_pil_blur_params sees)
        with pytest.raises(RuntimeError):
            capi.pil_blur_params(*e)


@pytest.mark.parametrize("make,word", [
    (lambda b: b.image_pil_gaussian_blur("image", -0.5), "image_pil_gaussian_blur: radius must be finite, not negative"),
    (lambda b: b.image_pil_gaussian_blur("image", 17.0), "image_pil_gaussian_blur: radius must be finite, not negative and small"),
    (lambda b: b.to_stream().image_pil_box_blur("image", float("nan")), "image_pil_box_blur: radius must be finite"),
    (lambda b: b.image_pil_box_blur("image", 16.0), "its box radius stays below 16"),
    (lambda b: b.image_random_pil_gaussian_blur("image", radius=(2.0, 0.1)), "image_random_pil_gaussian_blur: radius range has lo > hi"),
    (lambda b: b.image_random_pil_gaussian_blur("image", radius=(0.1, 40.0)), "image_random_pil_gaussian_blur: radius range must be finite"),
    (lambda b: b.image_random_pil_gaussian_blur("image", radius=1.0), "image_random_pil_gaussian_blur: radius must be a (lo, hi) pair"),
])
def test_surface_refuses_bad_arguments_when_the_op_is_made(make, word):
    with pytest.raises(ValueError) as err:
        make(_buf())
    assert word in str(err.value), str(err.value)


def test_the_ops_mark_the_plan_as_image_gaussian_blur_does():
    with pytest.raises(RuntimeError) as err:
        _buf(c=4).image_pil_box_blur("image", 1.0)[0]
    assert str(err.value) == "image_pil_box_blur: image must have 3 channels, not 4"
    b = _buf().image_resize("image", 30, 20)
    q, t = _plan(b), b.image_pil_gaussian_blur("image", 0.1)
    p = _plan(t)
    assert p["enhance"] == ("pil_gaussian_blur", float(np.float32(0.1)))
    assert {k: p[k] for k in p if k != "enhance"} == {k: q[k] for k in q if k != "enhance"}
    e = _plan(t.image_equalize("image").image_random_h_flip("image", 1.0)
              .image_normalize("image", mean=0.5, std=0.5, dtype="bfloat16", layout="chw"))
    assert e["enhance"] == p["enhance"] and e["tone"] == ("equalize", None) and e["flip"] and e["shape"] == [3, 20, 30]
    assert _plan(b.image_pil_box_blur("image", 3))["enhance"] == ("pil_box_blur", 3.0)
    assert _plan(b.image_random_pil_gaussian_blur("image", radius=(2, 2)))["enhance"] == ("pil_gaussian_blur", 2.0)
    assert _plan(b.image_pil_gaussian_blur_if(False, "image", 1.0))["enhance"] is None
    assert _plan(b.image_pil_box_blur_if(True, "image", 1.0))["enhance"] == ("pil_box_blur", 1.0)
    o = b.image_pil_gaussian_blur("image", 1.0, output_key="o")
    assert _plan(o, 0, "o")["enhance"] == ("pil_gaussian_blur", 1.0) and _plan(o, 0, "image")["enhance"] is None
