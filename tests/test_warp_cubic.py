"""MXD_WARP_BICUBIC without a device: the CPU statement (mxd_warp_apply_u8) against Pillow's
Image.transform(AFFINE, BICUBIC), the mode's refusals, the header, and resample="cubic" on the surface."""
import importlib
import os
import sys

import numpy as np
import pytest
from PIL import Image

import warp_ref as W
from mlx_data_amd import _pipeline, capi

CUBIC, FILL = 8, (10, 200, 90)
SIZES = [(1, 1), (2, 3), (3, 2), (7, 5), (64, 17)]  # (w, h)
FAMILIES = ["shear-x", "shear-xy", "translate-fraction", "translate-integer", "rotate-30", "rotate-random", "random",
            "scale", "outside"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mlx-data_amd", "compat"))  # import mlx.data, as tests/test_reference_buffer.py does
CORNER = "matrix maps a corner to a source coordinate of magnitude >= 32768"
W.RESAMPLE[CUBIC] = Image.BICUBIC  # this file's own: warp_ref maps NEAREST and BILINEAR


def image(kind, w, h, seed):  # uniform noise, or only 0 and 255: the latter overshoots into both clips
    px = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return px if kind == "noise" else np.where(px < 128, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("kind", ["noise", "binary"])
@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_apply_u8_equals_image_transform_bicubic(size, name, kind):
    w, h = size
    img = image(kind, w, h, 31 * w + h)
    m = W.OUTSIDE if name == "outside" else W.families(w, h, np.random.default_rng(1000 * h + w))[name]
    want = W.pillow_apply(img, (CUBIC, FILL, m))
    got = capi.warp_apply_u8(img, (CUBIC, FILL, m))
    assert np.array_equal(got, want), (m, int((got != want).sum()), np.argwhere(got != want)[:3])
    if kind == "binary" and size == (64, 17) and name != "outside":
        assert (want == 0).any() and (want == 255).any()  # both clips are exercised
    room = np.zeros((h + 2, w, 3), np.uint8)  # rgb and out overlap: out two rows below rgb
    room[:h] = img
    capi.warp_apply_u8(room[:h], (CUBIC, FILL, m), room[2:])
    assert np.array_equal(room[2:], want)


@pytest.mark.parametrize("m,what", [((1, 0, float("nan"), 0, 1, 0), "m[2] is not finite"), ((1024.0, 0, 0, 0, 1, 0), CORNER),
                                    (W.translate(0.0, -32768.0), CORNER)], ids=["nan", "scale", "translate"])
def test_refusals_of_the_mode(m, what):
    L = capi.lib()
    assert L.mxd_warp_validate(capi.make_warps([(CUBIC, 0, m)]), 32, 32) == capi.MXD_ERR_INVALID
    assert L.mxd_last_error().decode() == f"mxd_warp: {what} (image 0)"
    e = dict(src=4096, dst=4096, src_stride=64 * 3, src_w=64, src_h=64, channels=3, resize_w=32, resize_h=32, crop_x=0,
             crop_y=0, crop_w=32, crop_h=32, dst_stride=32 * 3 * 4)
    arr, n = capi.make_images([e, e])
    warps = capi.make_warps([(CUBIC, 0, W.IDENTITY), (CUBIC, 0, m)])
    enh, mix = capi.make_enhances([(capi.MXD_ENHANCE_NONE, 0.0)] * 2), capi.make_mixes([(capi.MXD_MIX_NONE,)] * 2)
    tail = (n, capi.MXD_U8, None, 0, None)
    for rc in (L.mxd_resize_crop_batch_warp(arr, warps, None, None, *tail),  # and the later calls that take warps
               L.mxd_resize_crop_batch_enhance(arr, warps, enh, None, None, *tail),
               L.mxd_resize_crop_batch_mix(arr, warps, enh, None, None, mix, *tail)):
        assert rc == capi.MXD_ERR_INVALID and L.mxd_last_error().decode() == f"mxd_warp: {what} (image 1)"


def test_header_and_constants():
    header = open(os.path.join(ROOT, "include", "mxd_amd.h")).read()
    assert "#define MXD_HAS_WARP_CUBIC 1" in header and "#define MXD_ABI_VERSION 7" in header
    assert "MXD_WARP_BILINEAR = 2, MXD_WARP_BICUBIC = 8 }" in header
    assert "p3 = 2 (v1 - v2) + v3 - v4" in header  # the statement stands beside BILINEAR's
    assert capi.MXD_WARP_BICUBIC == CUBIC


OPS = [("image_affine", ((1, 0.25, -2, 0.5, 1, 3),), {}, (1.0, 0.25, -2.0, 0.5, 1.0, 3.0)),
       ("image_shear", (0.3, -0.1), {}, W.shear(0.3, -0.1)), ("image_translate", (2.5, -4), {}, W.translate(2.5, -4.0)),
       ("image_affine_rotate", (30.0,), {}, W.rotate_matrix(30, 20, 30.0)),
       ("image_random_shear", (), dict(x=(0.2, 0.2)), W.shear(0.2, 0.0)),
       ("image_random_translate", (), dict(y=(3, 3)), W.translate(0.0, 3.0)),
       ("image_random_affine_rotate", ((-45, -45),), {}, W.rotate_matrix(30, 20, -45.0))]


@pytest.mark.parametrize("package", ["mlx_data_amd.data", "mlx.data"])
@pytest.mark.parametrize("op,args,kw,m", OPS, ids=[o[0] for o in OPS])
def test_cubic_marks_the_plan_on_every_op_and_composes(op, args, kw, m, package):
    dx = importlib.import_module(package)
    px = np.random.default_rng(0).integers(0, 256, (40, 60, 3), dtype=np.uint8)
    b = dx.buffer_from_vector([dict(image=px)]).image_resize("image", 30, 20)
    q = _pipeline._plan(b, 0, "image")
    for t in (getattr(b, op)("image", *args, resample="cubic", fill=(1, 2, 3), **kw),
              getattr(b, op + "_if")(True, "image", *args, resample="cubic", fill=(1, 2, 3), **kw)):
        p = _pipeline._plan(t, 0, "image")
        assert p["warp"] == ("cubic", (1, 2, 3), m)
        assert {k: p[k] for k in p if k != "warp"} == {k: q[k] for k in q if k != "warp"}
        e = _pipeline._plan(t.image_equalize("image").image_normalize("image", mean=0.5, std=0.5, layout="chw"), 0, "image")
        assert e["warp"] == p["warp"] and e["tone"] == ("equalize", None) and e["shape"] == [3, 20, 30]
    assert getattr(b.to_stream(), op)("image", *args, resample="cubic", **kw) is not None  # a Stream takes it too
    with pytest.raises(ValueError, match="unknown resample 'bicubic'"):
        getattr(b, op)("image", *args, resample="bicubic", **kw)
    with pytest.raises(RuntimeError, match="image_translate: mxd_warp: " + CORNER):
        b.image_translate("image", 40000.0, resample="cubic")[0]
