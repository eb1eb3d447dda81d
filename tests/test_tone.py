"""The per-image tone operations on the CPU (no device): the CPU statement of
the C ABI (mxd_tone_table_u8 / mxd_tone_apply_u8) bit-equal to Pillow and to
the NumPy restatement (tests/tone_ref.py) for every op, the contrast table for
every mean against Image.blend, the refusals of the C ABI with their messages,
the tone call's batch layout in the device-free environment
(tests/cpp/tone_layout_unit.cpp), and the operator surface's tone ops as far as
they go without a device (arguments, the marked plan, what composes)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tone_ref as R
from mlx_data_amd import capi

IMAGES = R.ref_images()
TONES = R.all_tones()


def _id(t):
    return f"{R.NAMES[t[0]]}-{t[1] if t[0] in (R.POSTERIZE, R.SOLARIZE) else t[2]}"


# ---- the CPU statement ------------------------------------------------------------

@pytest.mark.parametrize("tone", TONES, ids=[_id(t) for t in TONES])
def test_apply_u8_equals_pillow_and_the_restatement(tone):
    for name, img in IMAGES.items():
        got = capi.tone_apply_u8(img, tone)
        ref = R.apply(img, tone)
        pil = R.pillow_apply(img, tone)
        assert np.array_equal(ref, pil), (name, "restatement vs Pillow", np.argwhere(ref != pil)[:3])
        assert np.array_equal(got, pil), (name, "library vs Pillow", np.argwhere(got != pil)[:3])
        assert np.array_equal(capi.tone_table_u8(img, tone), R.table(img, tone)), name


def test_the_edge_images_take_the_branches_they_are_there_for():
    ident = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    eq, ac = (R.EQUALIZE, 0, 0.0), (R.AUTOCONTRAST, 0, 0.0)
    # a constant image: one bin, the identity for both
    assert np.array_equal(capi.tone_table_u8(IMAGES["constant-9x9"], eq), ident)
    assert np.array_equal(capi.tone_table_u8(IMAGES["constant-9x9"], ac), ident)
    # two levels: autocontrast stretches 20 / 220 to 0 / 255
    t = capi.tone_table_u8(IMAGES["two-level-16"], ac)
    assert t[0, 20] == 0 and t[0, 220] == 255 and t[1, 19] == 0 and t[2, 221] == 255
    # green is 255 except one pixel: step = (90000 - 89999) / 255 = 0, the identity for that channel only
    t = capi.tone_table_u8(IMAGES["green-255-but-one"], eq)
    assert np.array_equal(t[1], ident[1]) and not np.array_equal(t[0], ident[0])
    # zeros with five 255: (0 + 395) / 1 overshoots without the min
    t = capi.tone_table_u8(IMAGES["zeros-five-255"], eq)
    assert t[0, 0] == 0 and t[0, 1] == 255 and t[0, 255] == 255
    # NONE is the identity, whatever the pixels
    assert np.array_equal(capi.tone_table_u8(IMAGES["random-5x7"], (R.NONE, 0, 0.0)), ident)
    # in place
    img = IMAGES["mid-33x65"].copy()
    want = R.apply(img, eq)
    L = capi.lib()
    p = img.ctypes.data_as(ctypes.c_void_p)
    assert L.mxd_tone_apply_u8(p, ctypes.c_int64(img.size // 3), capi.make_tones([eq]), p) == capi.MXD_OK
    assert np.array_equal(img, want)


@pytest.mark.parametrize("factor", R.BLEND_FACTORS)
def test_contrast_table_for_every_mean_equals_image_blend(factor):
    """Row m of a (256, 256) image holds m (the grey of mean m), column v of
    the other holds v: one Image.blend gives t_m[v] for all 256 means."""
    from PIL import Image

    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    ramp = np.ascontiguousarray(grey.T)
    want = np.asarray(Image.blend(Image.fromarray(grey, "L"), Image.fromarray(ramp, "L"), factor))
    for m in range(256):
        # an image whose every luma byte is m: the grey (m, m, m)
        px = np.full((4, 3), m, np.uint8)
        assert R.mean_luma(px) == m
        got = capi.tone_table_u8(px, (R.CONTRAST, 0, factor))
        assert np.array_equal(got[0], want[m]), (m, np.flatnonzero(got[0] != want[m])[:3])
        assert np.array_equal(got[1], got[0]) and np.array_equal(got[2], got[0])
        assert np.array_equal(R.contrast_row(m, factor), want[m]), m


# ---- refusals of the calls ---------------------------------------------------------

def _entry(**kw):
    e = dict(src=4096, dst=4096, src_stride=64 * 3, src_w=64, src_h=64, channels=3, resize_w=32, resize_h=32, crop_x=0,
             crop_y=0, crop_w=32, crop_h=32, dst_stride=32 * 3 * 4)
    e.update(kw)
    return e


def _calls(arr, tones, colors, n, out_dtype, fmt):
    """The status of the two calls that take mxd_image, and the last message."""
    L = capi.lib()
    f = ctypes.byref(fmt) if fmt is not None else None
    rcs = (L.mxd_resize_crop_batch_tone(arr, tones, colors, n, out_dtype, f, 0, None),
           L.mxd_resize_crop_to_device_tone(arr, tones, colors, n, out_dtype, f, 0))
    return rcs, L.mxd_last_error().decode()


def _tone(op, arg=0, factor=0.0, reserved=0):
    t = capi.MxdTone()
    t.op, t.arg, t.factor, t.reserved = op, arg, factor, reserved
    return t


BAD_TONES = [
    (_tone(6), "unknown op 6"), (_tone(-1), "unknown op -1"), (_tone(R.POSTERIZE, 0), "posterize bits"),
    (_tone(R.POSTERIZE, 9), "posterize bits"), (_tone(R.SOLARIZE, -1), "solarize threshold"),
    (_tone(R.SOLARIZE, 257), "solarize threshold"), (_tone(R.CONTRAST, 0, -0.5), "factor"),
    (_tone(R.CONTRAST, 0, float("nan")), "factor"), (_tone(R.CONTRAST, 0, float("inf")), "factor"),
    (_tone(R.CONTRAST, 0, 2e6), "factor"), (_tone(R.EQUALIZE, 0, 0.0, 1), "reserved must be 0"),
]


def test_call_refusals_name_the_image_and_the_field():
    import color_ref

    bad = (capi.MXD_ERR_INVALID,) * 2
    arr, n = capi.make_images([_entry(), _entry()])
    good = capi.make_tones([(R.EQUALIZE, 0, 0.0), (R.CONTRAST, 0, 1e6)])  # (the bound itself is allowed)
    rcs, msg = _calls(arr, None, None, n, capi.MXD_U8, None)
    assert rcs == bad and msg == "mxd: null tones"
    for t, what in BAD_TONES:
        rcs, msg = _calls(arr, capi.make_tones([(R.NONE, 0, 0.0), t]), None, n, capi.MXD_U8, None)
        assert rcs == bad, (what, rcs)
        assert msg.startswith("mxd_tone: ") and what in msg and "(image 1)" in msg, msg
    # parameters an op does not read are not checked
    arr1, _ = capi.make_images([_entry(crop_x=8)])
    rcs, msg = _calls(arr1, capi.make_tones([(R.AUTOCONTRAST, 99, -3.0)]), None, 1, capi.MXD_U8, None)
    assert rcs == bad and "Array: sub: shape out of bound" in msg  # (the next refusal: geometry)
    arr4, _ = capi.make_images([_entry(), _entry(channels=4, src_stride=256)])
    rcs, msg = _calls(arr4, good, None, n, capi.MXD_U8, None)
    assert rcs == bad and msg == "mxd_tone: channels must be 3 (image 1)", msg
    # the colours' checks, when there are colours
    m = color_ref.SWAP.copy()
    m[2, 1] = float("nan")
    rcs, msg = _calls(arr, good, capi.make_colors([color_ref.IDENTITY, m]), n, capi.MXD_U8, None)
    assert rcs == bad and "m[2][1]" in msg and "(image 1)" in msg, msg
    rcs, msg = _calls(arr, good, None, n, 7, None)
    assert rcs == bad and msg == "mxd: bad out_dtype"
    # every check of the _fmt calls applies when fmt is given
    rcs, msg = _calls(arr, good, None, n, capi.MXD_U8, capi.make_out_format(elem=9))
    assert rcs == bad and "unknown elem" in msg
    odd, _ = capi.make_images([_entry(), _entry(dst=4097)])
    rcs, msg = _calls(odd, good, None, n, capi.MXD_U8, capi.make_out_format(capi.MXD_ELEM_F16))
    assert rcs == bad and "dst is not a multiple of the element size (image 1)" in msg
    short, _ = capi.make_images([_entry(), _entry(dst_stride=32 * 3 * 4 - 4)])
    rcs, msg = _calls(short, good, None, n, capi.MXD_F32_DIV255, None)
    assert rcs == bad and "dst_stride smaller than an output row (image 1)" in msg


def test_jpeg_call_and_cpu_statement_refusals():
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz"))
    coefs = capi.JpegCoefs(gold["caltech_300x200_jpg"])
    L = capi.lib()
    try:
        arr, n = capi.make_jpeg_images([dict(coefs=coefs, resize_w=150, resize_h=100, crop_x=0, crop_y=0, crop_w=150,
                                             crop_h=100, dst=4096, dst_stride=450)])
        assert L.mxd_jpeg_resize_crop_to_device_tone(arr, None, None, n, capi.MXD_U8, None, 0) == capi.MXD_ERR_INVALID
        assert L.mxd_last_error() == b"mxd: null tones"
        assert L.mxd_jpeg_resize_crop_to_device_tone(arr, capi.make_tones([(R.POSTERIZE, 0, 0.0)]), None, n, capi.MXD_U8,
                                                     None, 0) == capi.MXD_ERR_INVALID
        assert b"posterize bits" in L.mxd_last_error() and b"(image 0)" in L.mxd_last_error()
    finally:
        coefs.close()
    px = np.zeros((4, 3), np.uint8)
    p = px.ctypes.data_as(ctypes.c_void_p)
    table = np.zeros(768, np.uint8).ctypes.data_as(ctypes.c_void_p)
    ok = capi.make_tones([(R.EQUALIZE, 0, 0.0)])
    assert L.mxd_tone_apply_u8(p, ctypes.c_int64(4), None, p) == capi.MXD_ERR_INVALID
    assert L.mxd_last_error() == b"mxd: null tones"
    assert L.mxd_tone_table_u8(p, ctypes.c_int64(4), ok, None) == capi.MXD_ERR_INVALID
    assert L.mxd_tone_table_u8(None, ctypes.c_int64(4), ok, table) == capi.MXD_ERR_INVALID
    assert L.mxd_tone_apply_u8(p, ctypes.c_int64(4), ok, None) == capi.MXD_ERR_INVALID
    for t, what in BAD_TONES:
        assert L.mxd_tone_table_u8(p, ctypes.c_int64(4), capi.make_tones([t]), table) == capi.MXD_ERR_INVALID
        assert what.encode() in L.mxd_last_error()
    assert L.mxd_tone_table_u8(p, ctypes.c_int64(0), ok, table) == capi.MXD_OK  # no pixels: the identity


def test_every_declared_symbol_is_exported():
    L = capi.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mxd_amd.h")).read()
    assert "#define MXD_HAS_TONE 1" in header and "#define MXD_ABI_VERSION 7" in header
    for name in ("mxd_tone_table_u8", "mxd_tone_apply_u8", "mxd_resize_crop_batch_tone", "mxd_resize_crop_to_device_tone",
                 "mxd_jpeg_resize_crop_to_device_tone"):
        assert name + "(" in header and name in capi.EXPORTS
        assert getattr(L, name) is not None
    assert ctypes.sizeof(capi.MxdTone) == 16
    for k, name in enumerate(("NONE", "POSTERIZE", "SOLARIZE", "AUTOCONTRAST", "EQUALIZE", "CONTRAST")):
        assert f"MXD_TONE_{name} = {k}" in header and getattr(capi, "MXD_TONE_" + name) == k


# ---- the layout of a tone call ------------------------------------------------------

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mlx-data_amd")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_tone_layout_unit(tmp_path):
    """tests/cpp/tone_layout_unit.cpp: a tone batch of mixed routes and ops in
    the device-free environment -- entries, block counts (no tone_hist
    workgroups for the ops without statistics), the workspace, cache keys."""
    exe = str(tmp_path / "tone_layout_unit")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-I", os.path.join(os.path.dirname(HERE), "include"), "-I",
                    os.path.join(PKG, "csrc"), os.path.join(HERE, "cpp", "tone_layout_unit.cpp"), "-L", PKG,
                    "-lmxd_amd", "-Wl,-rpath," + PKG, "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


# ---- operator surface: arguments, the marked plan, what composes -----------------------

def _rgb(h=40, w=60, seed=0, c=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def _buf(n=1, **kw):
    from mlx_data_amd import data as dx

    return dx.buffer_from_vector([dict(image=_rgb(seed=k, **kw)) for k in range(n)])


def _plan(b, i=0, key="image"):
    from mlx_data_amd import _pipeline

    return _pipeline._plan(b, i, key)


@pytest.mark.parametrize("make,word", [
    (lambda b: b.image_posterize("image", 0), "image_posterize: bits must be in 1..8"),
    (lambda b: b.image_posterize("image", 9), "image_posterize: bits must be in 1..8"),
    (lambda b: b.image_solarize("image", -1), "image_solarize: threshold must be in 0..256"),
    (lambda b: b.image_solarize("image", 257), "image_solarize: threshold must be in 0..256"),
    (lambda b: b.image_contrast("image", -0.1), "image_contrast: factor must be finite"),
    (lambda b: b.image_contrast("image", float("nan")), "image_contrast: factor must be finite"),
    (lambda b: b.image_contrast("image", float("inf")), "image_contrast: factor must be finite"),
    (lambda b: b.image_contrast("image", 1e7), "image_contrast: factor must be finite"),
    (lambda b: b.to_stream().image_posterize("image", 12), "image_posterize: bits must be in 1..8"),
])
def test_surface_refuses_bad_arguments_when_the_op_is_made(make, word):
    with pytest.raises(ValueError) as err:
        make(_buf())
    assert word in str(err.value), str(err.value)


OPS = [("posterize", lambda b, **kw: b.image_posterize("image", 3, **kw), ("posterize", 3)),
       ("solarize", lambda b, **kw: b.image_solarize("image", **kw), ("solarize", 128)),
       ("autocontrast", lambda b, **kw: b.image_autocontrast("image", **kw), ("autocontrast", None)),
       ("equalize", lambda b, **kw: b.image_equalize("image", **kw), ("equalize", None)),
       ("contrast", lambda b, **kw: b.image_contrast("image", 1.5, **kw), ("contrast", 1.5))]


def test_surface_refuses_non_rgb_images_when_the_op_is_applied():
    for c in (1, 2, 4):
        for name, make, _ in OPS:
            b = make(_buf(c=c))  # made without complaint
            with pytest.raises(RuntimeError) as err:
                b[0]
            assert str(err.value) == f"image_{name}: image must have 3 channels, not {c}", str(err.value)


def test_the_op_marks_the_plan_and_what_composes_composes():
    b = _buf().image_resize("image", 30, 20)
    q = _plan(b)
    assert q["tone"] is None
    for name, make, want in OPS:
        t = make(b)
        p = _plan(t)
        assert p["tone"] == want, (name, p["tone"])
        assert {k: p[k] for k in p if k != "tone"} == {k: q[k] for k in q if k != "tone"}  # nothing else touched
        # flips compose after every tone op
        f = _plan(t.image_random_h_flip("image", 1.0))
        assert f["tone"] == want and f["flip"] and f["resize"] == (30, 20) and f["window"] == (0, 0, 60, 40)
        # a colour op, image_to_float and image_normalize compose on the toned plan
        c = _plan(t.image_color_twist("image", 1.2, 0.5))
        assert c["tone"] == want and np.array_equal(np.float32(c["color"]), capi.color_twist_matrix(1.2, 0.5))
        assert c["resize"] == (30, 20) and c["window"] == (0, 0, 60, 40)
        fl = _plan(t.image_to_float("image"))
        assert fl["tone"] == want and fl["shape"] == [20, 30, 3] and fl["window"] == (0, 0, 60, 40)
        n = _plan(t.image_normalize("image", mean=0.5, std=0.5, dtype="bfloat16", layout="chw"))
        assert n["tone"] == want and n["format"]["dtype"] == "bfloat16" and n["shape"] == [3, 20, 30]
        # a crop before the op is part of the plan the op marks
        pre = _plan(make(b.image_center_crop("image", 10, 10)))
        assert pre["tone"] == want and pre["crop"] == (10, 5, 10, 10) and pre["resize"] == (30, 20)
        # output_key and _if
        o = make(b, output_key="toned")
        assert _plan(o, 0, "toned")["tone"] == want and _plan(o, 0, "image")["tone"] is None
    # crops compose after the pointwise ops (center, random, random area)
    for t, want in ((b.image_posterize("image", 2), ("posterize", 2)), (b.image_solarize("image", 77), ("solarize", 77))):
        a = _plan(t.image_center_crop("image", 10, 10).image_random_h_flip("image", 1.0).image_random_crop("image", 4, 4))
        assert a["tone"] == want and a["resize"] == (30, 20) and a["flip"] and a["crop"][2:] == (4, 4)
        assert a["window"] == (0, 0, 60, 40)
        r = _plan(t.image_random_area_crop("image", (0.3, 0.6), (0.8, 1.2)))
        assert r["tone"] == want and r["window"] == (0, 0, 60, 40) and r["resize"] == (30, 20)
    assert _plan(b.image_posterize_if(False, "image", 2))["tone"] is None
    assert _plan(b.image_solarize_if(True, "image", 3))["tone"] == ("solarize", 3)
    assert _plan(b.image_autocontrast_if(True, "image"))["tone"] == ("autocontrast", None)
    assert _plan(b.image_equalize_if(False, "image"))["tone"] is None
    assert _plan(b.image_contrast_if(True, "image", 0.25))["tone"] == ("contrast", 0.25)
    assert _plan(b.image_solarize("image"))["tone"] == ("solarize", 128)  # the default
    # on a stream too
    s = _buf().to_stream().image_equalize("image").image_contrast_if(False, "image", 2.0)
    assert s is not None
