"""The per-image affine warps on the CPU (no device): the CPU statement of the
C ABI (mxd_warp_apply_u8) byte-equal to Pillow's Image.transform(AFFINE) and
Image.rotate, the refusals of the C ABI with their messages, the warp call's
batch layout in the device-free environment (tests/cpp/warp_layout_unit.cpp),
and the operator surface's warp ops as far as they go without a device
(arguments, the marked plan, what composes, the random ops' draws)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import warp_ref as W
from mlx_data_amd import capi

SIZES = [(1, 1), (5, 1), (1, 5), (13, 17), (40, 39), (8, 7)]  # (h, w)
MODES = [W.NEAREST, W.BILINEAR]
MODE_IDS = ["nearest", "bilinear"]


def _img(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- the CPU statement against Pillow -----------------------------------------------------

@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for h, w in SIZES])
def test_apply_u8_equals_image_transform(size, mode):
    """Six matrix families, seeded, with non-zero fills; then the same through
    strided inputs and outputs."""
    h, w = size
    rng = np.random.default_rng(1000 * h + w)
    for rep in range(3):
        img = _img(h, w, 17 * rep + h)
        for name, m in W.families(w, h, rng).items():
            fill = tuple(int(v) for v in rng.integers(1, 256, 3))
            warp = (mode, fill, m)
            want = W.pillow_apply(img, warp)
            got = capi.warp_apply_u8(img, warp)
            assert np.array_equal(got, want), (name, m, int((got != want).sum()))
            if rep == 0:
                wide = np.full((h, w + 3, 3), 0xEE, np.uint8)
                wide[:, 1:w + 1] = img
                out = np.full((h, w + 5, 3), 0xDD, np.uint8)
                capi.warp_apply_u8(wide[:, 1:w + 1], warp, out[:, 2:w + 2])
                assert np.array_equal(out[:, 2:w + 2], want), name
                assert (out[:, :2] == 0xDD).all() and (out[:, w + 2:] == 0xDD).all()


ANGLES = [0.0, 90.0, -90.0, 180.0, 270.0, 45.0, 1e-9, 360.0]


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("size", [(13, 17), (16, 16), (9, 9), (12, 31), (31, 12)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_the_rotate_matrix_equals_image_rotate(size, mode):
    """The matrix image_affine_rotate marks (read back from the plan) through
    the CPU statement, against Image.rotate."""
    from mlx_data_amd import data as dx

    h, w = size
    rng = np.random.default_rng(h * 100 + w)
    img = _img(h, w, 5)
    for angle in ANGLES + [float(a) for a in rng.uniform(-720, 720, 12)]:
        fill = tuple(int(v) for v in rng.integers(0, 256, 3))
        b = dx.buffer_from_vector([dict(image=img)]).image_affine_rotate(
            "image", angle, resample=MODE_IDS[mode - 1], fill=fill)
        name, f, m = _plan(b)["warp"]
        assert name == MODE_IDS[mode - 1] and f == fill
        assert m == W.rotate_matrix(w, h, angle), angle
        got = capi.warp_apply_u8(img, (mode, fill, m))
        want = W.pillow_rotate(img, angle, mode, fill)
        assert np.array_equal(got, want), (angle, int((got != want).sum()))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_none_and_the_identity_return_the_input(mode):
    for h, w in SIZES:
        img = _img(h, w, 3)
        assert np.array_equal(capi.warp_apply_u8(img, (W.NONE, 200, None)), img)
        assert np.array_equal(capi.warp_apply_u8(img, (mode, 200, W.IDENTITY)), img)
    img = _img(9, 11, 4)
    same = img.copy()
    capi.warp_apply_u8(same, (mode, 9, W.shear(0.5, 0.0)), same)  # in place
    assert np.array_equal(same, W.pillow_apply(img, (mode, 9, W.shear(0.5, 0.0))))


# ---- refusals ----------------------------------------------------------------------------

def _entry(**kw):
    e = dict(src=4096, dst=4096, src_stride=64 * 3, src_w=64, src_h=64, channels=3, resize_w=32, resize_h=32, crop_x=0,
             crop_y=0, crop_w=32, crop_h=32, dst_stride=32 * 3 * 4)
    e.update(kw)
    return e


def _calls(arr, warps, tones, colors, n, out_dtype, fmt):
    """The status of the two calls that take mxd_image, and the last message."""
    L = capi.lib()
    f = ctypes.byref(fmt) if fmt is not None else None
    rcs = (L.mxd_resize_crop_batch_warp(arr, warps, tones, colors, n, out_dtype, f, 0, None),
           L.mxd_resize_crop_to_device_warp(arr, warps, tones, colors, n, out_dtype, f, 0))
    return rcs, L.mxd_last_error().decode()


CORNER = "matrix maps a corner to a source coordinate of magnitude >= 32768"
BAD_WARPS = [
    ((3, 0, W.IDENTITY), "unknown mode 3"), ((-1, 0, W.IDENTITY), "unknown mode -1"),
    ((W.NEAREST, 0, (1, 0, float("nan"), 0, 1, 0)), "m[2] is not finite"),
    ((W.BILINEAR, 0, (1, 0, 0, 0, float("inf"), 0)), "m[4] is not finite"),
    ((W.NEAREST, 0, W.translate(32768.0, 0.0)), CORNER), ((W.BILINEAR, 0, W.translate(0.0, -32768.0)), CORNER),
    ((W.BILINEAR, 0, (1024.0, 0, 0, 0, 1, 0)), CORNER), ((W.NEAREST, 0, (1, 0, 0, 0, 1, 32768.0 - 32.0)), CORNER),
]


def test_call_refusals_name_the_image_and_the_field():
    import tone_ref

    bad = (capi.MXD_ERR_INVALID,) * 2
    arr, n = capi.make_images([_entry(), _entry()])
    good = capi.make_warps([(W.BILINEAR, 0, W.translate(32735.0, 0.0)), (W.NEAREST, 0, W.IDENTITY)])  # (the corner (32, 0) maps to 32767: inside)
    rcs, msg = _calls(arr, None, None, None, n, capi.MXD_U8, None)
    assert rcs == bad and msg == "mxd: null warps"
    for w, what in BAD_WARPS:
        rcs, msg = _calls(arr, capi.make_warps([(W.NONE, 0, None), w]), None, None, n, capi.MXD_U8, None)
        assert rcs == bad, (what, rcs)
        assert msg == f"mxd_warp: {what} (image 1)", msg
    # MXD_WARP_NONE reads nothing else
    arr1, _ = capi.make_images([_entry(crop_x=8)])
    rcs, msg = _calls(arr1, capi.make_warps([(W.NONE, 0, (float("nan"),) * 6)]), None, None, 1, capi.MXD_U8, None)
    assert rcs == bad and "Array: sub: shape out of bound" in msg  # (the next refusal: geometry)
    arr4, _ = capi.make_images([_entry(), _entry(channels=4, src_stride=256)])
    rcs, msg = _calls(arr4, good, None, None, n, capi.MXD_U8, None)
    assert rcs == bad and msg == "mxd_warp: channels must be 3 (image 1)", msg
    # the tones' checks when there are tones, and the output form's
    rcs, msg = _calls(arr, good, capi.make_tones([(tone_ref.EQUALIZE, 0, 0.0), (tone_ref.POSTERIZE, 9, 0.0)]), None, n,
                      capi.MXD_U8, None)
    assert rcs == bad and "posterize bits" in msg and "(image 1)" in msg, msg
    rcs, msg = _calls(arr, good, None, None, n, 7, None)
    assert rcs == bad and msg == "mxd: bad out_dtype"
    rcs, msg = _calls(arr, good, None, None, n, capi.MXD_U8, capi.make_out_format(elem=9))
    assert rcs == bad and "unknown elem" in msg


def test_jpeg_call_and_cpu_statement_refusals():
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz"))
    coefs = capi.JpegCoefs(gold["caltech_300x200_jpg"])
    L = capi.lib()
    try:
        arr, n = capi.make_jpeg_images([dict(coefs=coefs, resize_w=150, resize_h=100, crop_x=0, crop_y=0, crop_w=150,
                                             crop_h=100, dst=4096, dst_stride=450)])
        assert L.mxd_jpeg_resize_crop_to_device_warp(arr, None, None, None, n, capi.MXD_U8, None, 0) == capi.MXD_ERR_INVALID
        assert L.mxd_last_error() == b"mxd: null warps"
        assert L.mxd_jpeg_resize_crop_to_device_warp(arr, capi.make_warps([(5, 0, W.IDENTITY)]), None, None, n, capi.MXD_U8,
                                                     None, 0) == capi.MXD_ERR_INVALID
        assert L.mxd_last_error() == b"mxd_warp: unknown mode 5 (image 0)"
    finally:
        coefs.close()
    px = np.zeros((4, 4, 3), np.uint8)
    p = ctypes.c_void_p(px.ctypes.data)
    ok = capi.make_warps([(W.NEAREST, 0, W.IDENTITY)])
    assert L.mxd_warp_apply_u8(p, 4, 4, ctypes.c_int64(12), None, p, ctypes.c_int64(12)) == capi.MXD_ERR_INVALID
    assert L.mxd_last_error() == b"mxd: null warps"
    assert L.mxd_warp_apply_u8(None, 4, 4, ctypes.c_int64(12), ok, p, ctypes.c_int64(12)) == capi.MXD_ERR_INVALID
    assert L.mxd_warp_apply_u8(p, 4, 4, ctypes.c_int64(11), ok, p, ctypes.c_int64(12)) == capi.MXD_ERR_INVALID
    for w, what in BAD_WARPS:
        assert L.mxd_warp_apply_u8(p, 32, 32, ctypes.c_int64(96), capi.make_warps([w]), p,
                                   ctypes.c_int64(96)) == capi.MXD_ERR_INVALID
        assert what.encode() in L.mxd_last_error()
        assert L.mxd_warp_validate(capi.make_warps([w]), 32, 32) == capi.MXD_ERR_INVALID
    assert L.mxd_warp_validate(ok, 32, 32) == capi.MXD_OK


def test_every_declared_symbol_is_exported():
    L = capi.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mxd_amd.h")).read()
    assert "#define MXD_HAS_WARP 1" in header and "#define MXD_ABI_VERSION 7" in header
    for name in ("mxd_warp_validate", "mxd_warp_apply_u8", "mxd_resize_crop_batch_warp", "mxd_resize_crop_to_device_warp",
                 "mxd_jpeg_resize_crop_to_device_warp"):
        assert name + "(" in header and name in capi.EXPORTS
        assert getattr(L, name) is not None
    assert ctypes.sizeof(capi.MxdWarp) == 56
    assert "MXD_WARP_NONE = 0, MXD_WARP_NEAREST = 1, MXD_WARP_BILINEAR = 2" in header
    assert (capi.MXD_WARP_NONE, capi.MXD_WARP_NEAREST, capi.MXD_WARP_BILINEAR) == (0, 1, 2)


# ---- the layout of a warp call ------------------------------------------------------

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mlx-data_amd")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_warp_layout_unit(tmp_path):
    """tests/cpp/warp_layout_unit.cpp: a warp batch of mixed routes and code
    paths in the device-free environment -- scratch rows B behind A (none when
    nothing follows the warp), the index tables, the entries, cache keys."""
    exe = str(tmp_path / "warp_layout_unit")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-I", os.path.join(os.path.dirname(HERE), "include"), "-I",
                    os.path.join(PKG, "csrc"), os.path.join(HERE, "cpp", "warp_layout_unit.cpp"), "-L", PKG,
                    "-lmxd_amd", "-Wl,-rpath," + PKG, "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


# ---- operator surface: arguments, the marked plan, what composes, the draws ---------------

def _rgb(h=40, w=60, seed=0, c=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def _buf(n=1, **kw):
    from mlx_data_amd import data as dx

    return dx.buffer_from_vector([dict(image=_rgb(seed=k, **kw)) for k in range(n)])


def _plan(b, i=0, key="image"):
    from mlx_data_amd import _pipeline

    return _pipeline._plan(b, i, key)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("make,word", [
    (lambda b: b.image_affine("image", (1, 0, 0, 0, 1)), "image_affine: matrix must be a sequence of 6 numbers"),
    (lambda b: b.image_affine("image", "abcdef"), "image_affine: matrix must be a sequence of 6 numbers"),
    (lambda b: b.image_affine("image", (1, 0, NAN, 0, 1, 0)), "image_affine: arguments must be finite"),
    (lambda b: b.image_affine("image", W.IDENTITY, resample="bicubic"), "image_affine: unknown resample 'bicubic'"),
    (lambda b: b.image_shear("image", x=INF), "image_shear: arguments must be finite"),
    (lambda b: b.image_shear("image", 0.1, fill=256), "image_shear: fill must be in 0..255"),
    (lambda b: b.image_translate("image", 1, 2, fill=(0, -1, 0)), "image_translate: fill must be in 0..255"),
    (lambda b: b.image_translate("image", 1, 2, fill=(0, 0)), "image_translate: fill must be an integer or"),
    (lambda b: b.image_translate("image", 1, 2, resample="Nearest"), "image_translate: unknown resample"),
    (lambda b: b.image_affine_rotate("image", NAN), "image_affine_rotate: arguments must be finite"),
    (lambda b: b.image_random_shear("image", x=(0.3, -0.3)), "image_random_shear: x range has lo > hi"),
    (lambda b: b.image_random_shear("image", y=(0.0, INF)), "image_random_shear: y range must be finite"),
    (lambda b: b.image_random_translate("image", x=3.0), "image_random_translate: x must be None or a (lo, hi) pair"),
    (lambda b: b.image_random_affine_rotate("image", (30, -30)), "image_random_affine_rotate: angle range has lo > hi"),
    (lambda b: b.image_random_affine_rotate("image", None), "image_random_affine_rotate: angle must be a (lo, hi) pair"),
    (lambda b: b.to_stream().image_shear("image", 0.1, fill=300), "image_shear: fill must be in 0..255"),
])
def test_surface_refuses_bad_arguments_when_the_op_is_made(make, word):
    with pytest.raises(ValueError) as err:
        make(_buf())
    assert word in str(err.value), str(err.value)


OPS = [("image_affine", lambda b, **kw: b.image_affine("image", (1, 0.25, -2, 0.5, 1, 3), **kw), (1.0, 0.25, -2.0, 0.5, 1.0, 3.0)),
       ("image_shear", lambda b, **kw: b.image_shear("image", 0.3, -0.1, **kw), W.shear(0.3, -0.1)),
       ("image_translate", lambda b, **kw: b.image_translate("image", 2.5, y=-4, **kw), W.translate(2.5, -4.0)),
       ("image_affine_rotate", lambda b, **kw: b.image_affine_rotate("image", 30.0, **kw), W.rotate_matrix(30, 20, 30.0)),
       ("image_random_shear", lambda b, **kw: b.image_random_shear("image", x=(0.2, 0.2), **kw), W.shear(0.2, 0.0)),
       ("image_random_translate", lambda b, **kw: b.image_random_translate("image", y=(3, 3), **kw), W.translate(0.0, 3.0)),
       ("image_random_affine_rotate", lambda b, **kw: b.image_random_affine_rotate("image", (-45, -45), **kw),
        W.rotate_matrix(30, 20, -45.0))]


def test_surface_refuses_non_rgb_images_and_matrices_past_the_bound_when_the_op_is_applied():
    for c in (1, 2, 4):
        for name, make, _ in OPS:
            b = make(_buf(c=c))  # made without complaint
            with pytest.raises(RuntimeError) as err:
                b[0]
            assert str(err.value) == f"{name}: image must have 3 channels, not {c}", str(err.value)
    b = _buf().image_translate("image", 40000.0)
    with pytest.raises(RuntimeError) as err:
        b[0]
    assert str(err.value) == "image_translate: mxd_warp: " + CORNER, str(err.value)


def test_the_op_marks_the_plan_and_what_composes_composes():
    b = _buf().image_resize("image", 30, 20)
    q = _plan(b)
    assert q["warp"] is None
    for name, make, m in OPS:
        t = make(b, resample="bilinear", fill=(1, 2, 3))
        p = _plan(t)
        assert p["warp"] == ("bilinear", (1, 2, 3), m), (name, p["warp"])
        assert {k: p[k] for k in p if k != "warp"} == {k: q[k] for k in q if k != "warp"}  # nothing else touched
        assert _plan(make(b))["warp"] == ("nearest", (0, 0, 0), m)  # the defaults
        assert _plan(make(b, fill=7))["warp"][1] == (7, 7, 7)
        # a tone op, a colour op, image_to_float and image_normalize compose on the warped plan
        e = _plan(t.image_equalize("image").image_color_twist("image", 1.2, 0.5))
        assert e["warp"] == p["warp"] and e["tone"] == ("equalize", None)
        assert np.array_equal(np.float32(e["color"]), capi.color_twist_matrix(1.2, 0.5))
        assert e["resize"] == (30, 20) and e["window"] == (0, 0, 60, 40)
        fl = _plan(t.image_to_float("image"))
        assert fl["warp"] == p["warp"] and fl["shape"] == [20, 30, 3] and fl["window"] == (0, 0, 60, 40)
        n = _plan(t.image_normalize("image", mean=0.5, std=0.5, dtype="bfloat16", layout="chw"))
        assert n["warp"] == p["warp"] and n["format"]["dtype"] == "bfloat16" and n["shape"] == [3, 20, 30]
        # output_key
        o = make(b, output_key="warped")
        assert _plan(o, 0, "warped")["warp"] is not None and _plan(o, 0, "image")["warp"] is None
    # crops and flips before the warp are part of the plan it marks; the rotate matrix is that of the crop
    pre = _plan(b.image_center_crop("image", 10, 8).image_random_h_flip("image", 1.0).image_affine_rotate("image", 30.0))
    assert pre["crop"] == (10, 6, 10, 8) and pre["flip"] and pre["resize"] == (30, 20)
    assert pre["warp"] == ("nearest", (0, 0, 0), W.rotate_matrix(10, 8, 30.0))
    # the _if forms
    assert _plan(b.image_affine_if(False, "image", W.IDENTITY))["warp"] is None
    assert _plan(b.image_shear_if(True, "image", 0.5))["warp"][2] == W.shear(0.5, 0.0)
    assert _plan(b.image_translate_if(False, "image", 1.0))["warp"] is None
    assert _plan(b.image_affine_rotate_if(True, "image", 90.0))["warp"][2] == W.rotate_matrix(30, 20, 90.0)
    assert _plan(b.image_random_shear_if(False, "image", x=(0, 1)))["warp"] is None
    assert _plan(b.image_random_translate_if(True, "image", x=(2, 2)))["warp"][2] == W.translate(2.0, 0.0)
    assert _plan(b.image_random_affine_rotate_if(False, "image", (0, 1)))["warp"] is None
    # on a stream too
    s = _buf().to_stream().image_shear("image", 0.1).image_random_affine_rotate_if(False, "image", (0, 9))
    assert s is not None


def test_the_random_ops_draw_one_uniform_double_per_given_range():
    """std::uniform_real_distribution<double> over the thread's mt19937, x then
    y: libstdc++'s generate_canonical<double, 53> takes two 32-bit outputs per
    draw, low word first, and the distribution returns u * (hi - lo) + lo."""
    from mlx_data_amd import data as dx

    def draws(seed, ranges):
        words = np.random.RandomState(seed)  # the same mt19937 seeding as std::mt19937(seed)
        out = []
        for lo, hi in ranges:
            r0, r1 = (int(words.randint(0, 2 ** 32, dtype=np.uint64)) for _ in range(2))
            u = (float(r0) + float(r1) * 4294967296.0) / 18446744073709551616.0
            out.append(u * (float(hi) - float(lo)) + float(lo))
        return out

    b = _buf(4)
    dx.set_state(11)
    x, y = draws(11, [(-0.3, 0.3), (0.1, 0.2)])
    assert _plan(b.image_random_shear("image", x=(-0.3, 0.3), y=(0.1, 0.2)), 0)["warp"][2] == W.shear(x, y)
    # a None draws nothing: y takes the first draw
    dx.set_state(12)
    (y,) = draws(12, [(-8, 8)])
    assert _plan(b.image_random_translate("image", y=(-8, 8)), 0)["warp"][2] == W.translate(0.0, y)
    dx.set_state(13)
    (a,) = draws(13, [(-30, 30)])
    assert _plan(b.image_random_affine_rotate("image", (-30, 30)), 0)["warp"][2] == W.rotate_matrix(60, 40, a)
    # the same seed, the same draws; another seed, others; the images of a buffer differ
    op = b.image_random_translate("image", x=(-8, 8), y=(-8, 8))

    def draw(seed):
        dx.set_state(seed)
        return [_plan(op, i)["warp"][2] for i in range(4)]

    one, again, other = draw(7), draw(7), draw(8)
    assert one == again and one != other and len(set(one)) == 4
    assert all(-8 <= m[2] <= 8 and -8 <= m[5] <= 8 and m[:2] + m[3:5] == (1.0, 0.0, 0.0, 1.0) for m in one)
