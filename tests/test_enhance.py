"""The per-image enhance ops on the CPU (no device): the CPU statement of the
C ABI (mxd_enhance_apply_u8) byte-equal to Pillow's ImageEnhance.Sharpness /
Color / Brightness and to the NumPy restatement, the refusals of the C ABI
with their messages, the enhance call's batch layout in the device-free
environment (tests/cpp/enhance_layout_unit.cpp), and the operator surface's
enhance ops as far as they go without a device (arguments, the marked plan,
what composes and what materialises, the random ops' draws)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import enhance_ref as E
from mlx_data_amd import capi

SIZES = [(1, 1), (9, 2), (2, 9), (3, 3), (3, 4), (53, 37)]  # (h, w): windows 1x1, 2x9, 9x2, 3x3, 4x3, 37x53
FACTORS = [0.0, 0.1, 0.5, 1.0, 1.9, 2.0, 7.5]


# ---- the CPU statement against Pillow and the restatement ---------------------------------

@pytest.mark.parametrize("op", E.OPS, ids=E.OP_IDS)
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for h, w in SIZES])
def test_apply_u8_equals_pillow_and_the_restatement(size, op):
    """Random, 0 / 255 and smooth-ramp inputs at every factor; then the same
    through strided inputs and outputs."""
    h, w = size
    for name, img in E.inputs(w, h, 100 * h + w).items():
        for f in FACTORS:
            enh = (op, f)
            want = E.pillow_apply(img, enh)
            got = capi.enhance_apply_u8(img, enh)
            assert np.array_equal(got, want), (name, f, int((got != want).sum()))
            assert np.array_equal(E.apply(img, enh), want), (name, f)
            if f == 1.0:
                assert np.array_equal(got, img)
            if f == 0.0:
                assert np.array_equal(got, E.degenerate(img, op).astype(np.uint8))
            wide = np.full((h, w + 3, 3), 0xEE, np.uint8)
            wide[:, 1:w + 1] = img
            out = np.full((h, w + 5, 3), 0xDD, np.uint8)
            capi.enhance_apply_u8(wide[:, 1:w + 1], enh, out[:, 2:w + 2])
            assert np.array_equal(out[:, 2:w + 2], want), (name, f)
            assert (out[:, :2] == 0xDD).all() and (out[:, w + 2:] == 0xDD).all()


def test_the_binary_input_drives_the_clip_branch_and_smooth_is_pillows():
    from PIL import Image, ImageFilter

    img = E.inputs(37, 53, 3)["binary"]
    d = E.degenerate(img, E.SHARPNESS)
    x = d + 7.5 * (img.astype(np.int32) - d)
    assert (x < 0).any() and (x > 255).any()
    assert np.array_equal(d.astype(np.uint8), np.asarray(Image.fromarray(img).filter(ImageFilter.SMOOTH)))
    assert np.array_equal(capi.enhance_apply_u8(img, (E.NONE, 3.0)), img)


# ---- refusals ----------------------------------------------------------------------------

def _entry(**kw):
    e = dict(src=4096, dst=4096, src_stride=64 * 3, src_w=64, src_h=64, channels=3, resize_w=32, resize_h=32, crop_x=0,
             crop_y=0, crop_w=32, crop_h=32, dst_stride=32 * 3 * 4)
    e.update(kw)
    return e


def _calls(arr, warps, enhs, tones, colors, n, out_dtype, fmt):
    """The status of the two calls that take mxd_image, and the last message."""
    L = capi.lib()
    f = ctypes.byref(fmt) if fmt is not None else None
    rcs = (L.mxd_resize_crop_batch_enhance(arr, warps, enhs, tones, colors, n, out_dtype, f, 0, None),
           L.mxd_resize_crop_to_device_enhance(arr, warps, enhs, tones, colors, n, out_dtype, f, 0))
    return rcs, L.mxd_last_error().decode()


def _reserved(k):
    e = capi.MxdEnhance()
    e.op, e.factor = E.COLOR, 1.0
    e.reserved[k] = 1
    return e


FACTOR = "factor must be finite and in 0..1e6"
BAD_ENHANCES = [
    ((4, 1.0), "unknown op 4"), ((-1, 1.0), "unknown op -1"),
    ((E.SHARPNESS, -0.5), FACTOR), ((E.COLOR, float("nan")), FACTOR), ((E.BRIGHTNESS, float("inf")), FACTOR),
    ((E.SHARPNESS, 1.5e6), FACTOR), (_reserved(0), "reserved must be 0"), (_reserved(1), "reserved must be 0"),
]


def test_call_refusals_name_the_image_and_the_field():
    import tone_ref
    import warp_ref

    bad = (capi.MXD_ERR_INVALID,) * 2
    arr, n = capi.make_images([_entry(), _entry()])
    good = capi.make_enhances([(E.SHARPNESS, 1e6), (E.COLOR, 0.0)])
    rcs, msg = _calls(arr, None, None, None, None, n, capi.MXD_U8, None)
    assert rcs == bad and msg == "mxd: null enhances"
    for e, what in BAD_ENHANCES:
        rcs, msg = _calls(arr, None, capi.make_enhances([(E.NONE, 0.0), e]), None, None, n, capi.MXD_U8, None)
        assert rcs == bad, (what, rcs)
        assert msg == f"mxd_enhance: {what} (image 1)", msg
    # MXD_ENHANCE_NONE reads no factor
    arr1, _ = capi.make_images([_entry(crop_x=8)])
    rcs, msg = _calls(arr1, None, capi.make_enhances([(E.NONE, float("nan"))]), None, None, 1, capi.MXD_U8, None)
    assert rcs == bad and "Array: sub: shape out of bound" in msg  # (the next refusal: geometry)
    arr4, _ = capi.make_images([_entry(), _entry(channels=4, src_stride=256)])
    rcs, msg = _calls(arr4, None, good, None, None, n, capi.MXD_U8, None)
    assert rcs == bad and msg == "mxd_enhance: channels must be 3 (image 1)", msg
    # the warps' and tones' checks when there are some, and the output form's
    rcs, msg = _calls(arr, capi.make_warps([(warp_ref.NONE, 0, None), (7, 0, warp_ref.IDENTITY)]), good, None, None, n,
                      capi.MXD_U8, None)
    assert rcs == bad and msg == "mxd_warp: unknown mode 7 (image 1)", msg
    rcs, msg = _calls(arr, None, good, capi.make_tones([(tone_ref.EQUALIZE, 0, 0.0), (tone_ref.POSTERIZE, 9, 0.0)]),
                      None, n, capi.MXD_U8, None)
    assert rcs == bad and "posterize bits" in msg and "(image 1)" in msg, msg
    rcs, msg = _calls(arr, None, good, None, None, n, 7, None)
    assert rcs == bad and msg == "mxd: bad out_dtype"
    rcs, msg = _calls(arr, None, good, None, None, n, capi.MXD_U8, capi.make_out_format(elem=9))
    assert rcs == bad and "unknown elem" in msg


def test_jpeg_call_and_cpu_statement_refusals():
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz"))
    coefs = capi.JpegCoefs(gold["caltech_300x200_jpg"])
    L = capi.lib()
    try:
        arr, n = capi.make_jpeg_images([dict(coefs=coefs, resize_w=150, resize_h=100, crop_x=0, crop_y=0, crop_w=150,
                                             crop_h=100, dst=4096, dst_stride=450)])
        assert L.mxd_jpeg_resize_crop_to_device_enhance(arr, None, None, None, None, n, capi.MXD_U8, None,
                                                        0) == capi.MXD_ERR_INVALID
        assert L.mxd_last_error() == b"mxd: null enhances"
        assert L.mxd_jpeg_resize_crop_to_device_enhance(arr, None, capi.make_enhances([(5, 1.0)]), None, None, n,
                                                        capi.MXD_U8, None, 0) == capi.MXD_ERR_INVALID
        assert L.mxd_last_error() == b"mxd_enhance: unknown op 5 (image 0)"
    finally:
        coefs.close()
    px, other = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8)
    p, o = ctypes.c_void_p(px.ctypes.data), ctypes.c_void_p(other.ctypes.data)
    ok = capi.make_enhances([(E.SHARPNESS, 1.5)])
    s12, s11 = ctypes.c_int64(12), ctypes.c_int64(11)
    assert L.mxd_enhance_apply_u8(p, 4, 4, s12, None, o, s12) == capi.MXD_ERR_INVALID
    assert L.mxd_last_error() == b"mxd: null enhances"
    assert L.mxd_enhance_apply_u8(None, 4, 4, s12, ok, o, s12) == capi.MXD_ERR_INVALID
    assert L.mxd_enhance_apply_u8(p, 4, 4, s11, ok, o, s12) == capi.MXD_ERR_INVALID
    assert L.mxd_enhance_apply_u8(p, 4, 4, s12, ok, p, s12) == capi.MXD_ERR_INVALID  # out overlaps rgb
    assert L.mxd_last_error() == b"mxd_enhance: out overlaps rgb"
    assert L.mxd_enhance_apply_u8(p, 4, 4, s12, ok, o, s12) == capi.MXD_OK
    for e, what in BAD_ENHANCES:
        assert L.mxd_enhance_apply_u8(p, 4, 4, s12, capi.make_enhances([e]), o, s12) == capi.MXD_ERR_INVALID
        assert L.mxd_last_error().decode() == f"mxd_enhance: {what} (image 0)"
        assert L.mxd_enhance_validate(capi.make_enhances([e])) == capi.MXD_ERR_INVALID
    assert L.mxd_enhance_validate(ok) == capi.MXD_OK
    assert L.mxd_enhance_validate(None) == capi.MXD_ERR_INVALID


def test_every_declared_symbol_is_exported():
    L = capi.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mxd_amd.h")).read()
    assert "#define MXD_HAS_ENHANCE 1" in header and "#define MXD_ABI_VERSION 7" in header
    assert capi.lib().mxd_abi_version() == 7
    for name in ("mxd_enhance_validate", "mxd_enhance_apply_u8", "mxd_resize_crop_batch_enhance",
                 "mxd_resize_crop_to_device_enhance", "mxd_jpeg_resize_crop_to_device_enhance"):
        assert name + "(" in header and name in capi.EXPORTS
        assert getattr(L, name) is not None
    assert ctypes.sizeof(capi.MxdEnhance) == 16
    for name, value in (("NONE", 0), ("SHARPNESS", 1), ("COLOR", 2), ("BRIGHTNESS", 3)):
        assert f"MXD_ENHANCE_{name} = {value}" in header and getattr(capi, f"MXD_ENHANCE_{name}") == value


# ---- the layout of an enhance call ----------------------------------------------------

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mlx-data_amd")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_enhance_layout_unit(tmp_path):
    """tests/cpp/enhance_layout_unit.cpp: an enhance batch of mixed routes and
    ops in the device-free environment, with and without a warp, a tone, a
    matrix and a format -- which rows the stage reads and writes (A to B, B
    to A behind a warp, the destinations when nothing follows), no third
    scratch, the entries, cache keys, a chunk's slice."""
    exe = str(tmp_path / "enhance_layout_unit")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-I", os.path.join(os.path.dirname(HERE), "include"), "-I",
                    os.path.join(PKG, "csrc"), os.path.join(HERE, "cpp", "enhance_layout_unit.cpp"), "-L", PKG,
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
NAMES = ["sharpness", "color", "brightness"]


@pytest.mark.parametrize("make,word", [
    (lambda b: b.image_sharpness("image", -0.1), "image_sharpness: factor must be finite and in 0..1e6"),
    (lambda b: b.image_color("image", NAN), "image_color: factor must be finite and in 0..1e6"),
    (lambda b: b.image_brightness("image", INF), "image_brightness: factor must be finite and in 0..1e6"),
    (lambda b: b.image_brightness("image", 1e6 + 1), "image_brightness: factor must be finite and in 0..1e6"),
    (lambda b: b.image_random_sharpness("image", factor=(1.5, 0.5)), "image_random_sharpness: factor range has lo > hi"),
    (lambda b: b.image_random_color("image", factor=(-1.0, 0.5)),
     "image_random_color: factor range must be finite and in 0..1e6"),
    (lambda b: b.image_random_brightness("image", factor=(0.0, INF)),
     "image_random_brightness: factor range must be finite and in 0..1e6"),
    (lambda b: b.image_random_brightness("image", factor=1.0), "image_random_brightness: factor must be a (lo, hi) pair"),
    (lambda b: b.to_stream().image_color("image", -2.0), "image_color: factor must be finite and in 0..1e6"),
])
def test_surface_refuses_bad_arguments_when_the_op_is_made(make, word):
    with pytest.raises(ValueError) as err:
        make(_buf())
    assert word in str(err.value), str(err.value)


def _fixed(name):
    return lambda b, f=1.5, **kw: getattr(b, "image_" + name)("image", f, **kw)


def _random(name):
    return lambda b, f=1.5, **kw: getattr(b, "image_random_" + name)("image", factor=(f, f), **kw)


OPS = [("image_" + n, n, _fixed(n)) for n in NAMES] + [("image_random_" + n, n, _random(n)) for n in NAMES]


def test_surface_refuses_non_rgb_images_when_the_op_is_applied():
    for c in (1, 2, 4):
        for name, _, make in OPS:
            b = make(_buf(c=c))  # made without complaint
            with pytest.raises(RuntimeError) as err:
                b[0]
            assert str(err.value) == f"{name}: image must have 3 channels, not {c}", str(err.value)


def test_the_op_marks_the_plan_and_what_composes_composes():
    b = _buf().image_resize("image", 30, 20)
    q = _plan(b)
    assert q["enhance"] is None
    for name, short, make in OPS:
        t = make(b)
        p = _plan(t)
        assert p["enhance"] == (short, 1.5), (name, p["enhance"])
        assert {k: p[k] for k in p if k != "enhance"} == {k: q[k] for k in q if k != "enhance"}  # nothing else touched
        assert _plan(make(b, 0.1))["enhance"] == (short, float(np.float32(0.1)))  # the factor as float32
        # a tone op, a colour op, image_to_float and image_normalize compose on the enhanced plan
        e = _plan(t.image_equalize("image").image_color_twist("image", 1.2, 0.5))
        assert e["enhance"] == p["enhance"] and e["tone"] == ("equalize", None)
        assert np.array_equal(np.float32(e["color"]), capi.color_twist_matrix(1.2, 0.5))
        assert e["resize"] == (30, 20) and e["window"] == (0, 0, 60, 40)
        fl = _plan(t.image_to_float("image"))
        assert fl["enhance"] == p["enhance"] and fl["shape"] == [20, 30, 3] and fl["window"] == (0, 0, 60, 40)
        n = _plan(t.image_normalize("image", mean=0.5, std=0.5, dtype="bfloat16", layout="chw"))
        assert n["enhance"] == p["enhance"] and n["format"]["dtype"] == "bfloat16" and n["shape"] == [3, 20, 30]
        # image_random_h_flip composes after all three ops
        fp = _plan(t.image_random_h_flip("image", 1.0))
        assert fp["enhance"] == p["enhance"] and fp["flip"] and fp["resize"] == (30, 20) and fp["window"] == (0, 0, 60, 40)
        # an enhance op on a warped plan composes
        wp = _plan(make(b.image_shear("image", 0.3)))
        assert wp["enhance"] == p["enhance"] and wp["warp"] is not None and wp["resize"] == (30, 20)
        # output_key
        o = make(b, output_key="enhanced")
        assert _plan(o, 0, "enhanced")["enhance"] is not None and _plan(o, 0, "image")["enhance"] is None
    # a crop composes after color and brightness: the same plan as the crop before the op
    for short in ("color", "brightness"):
        t = _fixed(short)(b)
        c = _plan(t.image_center_crop("image", 10, 8))
        assert c["enhance"] == (short, 1.5) and c["crop"] == (10, 6, 10, 8) and c["resize"] == (30, 20)
        assert c == _plan(_fixed(short)(b.image_center_crop("image", 10, 8)))
    # crops and flips before the op are part of the plan it marks
    pre = _plan(b.image_center_crop("image", 10, 8).image_random_h_flip("image", 1.0).image_sharpness("image", 0.5))
    assert pre["crop"] == (10, 6, 10, 8) and pre["flip"] and pre["resize"] == (30, 20) and pre["enhance"] == ("sharpness", 0.5)
    # the _if forms
    assert _plan(b.image_sharpness_if(False, "image", 2.0))["enhance"] is None
    assert _plan(b.image_sharpness_if(True, "image", 2.0))["enhance"] == ("sharpness", 2.0)
    assert _plan(b.image_color_if(True, "image", 0.5))["enhance"] == ("color", 0.5)
    assert _plan(b.image_brightness_if(False, "image", 0.5))["enhance"] is None
    assert _plan(b.image_random_sharpness_if(False, "image", factor=(0, 1)))["enhance"] is None
    assert _plan(b.image_random_color_if(True, "image", factor=(2, 2)))["enhance"] == ("color", 2.0)
    assert _plan(b.image_random_brightness_if(False, "image", factor=(0, 1)))["enhance"] is None
    # on a stream too, and through the compat package
    s = _buf().to_stream().image_sharpness("image", 0.1).image_random_color_if(False, "image", factor=(0, 9))
    assert s is not None


def test_the_compat_package_carries_the_ops():
    import sys

    compat = os.path.join(PKG, "compat")
    sys.path.insert(0, compat)
    try:
        import mlx.data as md
    finally:
        sys.path.remove(compat)
    for cls in (md.Buffer, md.Stream):
        for n in NAMES:
            for form in ("image_" + n, "image_random_" + n, f"image_{n}_if", f"image_random_{n}_if"):
                assert callable(getattr(cls, form)), (cls, form)


# ---- operator surface: what materialises -------------------------------------------------

NO_DEVICE = "mxd: no HIP device visible"


def _materialised(make_chain):
    """The plan the chain leaves, given that its last op had to run what was
    pending: the new source is the 30 x 20 result.  Without a device the
    pending launch cannot run and the attempt itself is the evidence."""
    try:
        p = _plan(make_chain())
    except RuntimeError as err:
        assert NO_DEVICE in str(err), str(err)
        return None
    assert p["src_shape"] == [20, 30, 3] and p["window"][:2] == (0, 0), p
    return p


def test_what_materialises_the_pending_plan():
    b = _buf().image_resize("image", 30, 20)
    for name, short, make in OPS:
        t = make(b)
        assert _plan(t)["src_shape"] == [40, 60, 3]  # (pending: the source is still the 40 x 60 image)
        # a resize, image_rotate, a warp op or a second enhance op on an enhanced plan
        p = _materialised(lambda: t.image_resize("image", 15, 10))
        assert p is None or (p["enhance"] is None and p["resize"] == (15, 10))
        p = _materialised(lambda: t.image_shear("image", 0.3))
        assert p is None or (p["enhance"] is None and p["warp"] is not None)
        p = _materialised(lambda: t.image_brightness("image", 0.5))
        assert p is None or p["enhance"] == ("brightness", 0.5)
        try:
            r = t.image_rotate("image", 90.0)[0]["image"]
            assert r.shape == b.image_rotate("image", 90.0)[0]["image"].shape  # (the op ran on the enhanced bytes)
        except RuntimeError as err:
            assert NO_DEVICE in str(err), str(err)
        # an enhance op on a plan that is already toned or coloured
        p = _materialised(lambda: make(b.image_posterize("image", 4)))
        assert p is None or (p["enhance"] == (short, 1.5) and p["tone"] is None)
        p = _materialised(lambda: make(b.image_color_twist("image", 1.2)))
        assert p is None or (p["enhance"] == (short, 1.5) and p["color"] is None)
    # a crop after SHARPNESS: the copied ring is the uncropped window's
    p = _materialised(lambda: b.image_sharpness("image", 1.5).image_center_crop("image", 10, 8))
    assert p is None or (p["enhance"] is None and p["crop"] == (10, 6, 10, 8))
    p = _materialised(lambda: b.image_random_sharpness("image", factor=(0.5, 1.5)).image_random_crop("image", 10, 8))
    assert p is None or p["enhance"] is None


def test_the_random_ops_draw_one_uniform_double_per_image():
    """std::uniform_real_distribution<double> over the thread's mt19937:
    libstdc++'s generate_canonical<double, 53> takes two 32-bit outputs per
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
    for seed, short, (lo, hi) in ((11, "sharpness", (0.1, 1.9)), (12, "color", (0.0, 2.0)), (13, "brightness", (0.5, 1.5))):
        dx.set_state(seed)
        (f,) = draws(seed, [(lo, hi)])
        got = _plan(getattr(b, "image_random_" + short)("image", factor=(lo, hi)), 0)["enhance"]
        assert got == (short, float(np.float32(f))), (short, got, f)
    # the same seed, the same draws; another seed, others; the images of a buffer differ
    op = b.image_random_sharpness("image", factor=(0.1, 1.9))

    def draw(seed):
        dx.set_state(seed)
        return [_plan(op, i)["enhance"][1] for i in range(4)]

    one, again, other = draw(7), draw(7), draw(8)
    assert one == again and one != other and len(set(one)) == 4
    assert all(0.1 <= f <= 1.9 for f in one)
