"""The per-image colour transform on the CPU (no device): the twist matrix
against a float64 NumPy restatement, the CPU statement of the map bit-equal to
the NumPy expression on every RGB triple, the refusals of the C ABI with their
messages, the colour call's batch layout in the device-free environment
(tests/cpp/color_layout_unit.cpp), and the operator surface's colour ops as
far as they go without a device (arguments, the marked plan, the random
draws).  References: tests/color_ref.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import color_ref as R
from mlx_data_amd import capi


# ---- the twist matrix -----------------------------------------------------------

def _unit(m):
    """A library matrix (byte units) in the [0, 1] units it is specified in."""
    m = np.asarray(m, np.float64).copy()
    m[:, 3] /= 255.0
    return m


def test_twist_matrix_against_the_float64_restatement():
    """200 seeded parameter sets, factors in [0, 2], hue in [-180, 180]: within
    1e-6 per entry, in the [0, 1] units the matrix is defined in.  The entries
    of such a product stay below 16 in magnitude, where half a float32 ulp is
    4.8e-7: the one rounding to float the specification allows fits 1e-6."""
    rng = np.random.default_rng(2024)
    worst = 0.0
    for _ in range(200):
        b, c, s = rng.uniform(0, 2, 3)
        h = rng.uniform(-180, 180)
        ref = R.twist_ref(b, c, s, h)
        assert np.abs(ref).max() < 16
        worst = max(worst, np.abs(_unit(capi.color_twist_matrix(b, c, s, h)) - ref).max())
    print("worst entry error", worst)
    assert worst <= 1e-6


def test_twist_defaults_are_exactly_the_identity():
    assert np.array_equal(capi.color_twist_matrix(), R.IDENTITY)
    assert np.array_equal(capi.color_twist_matrix(1.0, 1.0, 1.0, 0.0), R.IDENTITY)


def test_twist_single_factors_in_closed_form():
    w = R.YIQ[0]
    for b in (0.0, 0.25, 1.7):
        assert np.array_equal(capi.color_twist_matrix(brightness=b), (b * np.eye(3, 4)).astype(np.float32))
    for c in (0.0, 0.5, 1.5):
        want = np.concatenate([c * np.eye(3), np.full((3, 1), 0.5 * (1 - c) * 255.0)], axis=1).astype(np.float32)
        assert np.array_equal(capi.color_twist_matrix(contrast=c), want)
    for s in (0.0, 0.4, 2.0):
        want = np.concatenate([s * np.eye(3) + (1 - s) * np.outer(np.ones(3), w), np.zeros((3, 1))], axis=1)
        assert np.array_equal(capi.color_twist_matrix(saturation=s), want.astype(np.float32))
    # S(0): three rows equal to the luma weights
    assert np.array_equal(capi.color_twist_matrix(saturation=0.0)[:, :3], np.tile(w.astype(np.float32), (3, 1)))
    for h in (-120.0, 33.0, 90.0, 360.0):
        a = np.radians(h)
        rot = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        want = np.concatenate([np.linalg.inv(R.YIQ) @ rot @ R.YIQ, np.zeros((3, 1))], axis=1)
        assert np.abs(capi.color_twist_matrix(hue=h).astype(np.float64) - want).max() <= 1e-6
    assert np.abs(capi.color_twist_matrix(hue=360.0) - R.IDENTITY).max() <= 1e-6
    # brightness scales the contrast offset too: 1.2 * (0.5 I, 0.25) = (0.6 I, 0.3) -> 76.5 in byte units
    want = np.concatenate([0.6 * np.eye(3), np.full((3, 1), 76.5)], axis=1).astype(np.float32)
    assert np.abs(capi.color_twist_matrix(1.2, 0.5) - want).max() <= 1e-5
    assert np.abs(_unit(capi.color_twist_matrix(1.2, 0.5)) - _unit(want)).max() <= 1e-6


@pytest.mark.parametrize("args,word", [
    ((-0.1, 1, 1, 0), "brightness"), ((float("nan"), 1, 1, 0), "brightness"), ((1, -1e-9, 1, 0), "contrast"),
    ((1, float("inf"), 1, 0), "contrast"), ((1, 1, -2, 0), "saturation"), ((1, 1, float("nan"), 0), "saturation"),
    ((1, 1, 1, float("inf")), "hue"), ((1, 1, 1, float("nan")), "hue")])
def test_twist_refusals(args, word):
    with pytest.raises(capi.MxdError) as err:
        capi.color_twist_matrix(*args)
    assert err.value.code == capi.MXD_ERR_INVALID
    assert str(err.value).startswith("mxd_color_twist_matrix: " + word)
    assert capi.lib().mxd_color_twist_matrix(ctypes.c_double(1), ctypes.c_double(1), ctypes.c_double(1),
                                             ctypes.c_double(0), None) == capi.MXD_ERR_INVALID


# ---- the CPU statement ------------------------------------------------------------

@pytest.fixture(scope="module")
def all_triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16).astype(np.uint8), (v >> 8).astype(np.uint8), v.astype(np.uint8)], axis=1)


@pytest.mark.parametrize("name", ["CLAMPING", "NEGATIVE", "SWAP", "IDENTITY"])
def test_apply_u8_on_every_triple(all_triples, name):
    m = getattr(R, name)
    got = capi.color_apply_u8(all_triples, m)
    want = R.apply_ref(all_triples, m)
    assert np.array_equal(got, want), np.argwhere(got != want)[:3]
    if name == "IDENTITY":
        assert np.array_equal(got, all_triples)
    if name == "SWAP":
        assert np.array_equal(got, all_triples[:, ::-1])
    if name == "CLAMPING":
        assert (got == 0).any() and (got == 255).any()


def test_a_tiny_entry_acts_as_zero():
    rng = np.random.default_rng(7)
    px = rng.integers(0, 256, (4096, 3), dtype=np.uint8)
    m = R.NEGATIVE.copy()
    z = m.copy()
    m[0, 1], m[2, 3], z[0, 1], z[2, 3] = 1e-42, -1e-42, 0.0, 0.0
    assert np.float32(1e-42) != 0
    assert np.array_equal(capi.color_apply_u8(px, m), capi.color_apply_u8(px, z))
    assert np.array_equal(capi.color_apply_u8(px, m), R.apply_ref(px, z))
    # 2^-100 itself is kept
    k = R.IDENTITY.copy()
    k[1, 0] = 2.0 ** -100
    assert np.array_equal(capi.color_apply_u8(px, k), R.apply_ref(px, k))


# ---- refusals of the calls ---------------------------------------------------------

def _entry(**kw):
    e = dict(src=4096, dst=4096, src_stride=64 * 3, src_w=64, src_h=64, channels=3, resize_w=32, resize_h=32, crop_x=0,
             crop_y=0, crop_w=32, crop_h=32, dst_stride=32 * 3 * 4)
    e.update(kw)
    return e


def _calls(arr, colors, n, out_dtype, fmt):
    """The status of the two calls that take mxd_image, and the last message."""
    L = capi.lib()
    f = ctypes.byref(fmt) if fmt is not None else None
    rcs = (L.mxd_resize_crop_batch_color(arr, colors, n, out_dtype, f, 0, None),
           L.mxd_resize_crop_to_device_color(arr, colors, n, out_dtype, f, 0))
    return rcs, L.mxd_last_error().decode()


def test_call_refusals_name_the_image_and_the_field():
    arr, n = capi.make_images([_entry(), _entry()])
    good = capi.make_colors([R.IDENTITY, R.SWAP])
    rcs, msg = _calls(arr, None, n, capi.MXD_U8, None)
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and msg == "mxd: null colors"
    for bad, what in ((float("nan"), "not finite"), (float("inf"), "not finite"), (2e6, "larger than 1e6"),
                      (-1.5e6, "larger than 1e6")):
        m = R.SWAP.copy()
        m[2, 1] = bad
        rcs, msg = _calls(arr, capi.make_colors([R.IDENTITY, m]), n, capi.MXD_U8, None)
        assert rcs == (capi.MXD_ERR_INVALID,) * 2, (bad, rcs)
        assert "m[2][1]" in msg and what in msg and "(image 1)" in msg, msg
    m = R.SWAP.copy()
    m[0, 3] = 1e6  # the bound itself is allowed: the next refusal is another one
    arr4, _ = capi.make_images([_entry(), _entry(channels=4, src_stride=256)])
    rcs, msg = _calls(arr4, capi.make_colors([m, R.IDENTITY]), n, capi.MXD_U8, None)
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and msg == "mxd_color: channels must be 3 (image 1)", msg
    rcs, msg = _calls(arr, good, n, 7, None)
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and msg == "mxd: bad out_dtype"
    # every check of the _fmt calls applies when fmt is given
    rcs, msg = _calls(arr, good, n, capi.MXD_U8, capi.make_out_format(elem=9))
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and "unknown elem" in msg
    rcs, msg = _calls(arr, good, n, capi.MXD_U8, capi.make_out_format(capi.MXD_ELEM_F16, std=0.0))
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and "std[0]" in msg
    odd, _ = capi.make_images([_entry(), _entry(dst=4097)])
    rcs, msg = _calls(odd, good, n, capi.MXD_U8, capi.make_out_format(capi.MXD_ELEM_F16))
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and "dst is not a multiple of the element size (image 1)" in msg
    rcs, msg = _calls(arr, good, n, capi.MXD_U8,
                      capi.make_out_format(capi.MXD_ELEM_F32, capi.MXD_LAYOUT_CHW, plane_stride=64))
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and "plane_stride smaller than crop_h * dst_stride" in msg
    # MXD_F32_DIV255 without a format: the checks of the {F32, HWC} format
    short, _ = capi.make_images([_entry(), _entry(dst_stride=32 * 3 * 4 - 4)])
    rcs, msg = _calls(short, good, n, capi.MXD_F32_DIV255, None)
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and "dst_stride smaller than an output row (image 1)" in msg
    # the geometry checks of the plain calls
    out, _ = capi.make_images([_entry(crop_x=8)])
    rcs, msg = _calls(out, good, 1, capi.MXD_U8, None)
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and "Array: sub: shape out of bound" in msg


def test_jpeg_call_refusals():
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz"))
    coefs = capi.JpegCoefs(gold["caltech_300x200_jpg"])
    try:
        arr, n = capi.make_jpeg_images([dict(coefs=coefs, resize_w=150, resize_h=100, crop_x=0, crop_y=0, crop_w=150,
                                             crop_h=100, dst=4096, dst_stride=450)])
        L = capi.lib()
        assert L.mxd_jpeg_resize_crop_to_device_color(arr, None, n, capi.MXD_U8, None, 0) == capi.MXD_ERR_INVALID
        assert L.mxd_last_error() == b"mxd: null colors"
        m = R.IDENTITY.copy()
        m[1, 3] = float("nan")
        assert L.mxd_jpeg_resize_crop_to_device_color(arr, capi.make_colors([m]), n, capi.MXD_U8, None,
                                                      0) == capi.MXD_ERR_INVALID
        assert b"m[1][3]" in L.mxd_last_error() and b"(image 0)" in L.mxd_last_error()
    finally:
        coefs.close()


def test_apply_u8_refusals():
    L = capi.lib()
    px = np.zeros((4, 3), np.uint8)
    p = px.ctypes.data_as(ctypes.c_void_p)
    assert L.mxd_color_apply_u8(p, ctypes.c_int64(4), None, p) == capi.MXD_ERR_INVALID
    assert L.mxd_last_error() == b"mxd: null colors"
    m = R.IDENTITY.copy()
    m[0, 0] = float("inf")
    assert L.mxd_color_apply_u8(p, ctypes.c_int64(4), capi.make_colors([m]), p) == capi.MXD_ERR_INVALID
    assert b"m[0][0]" in L.mxd_last_error()
    assert L.mxd_color_apply_u8(None, ctypes.c_int64(4), capi.make_colors([R.IDENTITY]), p) == capi.MXD_ERR_INVALID


# ---- the layout of a colour call ---------------------------------------------------

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mlx-data_amd")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_color_layout_unit(tmp_path):
    """tests/cpp/color_layout_unit.cpp: a colour batch of mixed routes in the
    device-free environment -- every image in scratch at a 256-byte aligned
    offset, one entry per image with the matrix of its image, fmt_blocks."""
    exe = str(tmp_path / "color_layout_unit")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-I", os.path.join(os.path.dirname(HERE), "include"), "-I",
                    os.path.join(PKG, "csrc"), os.path.join(HERE, "cpp", "color_layout_unit.cpp"), "-L", PKG,
                    "-lmxd_amd", "-Wl,-rpath," + PKG, "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


# ---- operator surface: arguments, the marked plan, random draws ----------------------

def _rgb(h=40, w=60, seed=0, c=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def _buf(n=1, **kw):
    from mlx_data_amd import data as dx

    return dx.buffer_from_vector([dict(image=_rgb(seed=k, **kw)) for k in range(n)])


def _plan(b, i=0, key="image"):
    from mlx_data_amd import _pipeline

    return _pipeline._plan(b, i, key)


@pytest.mark.parametrize("make,word", [
    (lambda b: b.image_color_twist("image", brightness=-0.5), "image_color_twist: brightness"),
    (lambda b: b.image_color_twist("image", contrast=float("nan")), "image_color_twist: contrast"),
    (lambda b: b.image_color_twist("image", saturation=float("inf")), "image_color_twist: saturation"),
    (lambda b: b.image_color_twist("image", hue=float("nan")), "image_color_twist: hue"),
    (lambda b: b.image_color_matrix("image", np.eye(2)), "image_color_matrix: matrix must be 3x3 or 3x4"),
    (lambda b: b.image_color_matrix("image", np.zeros((3, 5))), "image_color_matrix: matrix must be 3x3 or 3x4"),
    (lambda b: b.image_color_matrix("image", [[1, 0, 0], [0, 1, 0], [0, 0]]), "image_color_matrix: matrix must be"),
    (lambda b: b.image_color_matrix("image", "abc"), "image_color_matrix: matrix must be"),
    (lambda b: b.image_color_matrix("image", np.full((3, 4), np.nan)), "image_color_matrix: entries must be finite"),
    (lambda b: b.image_color_matrix("image", np.eye(3) * 1e7), "image_color_matrix: entries must be finite and at most"),
    (lambda b: b.image_random_color_twist("image", brightness=(1.2, 0.8)), "brightness range has lo > hi"),
    (lambda b: b.image_random_color_twist("image", contrast=(-0.1, 0.8)), "contrast must be >= 0"),
    (lambda b: b.image_random_color_twist("image", saturation=(0.0, float("inf"))), "saturation range must be finite"),
    (lambda b: b.image_random_color_twist("image", hue=(float("nan"), 1.0)), "hue range must be finite"),
    (lambda b: b.image_random_color_twist("image", hue=3.0), "hue must be None or a (lo, hi) pair"),
])
def test_surface_refuses_bad_arguments_when_the_op_is_made(make, word):
    with pytest.raises(ValueError) as err:
        make(_buf())
    assert word in str(err.value), str(err.value)


def test_surface_refuses_non_rgb_images_when_the_op_is_applied():
    for c in (1, 2, 4):
        for make in (lambda b: b.image_color_twist("image", 1.2), lambda b: b.image_color_matrix("image", np.eye(3)),
                     lambda b: b.image_random_color_twist("image", hue=(-10, 10))):
            b = make(_buf(c=c))  # made without complaint
            with pytest.raises(RuntimeError) as err:
                b[0]
            assert str(err.value).startswith("image_color_twist: image must have 3 channels"), str(err.value)


def test_the_op_marks_the_plan_and_geometry_composes():
    b = _buf().image_resize("image", 30, 20)
    assert _plan(b)["color"] is None
    t = b.image_color_twist("image", 1.2, 0.5)
    p = _plan(t)
    assert np.array_equal(np.float32(p["color"]), capi.color_twist_matrix(1.2, 0.5))
    q = _plan(b)
    assert {k: p[k] for k in p if k != "color"} == {k: q[k] for k in q if k != "color"}  # geometry untouched
    # crop, flips and random crop still compose on the coloured plan
    after = t.image_center_crop("image", 10, 10).image_random_h_flip("image", 1.0).image_random_crop("image", 4, 4)
    plain = b.image_center_crop("image", 10, 10).image_random_h_flip("image", 1.0)
    pa = _plan(after)
    assert pa["color"] == p["color"] and pa["resize"] == (30, 20) and pa["flip"] and pa["crop"][2:] == (4, 4)
    assert _plan(plain)["crop"] == (10, 5, 10, 10) and pa["window"] == (0, 0, 60, 40)
    # image_to_float and image_normalize stack on top
    f = _plan(t.image_to_float("image"))
    assert f["color"] == p["color"] and f["shape"] == [20, 30, 3]
    n = _plan(t.image_normalize("image", mean=0.5, std=0.5, dtype="bfloat16", layout="chw"))
    assert n["color"] == p["color"] and n["format"]["dtype"] == "bfloat16" and n["shape"] == [3, 20, 30]
    # the matrix op: 3x3 and 3x4, offsets scaled by 255 in float32; output_key and _if
    m = np.array([[0.5, 0.1, 0, 0.25], [0, 1, 0, -0.1], [0.2, 0, 0.7, 0.0]])
    want = m.astype(np.float32)
    want[:, 3] = want[:, 3] * np.float32(255)
    assert np.array_equal(np.float32(_plan(b.image_color_matrix("image", m))["color"]), want)
    assert np.array_equal(np.float32(_plan(b.image_color_matrix("image", m[:, :3].tolist()))["color"])[:, :3], want[:, :3])
    assert np.array_equal(np.float32(_plan(b.image_color_matrix("image", m[:, :3]))["color"])[:, 3], np.zeros(3))
    o = b.image_color_twist("image", saturation=0.0, output_key="grey")
    assert _plan(o, 0, "grey")["color"] is not None and _plan(o, 0, "image")["color"] is None
    assert _plan(b.image_color_twist_if(False, "image", 2.0))["color"] is None
    assert _plan(b.image_color_matrix_if(True, "image", np.eye(3)))["color"] == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
    assert _plan(b.image_random_color_twist_if(True, "image", hue=(5, 5)))["color"] is not None
    assert _plan(b.image_color_twist("image"))["color"] == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]  # the defaults
    # on a stream too
    s = _buf().to_stream().image_color_twist("image", 1.5).image_to_float_if(False, "image")
    assert s is not None


def test_random_twist_draws():
    from mlx_data_amd import data as dx

    kw = dict(brightness=(0.6, 1.4), contrast=(0.5, 1.5), saturation=(0.0, 2.0), hue=(-30.0, 30.0))
    b = _buf(6).image_random_color_twist("image", **kw)

    def draw(seed):
        dx.set_state(seed)
        return [np.float32(_plan(b, i)["color"]) for i in range(6)]

    a, again, other = draw(7), draw(7), draw(8)
    assert all(np.array_equal(x, y) for x, y in zip(a, again))
    assert not any(np.array_equal(x, y) for x, y in zip(a, other))
    assert len({x.tobytes() for x in a}) == 6
    # a brightness-only range: b * I with b in range, nothing else drawn
    dx.set_state(3)
    for i in range(6):
        m = np.float32(_plan(_buf(6).image_random_color_twist("image", brightness=(0.8, 1.25)), i)["color"])
        bb = m[0, 0]
        assert 0.8 <= bb <= 1.25 and np.array_equal(m, (np.float64(bb) * np.eye(3, 4)).astype(np.float32))
    # the draws are std::uniform_real_distribution<double>'s over mt19937, in the order b, c, s, h:
    # libstdc++'s generate_canonical<double, 53> takes two 32-bit outputs per draw, low word first
    dx.set_state(11)
    got = np.float32(_plan(b, 0)["color"])
    words = np.random.RandomState(11)  # the same mt19937 seeding as std::mt19937(seed)
    raw = [int(words.randint(0, 2 ** 32, dtype=np.uint64)) for _ in range(8)]
    u = [(raw[2 * k] + raw[2 * k + 1] * 2.0 ** 32) / 2.0 ** 64 for k in range(4)]
    f = [lo + (hi - lo) * x for (lo, hi), x in zip(kw.values(), u)]
    assert np.abs(R.to_bytes_units(R.twist_ref(*f)) - got).max() < 1e-3
    # a None draws nothing: a following image_random_crop sees the generator state it would see without the op
    base = _buf(6).image_random_crop("image", 7, 5)
    none = _buf(6).image_random_color_twist("image").image_random_crop("image", 7, 5)
    hue = _buf(6).image_random_color_twist("image", hue=(-5, 5)).image_random_crop("image", 7, 5)
    dx.set_state(21)
    want = [_plan(base, i)["crop"] for i in range(6)]
    dx.set_state(21)
    assert [_plan(none, i)["crop"] for i in range(6)] == want
    dx.set_state(21)
    assert [_plan(hue, i)["crop"] for i in range(6)] != want
    assert _plan(none, 0)["color"] == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
