"""CPU: formatted outputs (mxd_out_format, include/mxd_amd.h) without a device.

The element a result byte q of channel c becomes is defined by three float32
operations, each correctly rounded -- x = q / 255, y = (x - mean[c]) / std[c],
out = y converted to float32 / float16 / bfloat16 (round to nearest even) --
i.e. NumPy's ((u8.astype("float32") / 255) - mean) / std, then
.astype("float16") or torch's .to(torch.bfloat16).  mxd_out_format_table is the
one place the library computes those values (the kernels look them up), so
pinning it to the NumPy / torch expression bit for bit pins every output; the
GPU tests (tests/test_gpu_out_format.py) then compare the kernels' outputs with
tables built by the same expression.  Also: every validation rule of the _fmt
entry points, which all refuse before any device work."""
import ctypes
import os

import numpy as np
import pytest

from mlx_data_amd import capi
from out_format_util import ELEMS, IMAGENET_MEAN, IMAGENET_STD, expected_table

HERE = os.path.dirname(os.path.abspath(__file__))
LUT = np.load(os.path.join(HERE, "golden", "golden.npz"))["lut"]

# A mean equal to q / 255 exactly (zero results), and one within a float16
# denormal of 1.0 (q = 255 gives |y| < 2^-14: a denormal float16).
MEAN_EXACT = float(np.float32(77) / np.float32(255))
MEAN_DENORMAL = float(np.float32(1.0) - np.float32(2.0 ** -16))
NORMS = {
    "none": (None, None),
    "imagenet": (IMAGENET_MEAN + (0.5,), IMAGENET_STD + (0.25,)),
    "scalar": (0.5, 0.25),
    "zero_result": (MEAN_EXACT, 0.3),
    "f16_denormal": (MEAN_DENORMAL, 1.0),
    "negative_std_tiny": ((0.1, 0.9, 0.3, 0.7), (-0.5, 1e-3, 3.0, 1e-6)),
}


@pytest.mark.parametrize("norm", sorted(NORMS))
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("elem", sorted(ELEMS))
def test_table_is_bit_equal_to_the_numpy_expression(elem, channels, norm):
    mean, std = NORMS[norm]
    cut = (lambda v: v[:channels] if isinstance(v, tuple) else v)
    fmt = capi.make_out_format(ELEMS[elem], capi.MXD_LAYOUT_HWC, cut(mean), cut(std))
    got = capi.out_format_table(fmt, channels)
    want = expected_table(elem, channels, cut(mean), cut(std))
    assert got.dtype == want.dtype and got.shape == want.shape == (channels, 256)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_unnormalised_float32_is_the_div255_lut():
    fmt = capi.make_out_format(capi.MXD_ELEM_F32)
    assert fmt.normalize == 0
    got = capi.out_format_table(fmt, 3)
    for c in range(3):
        assert np.array_equal(got[c], np.asarray(LUT, np.float32).view(np.uint32))


def test_the_special_means_give_zero_and_denormal_results():
    z = capi.out_format_table(capi.make_out_format(capi.MXD_ELEM_F32, mean=MEAN_EXACT, std=0.3), 1)
    assert z[0, 77] == 0
    d = capi.out_format_table(capi.make_out_format(capi.MXD_ELEM_F16, mean=MEAN_DENORMAL, std=1.0), 1)
    v = d[0].view(np.float16)
    assert v[255] != 0 and abs(float(v[255])) < 2.0 ** -14  # a denormal float16, not flushed
    assert d[0, 255] == expected_table("float16", 1, MEAN_DENORMAL, 1.0)[0, 255]


# ---- validation: MXD_ERR_INVALID before any device work ---------------------

def _images(n=1, **kw):
    e = dict(src=4096, src_stride=3 * 100, src_w=100, src_h=80, channels=3, resize_w=100, resize_h=80, crop_x=0,
             crop_y=0, crop_w=50, crop_h=40, flip=0, dst=4096, dst_stride=50 * 3 * 4)
    e.update(kw)
    return capi.make_images([dict(e) for _ in range(n)])


def _fmt(**kw):
    f = capi.make_out_format(kw.pop("elem", capi.MXD_ELEM_F32), kw.pop("layout", capi.MXD_LAYOUT_HWC),
                             kw.pop("mean", None), kw.pop("std", None), kw.pop("plane_stride", 0))
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _chw(**kw):
    return _fmt(layout=capi.MXD_LAYOUT_CHW, **kw)


BAD = [
    ("elem", _fmt(elem=3), {}, "elem"),
    ("layout", _fmt(layout=2), {}, "layout"),
    ("std zero", _fmt(mean=0.5, std=(0.2, 0.0, 0.2)), {}, r"std\[1\]"),
    ("std inf", _fmt(mean=0.5, std=(0.2, 0.2, float("inf"))), {}, r"std\[2\]"),
    ("std nan", _fmt(mean=0.5, std=(float("nan"), 0.2, 0.2)), {}, r"std\[0\]"),
    ("mean nan", _fmt(mean=(0.5, float("nan"), 0.5), std=0.2), {}, r"mean\[1\]"),
    ("dst odd f32", _fmt(), dict(dst=4098), "dst is not a multiple"),
    ("dst odd f16", _fmt(elem=capi.MXD_ELEM_F16), dict(dst=4097, dst_stride=300), "dst is not a multiple"),
    ("stride odd", _fmt(elem=capi.MXD_ELEM_BF16), dict(dst_stride=301), "dst_stride is not a multiple"),
    ("stride short", _fmt(elem=capi.MXD_ELEM_F16), dict(dst_stride=298), "dst_stride smaller"),
    ("plane short", _chw(plane_stride=40 * 200 - 4), dict(dst_stride=200), "plane_stride smaller"),
    ("plane odd", _chw(elem=capi.MXD_ELEM_F16, plane_stride=40 * 100 + 1), dict(dst_stride=100), "plane_stride is not"),
]


@pytest.mark.parametrize("name,fmt,kw,msg", BAD, ids=[b[0] for b in BAD])
def test_fmt_calls_refuse_bad_arguments(name, fmt, kw, msg):
    arr, n = _images(**kw)
    for call in (capi.resize_crop_batch_fmt, capi.resize_crop_to_device_fmt):
        with pytest.raises(capi.MxdError, match=msg) as e:
            call(arr, n, fmt)
        assert e.value.code == capi.MXD_ERR_INVALID, (name, call.__name__)


def test_a_fourth_channels_std_is_not_read_for_rgb():
    """Only mean / std of the image's channels are checked: std[3] = 0 is fine
    for RGB and refused for RGBA."""
    f = _fmt(mean=0.5, std=(0.2, 0.2, 0.2, 0.0))
    assert capi.out_format_table(f, 3).shape == (3, 256)
    with pytest.raises(capi.MxdError, match=r"std\[3\]"):
        capi.out_format_table(f, 4)


def test_null_fmt_and_table_arguments():
    arr, n = _images()
    for call in (capi.resize_crop_batch_fmt, capi.resize_crop_to_device_fmt, capi.jpeg_resize_crop_to_device_fmt):
        with pytest.raises(capi.MxdError, match="null fmt") as e:
            call(arr, n, None)
        assert e.value.code == capi.MXD_ERR_INVALID
    L = capi.lib()
    f = _fmt()
    assert L.mxd_out_format_table(None, 3, None) == capi.MXD_ERR_INVALID
    assert L.mxd_out_format_table(ctypes.byref(f), 3, None) == capi.MXD_ERR_INVALID
    buf = (ctypes.c_uint32 * 2048)()
    assert L.mxd_out_format_table(ctypes.byref(f), 0, buf) == capi.MXD_ERR_INVALID
    assert L.mxd_out_format_table(ctypes.byref(f), 5, buf) == capi.MXD_ERR_INVALID


def test_chw_refuses_mixed_channel_counts():
    arr, n = capi.make_images([
        dict(src=4096, src_stride=300, src_w=100, src_h=80, channels=c, resize_w=100, resize_h=80, crop_x=0, crop_y=0,
             crop_w=50, crop_h=40, flip=0, dst=4096, dst_stride=200) for c in (3, 1)])
    fmt = _chw(plane_stride=40 * 200)
    for call in (capi.resize_crop_batch_fmt, capi.resize_crop_to_device_fmt):
        with pytest.raises(capi.MxdError, match="channels differ") as e:
            call(arr, n, fmt)
        assert e.value.code == capi.MXD_ERR_INVALID


def test_jpeg_fmt_call_validates_like_the_others():
    gold = np.load(os.path.join(HERE, "golden", "jpeg.npz"))
    co = capi.JpegCoefs(gold["sub2_prog0_jpg"])
    try:
        entry = dict(coefs=co, resize_w=co.width, resize_h=co.height, crop_x=0, crop_y=0, crop_w=16, crop_h=16,
                     flip=0, dst=4098, dst_stride=16 * 3 * 4)
        arr, n = capi.make_jpeg_images([entry])
        with pytest.raises(capi.MxdError, match="dst is not a multiple") as e:
            capi.jpeg_resize_crop_to_device_fmt(arr, n, _fmt())
        assert e.value.code == capi.MXD_ERR_INVALID
        with pytest.raises(capi.MxdError, match="elem") as e:
            capi.jpeg_resize_crop_to_device_fmt(arr, n, _fmt(elem=7))
        assert e.value.code == capi.MXD_ERR_INVALID
    finally:
        co.close()


def test_existing_dtype_calls_still_refuse_what_they_refused():
    arr, n = _images(dst_stride=100)
    with pytest.raises(capi.MxdError, match="dst_stride smaller than an output row"):
        capi.resize_crop_batch(arr, n, capi.MXD_U8)
    arr, n = _images()
    with pytest.raises(capi.MxdError, match="bad out_dtype"):
        capi.resize_crop_batch(arr, n, 2)


# ---- the operator surface, without a device ----------------------------------
# image_normalize only marks the pending image, so its argument checks, the plan
# it leaves and batch's format checks all run before any device work.

def _buffer(channels=3, h=20, w=30):
    from mlx_data_amd import data as dx

    return dx.buffer_from_vector([dict(image=np.zeros((h, w, channels), np.uint8))])


@pytest.mark.parametrize("kw,msg", [
    (dict(dtype="int8"), "dtype"),
    (dict(dtype="float64"), "dtype"),
    (dict(layout="nchw"), "layout"),
    (dict(std=(0.2, 0.0, 0.2)), "std"),
    (dict(std=0.0), "std"),
    (dict(std=float("inf")), "std"),
    (dict(mean=float("nan")), "mean"),
    (dict(mean=(0.1, 0.2, 0.3, 0.4, 0.5)), "at most 4"),
    (dict(mean="0.5"), "mean"),
], ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_image_normalize_refuses_bad_arguments_when_the_op_is_made(kw, msg):
    with pytest.raises(ValueError, match=msg):
        _buffer().image_normalize("image", **kw)


@pytest.mark.parametrize("kw,fits", [(dict(mean=(0.5, 0.5)), 2), (dict(std=(0.2, 0.2, 0.2, 0.2)), 4),
                                     (dict(mean=0.5, std=(0.2, 0.2)), 2)], ids=["mean2", "std4", "std2"])
def test_image_normalize_checks_lengths_against_the_image(kw, fits):
    from mlx_data_amd import _pipeline

    with pytest.raises(ValueError, match="values, the image 3 channels"):
        _buffer().image_normalize("image", **kw)[0]
    # the same values are fine for an image with that many channels
    assert _pipeline._plan(_buffer(fits).image_normalize("image", **kw), 0, "image")["format"]["normalize"]


def test_image_normalize_only_marks_the_pending_plan():
    from mlx_data_amd import _pipeline

    b = _buffer().image_resize("image", 16, 12).image_random_h_flip("image", 1.0)
    base = _pipeline._plan(b, 0, "image")
    assert base["format"] is None and base["shape"] == [12, 16, 3]
    n = b.image_normalize("image", mean=IMAGENET_MEAN, std=0.25, dtype="bfloat16", layout="chw")
    assert _pipeline._pending(n, 0, "image")
    p = _pipeline._plan(n, 0, "image")
    assert p["shape"] == [3, 12, 16]
    f = p.pop("format")
    assert (f["dtype"], f["layout"], f["normalize"]) == ("bfloat16", "chw", True)
    assert f["mean"][:3] == [float(np.float32(m)) for m in IMAGENET_MEAN] and f["std"] == [0.25] * 4
    base.pop("format"), base.pop("shape"), p.pop("shape")
    assert p == base  # the geometry is untouched
    q = _pipeline._plan(b.image_normalize("image"), 0, "image")  # defaults: q / 255 in float32 HWC
    assert q["shape"] == [12, 16, 3] and q["format"]["normalize"] is False
    assert (q["format"]["dtype"], q["format"]["layout"]) == ("float32", "hwc")
    # no image op after it, as after image_to_float
    for bad in (n, b.image_normalize("image", dtype="float16"), b.image_normalize("image")):
        with pytest.raises((ValueError, RuntimeError)):
            bad.image_center_crop("image", 4, 4)[0]
    # (F, H, W, C) videos take hwc only
    from mlx_data_amd import data as dx
    video = dx.buffer_from_vector([dict(image=np.zeros((2, 8, 8, 3), np.uint8))])
    with pytest.raises(RuntimeError, match="chw"):
        video.image_normalize("image", layout="chw")[0]


def test_if_variants_exist_and_mlx_data_exposes_the_op():
    import sys

    from mlx_data_amd import data as dx

    b = _buffer()
    assert b.image_normalize_if(False, "image", mean=0.5) is b
    assert b.image_normalize_if(True, "image", mean=0.5) is not b
    s = b.to_stream()
    assert s.image_normalize_if(False, "image") is s and s.image_normalize_if(True, "image", std=2.0) is not s
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "mlx-data_amd", "compat"))
    import mlx.data

    for cls in (mlx.data.Buffer, mlx.data.Stream):
        assert callable(cls.image_normalize) and callable(cls.image_normalize_if)
    assert mlx.data.Buffer is dx.Buffer


def test_batch_refuses_unequal_formats_and_channel_counts_before_any_launch():
    from mlx_data_amd import _pipeline

    def norm(b, **kw):
        return b.image_resize("image", 16, 12).image_normalize("image", **kw)

    a = norm(_buffer(), mean=0.5, std=0.25, dtype="float16", layout="chw")
    with pytest.raises(RuntimeError, match="different output formats"):
        _pipeline._merge([a, norm(_buffer(), mean=0.4, std=0.25, dtype="float16", layout="chw")])
    with pytest.raises(RuntimeError, match="different types"):
        _pipeline._merge([a, norm(_buffer(), mean=0.5, std=0.25, dtype="bfloat16", layout="chw")])
    with pytest.raises(RuntimeError, match="different channel counts"):
        _pipeline._merge([a, norm(_buffer(1), mean=0.5, std=0.25, dtype="float16", layout="chw")])
    with pytest.raises(RuntimeError, match="different channel counts"):
        _pipeline._merge([norm(_buffer(), mean=0.5), norm(_buffer(4), mean=0.5)])
    # same dtype and shape, one not normalised: image_to_float's q / 255 against a mean / std
    with pytest.raises(RuntimeError, match="different output formats"):
        _pipeline._merge([norm(_buffer(), mean=0.5), _buffer().image_resize("image", 16, 12).image_to_float("image")])
