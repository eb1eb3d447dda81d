"""The resize filters (triangle, Catmull-Rom, Mitchell, cubic B-spline) on the
CPU: the product tap tables against the float64 restatement, the Catmull-Rom
restatement against torch bicubic and Pillow BICUBIC on replicate-padded
sources, the operator surface's ``filter=`` argument, the C ABI's filter field
and mxd_axis_taps_filter, and the host planner's routes for cubic images.
References: tests/filter_ref.py (nothing here comes from the code under test).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import filter_ref as R
from mlx_data_amd import capi
from test_border_evidence import GEOMS

AXES = sorted({(g[0], g[2]) for g in GEOMS} | {(g[1], g[3]) for g in GEOMS})

# (src w, src h, dst w, dst h) of the torch / Pillow cross-checks
BICUBIC_GEOMS = [
    (300, 200, 384, 256), (1280, 960, 341, 256), (500, 375, 341, 256), (375, 500, 256, 341),
    (640, 480, 341, 256), (731, 512, 224, 224), (97, 203, 224, 224), (7, 3, 5, 9), (1, 5, 3, 2),
    (256, 300, 256, 200), (129, 65, 64, 130),
]


def rand(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def whole(dw, dh):
    return (dw, dh, 0, 0, dw, dh, 0)


# ---- product tables -----------------------------------------------------------
@pytest.mark.parametrize("filter", R.FILTERS)
@pytest.mark.parametrize("n_in,n_out", AXES)
def test_product_tables(n_in, n_out, filter):
    """Weights sum to 1 in float32, indices stay in range, and the dense matrix
    is the float64 restatement's up to the float32 scale and weight arithmetic."""
    first, cnt, w = capi.axis_taps(n_in, n_out, filter=filter)
    assert np.abs(w.astype(np.float64).sum(axis=1) - 1).max() < 1e-5
    assert first.min() >= 0 and (first + cnt).max() <= n_in and cnt.min() >= 1
    dense = np.zeros((n_out, n_in))
    for j in range(n_out):
        dense[j, first[j]:first[j] + cnt[j]] = w[j, :cnt[j]]
    assert np.abs(dense - R.axis_matrix(n_in, n_out, filter)).max() < 5e-5


@pytest.mark.parametrize("filter", R.CUBICS)
def test_cubic_tables_have_the_support_of_two(filter):
    """About twice the triangle's taps: 4 upsampling, 15 at 960 -> 256, 6 at
    375 -> 256, 34 at 2160 -> 256; Catmull-Rom keeps its interior zeros."""
    for n_in, n_out, taps in [(200, 256, 4), (960, 256, 15), (375, 256, 6), (2160, 256, 34)]:
        assert capi.axis_taps(n_in, n_out, filter=filter)[2].shape[1] == taps
    first, cnt, w = capi.axis_taps(768, 256, filter="catmullrom")  # 3:1: the taps at s * distance = +-1 are zero
    mid = w[128, :cnt[128]]
    assert (mid[1:-1] == 0).sum() == 2 and mid[0] != 0 and mid[-1] != 0


@pytest.mark.parametrize("filter", R.FILTERS)
def test_identity_axis_is_the_identity(filter):
    first, cnt, w = capi.axis_taps(37, 37, filter=filter)
    assert (cnt == 1).all() and (first == np.arange(37)).all() and (w[:, 0] == 1).all()
    img = rand(9, 37, 3, 5)
    assert np.array_equal(R.vfirst(img, (37, 9, 3, 2, 30, 6, 1), filter), img[2:8, 3:33][:, ::-1])
    assert np.array_equal(R.resize(img, 37, 9, filter), img)


@pytest.mark.parametrize("filter", R.FILTERS)
@pytest.mark.parametrize("w,h,dw,dh", GEOMS)
def test_constants_stay_exact(w, h, dw, dh, filter):
    for value in (0, 1, 128, 254, 255):
        img = np.full((h, w, 3), value, np.uint8)
        assert (R.vfirst(img, whole(dw, dh), filter) == value).all()


@pytest.mark.parametrize("filter", R.FILTERS)
@pytest.mark.parametrize("w,h,dw,dh", BICUBIC_GEOMS)
def test_kernel_order_against_float64(w, h, dw, dh, filter):
    """The float32 vertical-first sums of the product tables against the
    float64 restatement, whole frames, borders included."""
    img = rand(h, w, 3, w * 11 + h)
    R.gate(R.resize(img, dw, dh, filter), R.vfirst(img, whole(dw, dh), filter))


def test_triangle_restatement_is_the_oracles():
    """filter 0 through the new references is what the existing oracle gives."""
    import oracle as O

    img = rand(375, 500, 3, 1)
    g = (341, 256, 58, 16, 224, 224, 1)
    assert np.array_equal(R.vfirst(img, g, "triangle"), O.resize_crop_vfirst(img, g))


# ---- Catmull-Rom is bicubic -----------------------------------------------------
@pytest.mark.parametrize("w,h,dw,dh", BICUBIC_GEOMS)
def test_catmullrom_is_torch_bicubic(w, h, dw, dh):
    img = rand(h, w, 3, w * 5 + h)
    R.gate(R.resize(img, dw, dh, "catmullrom"), R.torch_clamp(img, dw, dh))


@pytest.mark.parametrize("w,h,dw,dh", BICUBIC_GEOMS)
def test_catmullrom_is_pillow_bicubic(w, h, dw, dh):
    img = rand(h, w, 3, w * 3 + h)
    R.gate(R.resize(img, dw, dh, "catmullrom"), R.pillow_clamp(img, dw, dh))


def test_overshoot_clamps():
    """A 0 / 255 checkerboard of 3-pixel cells under Catmull-Rom overshoots on
    both sides; the encode clamps (never wraps)."""
    yy, xx = np.mgrid[0:48, 0:64]
    img = np.repeat(((((yy // 3) + (xx // 3)) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    v = R.resize_float(img, 96, 72, "catmullrom")
    assert v.min() < -1 and v.max() > 256
    out = R.vfirst(img, whole(96, 72), "catmullrom")
    assert (out[v < -0.01] == 0).all() and (out[v > 255.01] == 255).all()
    assert np.abs(out.astype(np.float64) - np.clip(v, 0, 255)).max() < 0.51  # rounds, never wraps


# ---- C ABI ----------------------------------------------------------------------
def test_abi_filter_symbols_and_version():
    assert capi.lib().mxd_abi_version() == 7
    assert hasattr(capi.lib(), "mxd_axis_taps_filter")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "mxd_amd.h")).read()
    assert "#define MXD_HAS_FILTERS 1" in header and "#define MXD_ABI_VERSION 7" in header
    assert capi.MxdImage.filter.offset == capi.MxdImage.rgba_weighted.offset + 4
    assert ctypes.sizeof(capi.MxdImage) == 80


@pytest.mark.parametrize("n_in,n_out", [(960, 256), (200, 256), (7, 5), (64, 64)])
def test_axis_taps_filter_zero_is_axis_taps(n_in, n_out):
    L = capi.lib()
    i32, f32 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    res = []
    for filtered in (False, True):
        first, cnt, w = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((n_out, 12), np.float32)
        need = ctypes.c_int32()
        args = (first.ctypes.data_as(i32), cnt.ctypes.data_as(i32), w.ctypes.data_as(f32), ctypes.byref(need))
        rc = (L.mxd_axis_taps_filter(n_in, n_out, 0, n_out, 0, 12, *args) if filtered
              else L.mxd_axis_taps(n_in, n_out, 0, n_out, 12, *args))
        assert rc == capi.MXD_OK
        res.append((first, cnt, w.view(np.uint32), need.value))
    for a, b in zip(*res):
        assert np.array_equal(a, b)


def test_unknown_filter_is_invalid():
    need = ctypes.c_int32()
    L = capi.lib()
    for bad in (99, -1, 4):
        assert L.mxd_axis_taps_filter(10, 5, 0, 5, bad, 0, None, None, None, ctypes.byref(need)) == capi.MXD_ERR_INVALID
        assert b"filter" in L.mxd_last_error()
        e = dict(src_stride=64 * 3, src_w=64, src_h=64, channels=3, resize_w=32, resize_h=32, crop_x=0, crop_y=0,
                 crop_w=32, crop_h=32, dst_stride=96, filter=bad)
        with pytest.raises(capi.MxdError) as err:
            capi.describe_plan(e)
        assert err.value.code == capi.MXD_ERR_INVALID and "filter" in str(err.value)
        arr, n = capi.make_images([dict(e, src=4096, dst=4096)])
        assert L.mxd_resize_crop_batch(arr, n, capi.MXD_U8, 0, None) == capi.MXD_ERR_INVALID
        assert L.mxd_resize_crop_host(arr, n, capi.MXD_U8, 0) == capi.MXD_ERR_INVALID


# ---- planner (Python side; the C++ walk is test_filter_planner_unit) -----------
def _entry(w, h, rw, rh, cx, cy, cw=224, ch=224, filter=0, c=3):
    return dict(src_stride=(w * c + 15) // 16 * 16, src_w=w, src_h=h, channels=c, resize_w=rw, resize_h=rh,
                crop_x=cx, crop_y=cy, crop_w=cw, crop_h=ch, dst_stride=cw * c, filter=filter)


@pytest.mark.parametrize("filter", [1, 2, 3])
def test_cubic_plans(filter):
    c2 = capi.describe_plan(_entry(1280, 960, 341, 256, 58, 16, filter=filter))
    assert (c2["wave"], c2["kind"], c2["s"], c2["dmax"], c2["taps"]) == (1, 2, 4, 4, 17)
    c4 = capi.describe_plan(_entry(500, 375, 341, 256, 58, 16, filter=filter))
    assert (c4["wave"], c4["kind"], c4["s"], c4["dmax"], c4["taps"]) == (1, 2, 4, 2, 6)
    up = capi.describe_plan(_entry(300, 200, 384, 256, 80, 16, filter=filter))
    assert (up["wave"], up["kind"], up["taps"]) == (1, 0, 4)  # 4-tap gather
    far = capi.describe_plan(_entry(3840, 2160, 455, 256, 115, 16, filter=filter))
    assert far["wave"] == 0  # 34 taps: past the largest bucket
    rgba = capi.describe_plan(_entry(500, 375, 341, 256, 58, 16, filter=filter, c=4))
    assert rgba["wave"] == 0


def test_triangle_plans_are_unchanged():
    """Filter 0, named or left at its zero default, plans what tests/test_capi.py
    pins for the same geometries (values from that file, which predates the
    filters)."""
    for kw in ({}, {"filter": 0}):
        e = dict(_entry(1280, 960, 341, 256, 58, 16), src_stride=1280 * 3, dst_stride=224 * 12, **kw)
        p = capi.describe_plan(e, capi.MXD_F32_DIV255)
        assert (p["wave"], p["kind"], p["taps"], p["s"], p["dmax"], p["p"], p["nstrips"], p["q"]) == (1, 2, 8, 2, 4, 8, 2, 2)
        c4 = capi.describe_plan(dict(e, src_w=500, src_h=375, src_stride=1500), capi.MXD_F32_DIV255)
        assert (c4["p"], c4["nstrips"], c4["q"], c4["s"], c4["taps"]) == (4, 2, 2, 2, 3)
        # a triangle window whose scatter shape has four slots keeps its gather kernel
        up = capi.describe_plan(dict(_entry(417, 167, 639, 256, 305, 91, 28, 73), **kw))
        assert (up["wave"], up["kind"], up["taps"]) == (1, 0, 2)
        big = capi.describe_plan(dict(e, src_w=4032, src_h=3024, src_stride=4032 * 3), capi.MXD_F32_DIV255)
        assert (big["taps"], big["dmax"], big["p"], big["nstrips"]) == (24, 12, 8, 6)


HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mlx-data_amd")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_filter_planner_unit(tmp_path):
    """tests/cpp/filter_planner_unit.cpp: build_layout in the device-free
    environment for cubic batches, and filter-0 plans as planner_unit.cpp sees them."""
    exe = str(tmp_path / "filter_planner_unit")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-I", os.path.join(os.path.dirname(HERE), "include"), "-I",
                    os.path.join(PKG, "csrc"), os.path.join(HERE, "cpp", "filter_planner_unit.cpp"), "-L", PKG,
                    "-lmxd_amd", "-Wl,-rpath," + PKG, "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


# ---- operator surface -------------------------------------------------------------
def _buffer(img=None):
    from mlx_data_amd import data as dx

    return dx.buffer_from_vector([dict(image=rand(40, 60, 3, 0) if img is None else img)])


@pytest.mark.parametrize("filter", R.FILTERS)
def test_surface_carries_the_filter(filter):
    from mlx_data_amd import _pipeline

    b = _buffer()
    for ds, key in ((b.image_resize("image", 30, 20, filter=filter), "image"),
                    (b.image_resize_smallest_side("image", 20, filter=filter), "image"),
                    (b.image_resize_if(True, "image", 30, 20, filter=filter), "image"),
                    (b.image_resize_smallest_side_if(True, "image", 20, filter=filter), "image"),
                    (b.image_resize("image", 30, 20, "out", filter=filter), "out")):
        p = _pipeline._plan(ds, 0, key)
        assert p["filter"] == filter and p["resize"] == (30, 20)
    # Stream carries the same ops
    b.to_stream().image_resize("image", 30, 20, filter=filter).image_resize_smallest_side_if(False, "image", 9)
    # a crop after the resize keeps it; an if-form with a false condition leaves the sample alone
    p = _pipeline._plan(b.image_resize("image", 30, 20, filter=filter).image_center_crop("image", 8, 8), 0, "image")
    assert p["filter"] == filter and p["crop"] == (11, 6, 8, 8)
    assert _pipeline._plan(b.image_resize_if(False, "image", 30, 20, filter=filter), 0, "image") is None
    # a second resize materialises the first (a GPU launch), so only its plan is looked at here:
    # a resize of a crop-only plan takes the crop as its source window and the new filter
    p = _pipeline._plan(b.image_center_crop("image", 32, 32).image_resize("image", 16, 16, filter=filter), 0, "image")
    assert p["filter"] == filter and p["window"] == (14, 4, 32, 32)


def test_surface_default_and_errors():
    from mlx_data_amd import _pipeline

    b = _buffer()
    base = _pipeline._plan(b.image_resize("image", 30, 20), 0, "image")
    assert base["filter"] == "triangle"
    assert _pipeline._plan(b.image_resize("image", 30, 20, filter="triangle"), 0, "image") == base
    assert _pipeline._plan(b.image_center_crop("image", 8, 8), 0, "image")["filter"] == "triangle"
    for op, args in (("image_resize", ("image", 30, 20)), ("image_resize_smallest_side", ("image", 20))):
        with pytest.raises(ValueError, match="triangle, catmullrom, mitchell, cubicbspline"):
            getattr(b, op)(*args, filter="lanczos")  # raised when the op is made, before any sample is read
        with pytest.raises(ValueError, match="triangle, catmullrom, mitchell, cubicbspline"):
            getattr(b.to_stream(), op)(*args, filter="bicubic")
        with pytest.raises(TypeError):
            getattr(b, op)(*args, "", "catmullrom")  # keyword only


def test_mlx_data_exposes_the_filter():
    import sys

    compat = os.path.join(PKG, "compat")
    if compat not in sys.path:
        sys.path.insert(0, compat)
    import mlx.data as dx
    from mlx_data_amd import _pipeline

    b = dx.buffer_from_vector([dict(image=rand(40, 60, 3, 0))]).image_resize_smallest_side("image", 20, filter="mitchell")
    assert _pipeline._plan(b, 0, "image")["filter"] == "mitchell"
