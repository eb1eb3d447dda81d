"""Pillow's 8-bit resize filters (pil_bilinear, pil_bicubic, pil_lanczos) on the
CPU: mxd_pil_resize_u8 against Pillow itself, byte for byte, the tap tables'
8.22 form, the operator surface's names and the refusal of alpha images.
(On the inputs of pil_resize_cases.image a restatement without the clamp
between the two passes differs from Pillow at 16x20 -> 45x33 in 542 bytes for
pil_bicubic and 1051 for pil_lanczos, and at 105x207 -> 69x35 in 8 and 67: the
tests see that clamp.)"""
import ctypes
import os

import numpy as np
import pytest

import pil_resize_cases as P
from mlx_data_amd import capi


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("geom,filter", P.CASES, ids=P.IDS)
def test_cpu_statement_is_pillow(geom, filter, channels):
    a = P.image(geom[0], geom[1], channels)
    got = capi.pil_resize_u8(a, filter, geom[2], geom[3], geom[4], geom[5])
    assert np.array_equal(got, P.pillow(a, geom, filter))


@pytest.mark.parametrize("filter", P.FILTERS)
@pytest.mark.parametrize("in_size,out_size", [(90, 24), (20, 45), (64, 64), (320, 20)])
def test_taps_are_8_22_fixed_point(filter, in_size, out_size):
    first, cnt, w = capi.axis_taps(in_size, out_size, filter=filter)
    k = w.astype(np.float64) * 2.0 ** 22
    assert np.array_equal(k, np.round(k)) and np.all(first >= 0) and np.all(first + cnt <= in_size)
    assert np.all(np.abs(w.astype(np.float64).sum(axis=1) - 1.0) <= cnt * 2.0 ** -23)
    if in_size == out_size:  # Pillow skips the pass: the coefficients leave every byte as it is
        assert np.all(k.sum(axis=1) == 2 ** 22) and np.all(np.count_nonzero(k, axis=1) == 1)


@pytest.mark.parametrize("filter", P.FILTERS)
def test_surface_carries_the_names(filter):
    import sys

    from mlx_data_amd import _pipeline
    from mlx_data_amd import data as dx

    b = dx.buffer_from_vector([dict(image=P.image(40, 60, 3))])
    for ds in (b.image_resize("image", 30, 20, filter=filter), b.image_resize_smallest_side("image", 20, filter=filter),
               b.image_resize_if(True, "image", 30, 20, filter=filter),
               b.image_resize_smallest_side_if(True, "image", 20, filter=filter)):
        p = _pipeline._plan(ds, 0, "image")
        assert p["filter"] == filter and p["resize"] == (30, 20)
    b.to_stream().image_resize("image", 30, 20, filter=filter).image_resize_smallest_side_if(False, "image", 9)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))), "compat"))
    import mlx.data as mdx

    m = mdx.buffer_from_vector([dict(image=P.image(40, 60, 3))]).image_resize("image", 30, 20, filter=filter)
    assert _pipeline._plan(m, 0, "image")["filter"] == filter
    assert capi.describe_plan(dict(src_stride=180, src_w=60, src_h=40, channels=3, resize_w=30, resize_h=20, crop_x=0,
                                   crop_y=0, crop_w=30, crop_h=20, dst_stride=90, filter=capi.FILTERS[filter]))["wave"] == 2


@pytest.mark.parametrize("channels", [2, 4])
def test_alpha_images_are_refused(channels):
    e = dict(src_stride=60 * channels, src_w=60, src_h=40, channels=channels, resize_w=30, resize_h=20, crop_x=0,
             crop_y=0, crop_w=30, crop_h=20, dst_stride=30 * channels, filter=capi.FILTERS["pil_bicubic"])
    with pytest.raises(capi.MxdError) as err:
        capi.describe_plan(e)
    assert err.value.code == capi.MXD_ERR_UNSUPPORTED and "premultiplies" in str(err.value)
    arr, n = capi.make_images([dict(e, src=4096, dst=4096)])
    assert capi.lib().mxd_resize_crop_batch(arr, n, capi.MXD_U8, 0, None) == capi.MXD_ERR_UNSUPPORTED
    src, dst = np.zeros((40, 60, channels), np.uint8), np.zeros((20, 30, channels), np.uint8)
    assert capi.lib().mxd_pil_resize_u8(src.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(60 * channels), 60, 40,
                                        channels, 17, 30, 20, 0, 0, 30, 20, 0, dst.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.c_int64(30 * channels)) == capi.MXD_ERR_UNSUPPORTED
