"""TEST INFRASTRUCTURE ONLY -- references for the resize filters.

Three statements of the filtered resize that share no code with the product
tap builder (mlx-data_amd/csrc/taps.cpp):

1. A float64 dense-matrix restatement of the filter arithmetic, written like
   oracle/stbir_f64.py with the kernel and its support as parameters:
   stb_image_resize2's cubic kernels (all of support 2, x = |distance|),
   upsampling over the source pixels within `support` of (j + 0.5) / s,
   downsampling with the kernel evaluated at s * distance, weighted by s, over
   support / s source pixels; out-of-range taps folded onto the edge pixel by
   index clamping; every row renormalised to sum 1; `out == in` the identity
   for every filter (this project's rule: a crop-only plan is an exact copy).
2. torch (``interpolate(bicubic, antialias=True)``) and Pillow (mode "F"
   ``BICUBIC``) on replicate-padded sources, as tests/test_border_evidence.py
   does for the triangle filter.  The pad is m * in/gcd source pixels and
   m * out/gcd output pixels, m the smallest integer with
   m * in/gcd >= ceil(2 * max(1, in/out)) + 2: multiples of in/gcd keep the
   grids aligned, and the cubic support needs more than one.
3. A C restatement in kernel order (tests/native/filter_vfirst.c, compiled
   here with the host C compiler): vertical pass first in byte units, fmaf
   chains in tap order from 0, then the horizontal pass, then stbir's encode,
   over tap tables passed in (the product's, from mxd_axis_taps_filter) -- the
   "bit-exact when the tables are shared" gate of the GPU kernels.

`run_device` runs images through mxd_resize_crop_batch with a filter each.
"""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np

FILTERS = ("triangle", "catmullrom", "mitchell", "cubicbspline")
CUBICS = FILTERS[1:]


def _tent(x):
    return np.maximum(0.0, 1.0 - x)


def _catmullrom(x):
    return np.where(x < 1, 1 - x * x * (2.5 - 1.5 * x), np.where(x < 2, 2 - x * (4 + x * (0.5 * x - 2.5)), 0.0))


def _mitchell(x):
    return np.where(x < 1, (16 + x * x * (21 * x - 36)) / 18,
                    np.where(x < 2, (32 + x * (-60 + x * (36 - 7 * x))) / 18, 0.0))


def _bspline(x):
    return np.where(x < 1, (4 + x * x * (3 * x - 6)) / 6, np.where(x < 2, (8 + x * (-12 + x * (6 - x))) / 6, 0.0))


# name -> (kernel of |distance|, support)
KERNELS = {"triangle": (_tent, 1.0), "catmullrom": (_catmullrom, 2.0), "mitchell": (_mitchell, 2.0),
           "cubicbspline": (_bspline, 2.0)}


def axis_matrix(n_in, n_out, filter):
    """(n_out, n_in) float64 weights of one axis, clamp-folded and row-normalised."""
    if n_in == n_out:
        return np.eye(n_in)
    kernel, support = KERNELS[filter]
    s = n_out / n_in
    j = np.arange(n_out, dtype=np.float64)[:, None]
    centre = (j + 0.5) / s
    if s >= 1.0:
        lo = np.floor(centre - support).astype(np.int64) - 1
        n = lo + np.arange(int(2 * support) + 3)[None, :]
        w = kernel(np.abs((n + 0.5) - centre))
    else:
        radius = support / s
        lo = np.floor(centre - radius).astype(np.int64) - 1
        n = lo + np.arange(int(np.ceil(2 * radius)) + 4)[None, :]
        w = s * kernel(np.abs((j + 0.5) - (n + 0.5) * s))
    idx = np.clip(n, 0, n_in - 1)
    m = np.zeros((n_out, n_in), np.float64)
    rows = np.broadcast_to(np.arange(n_out)[:, None], idx.shape)
    np.add.at(m, (rows, idx), w)
    m /= m.sum(axis=1, keepdims=True)
    return m


def resize_float(img, dw, dh, filter):
    """(dh, dw, C) float64 values in byte units (before the encode)."""
    h, w, c = img.shape
    v = img.astype(np.float64)
    t = np.einsum("yh,hwc->ywc", axis_matrix(h, dh, filter), v)
    return np.einsum("xw,ywc->yxc", axis_matrix(w, dw, filter), t)


def encode(v255):
    """trunc(clamp(v + 0.5, 0, 255)) of values in byte units."""
    return np.trunc(np.clip(v255 + 0.5, 0, 255)).astype(np.uint8)


def resize(img, dw, dh, filter):
    return encode(resize_float(img, dw, dh, filter))


def resize_crop(img, g, filter):
    """The float64 restatement of a geometry tuple (rw, rh, cx, cy, cw, ch, flip)."""
    rw, rh, cx, cy, cw, ch, flip = g
    out = resize(img, rw, rh, filter)[cy:cy + ch, cx:cx + cw]
    return out[:, ::-1] if flip else out


def pads(n_in, n_out):
    """(source pad, output pad) of the replicate-padded cubic cross-checks."""
    g = math.gcd(n_in, n_out)
    need = math.ceil(2 * max(1.0, n_in / n_out)) + 2
    m = -(-need // (n_in // g))
    return m * (n_in // g), m * (n_out // g)


def torch_clamp(img, dw, dh):
    import torch

    h, w, c = img.shape
    px, mx = pads(w, dw)
    py, my = pads(h, dh)
    t = torch.from_numpy(np.pad(img.astype(np.float64) / 255.0, ((py, py), (px, px), (0, 0)), mode="edge"))
    t = t.permute(2, 0, 1)[None]
    o = torch.nn.functional.interpolate(t, size=(dh + 2 * my, dw + 2 * mx), mode="bicubic", antialias=True,
                                        align_corners=False)
    return encode(o[0, :, my:my + dh, mx:mx + dw].permute(1, 2, 0).numpy() * 255.0)


def pillow_clamp(img, dw, dh):
    import pytest

    Image = pytest.importorskip("PIL.Image")
    h, w, c = img.shape
    px, mx = pads(w, dw)
    py, my = pads(h, dh)
    p = np.pad(img.astype(np.float32) / 255.0, ((py, py), (px, px), (0, 0)), mode="edge")
    planes = [np.asarray(Image.fromarray(p[:, :, k], mode="F").resize((dw + 2 * mx, dh + 2 * my), Image.BICUBIC))
              for k in range(c)]
    return encode(np.stack(planes, -1)[my:my + dh, mx:mx + dw].astype(np.float64) * 255.0)


def stats(a, b):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return int(d.max()), float((d > 0).mean())


def gate(ref, other):
    """The project's resize gate: max |d| <= 1, and on frames >= 64 x 64 fewer
    than 2e-3 of the channels differ."""
    m, frac = stats(ref, other)
    assert m <= 1, m
    if ref.shape[0] * ref.shape[1] >= 64 * 64:
        assert frac < 2e-3, frac
    return m, frac


# ---- the C restatement in kernel order -------------------------------------
_vfirst = None


def _vfirst_lib():
    global _vfirst
    if _vfirst is None:
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "filter_vfirst.c")
        out = os.path.join(tempfile.mkdtemp(prefix="filter_vfirst_"), "libfilter_vfirst.so")
        subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off",
                        "-Wall", "-o", out, src, "-lm"], check=True)
        _vfirst = ctypes.CDLL(out)
    return _vfirst


def _tables(n_in, n_out, filter):
    from mlx_data_amd import capi

    first, cnt, w = capi.axis_taps(n_in, n_out, filter=filter)
    return (np.ascontiguousarray(first, np.int32), np.ascontiguousarray(cnt, np.int32),
            np.ascontiguousarray(w, np.float32))


def vfirst(img, g, filter):
    """Kernel-order result of geometry g = (rw, rh, cx, cy, cw, ch, flip) with
    the product's tap tables of `filter` (channels filtered independently)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w, c = img.shape
    rw, rh, cx, cy, cw, ch, flip = g
    xf, xn, xw = _tables(w, rw, filter)
    yf, yn, yw = _tables(h, rh, filter)
    out = np.zeros((ch, cw, c), np.uint8)
    i32, f32, u8 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8)
    rc = _vfirst_lib().filter_vfirst(
        img.ctypes.data_as(u8), w, h, c, ctypes.c_int64(w * c), out.ctypes.data_as(u8),
        xf.ctypes.data_as(i32), xn.ctypes.data_as(i32), xw.ctypes.data_as(f32), xw.shape[1],
        yf.ctypes.data_as(i32), yn.ctypes.data_as(i32), yw.ctypes.data_as(f32), yw.shape[1],
        cx, cy, cw, ch, int(flip))
    assert rc == 0
    return out


F32_LUT = (np.arange(256, dtype=np.uint8).astype("float32") / 255).view(np.uint32)


# ---- the device call ---------------------------------------------------------
def run_device(images, geoms, filters, f32=False, base_shift=0, rgba_weighted=0, device=0, policy=None):
    """mxd_resize_crop_batch over (H, W, C) uint8 images with geometry tuples
    (rw, rh, cx, cy, cw, ch, flip) and one filter name each (or one for all).
    Sources are packed with 16-byte row pitches, each ``base_shift`` bytes past
    a 256-byte boundary.  Returns the outputs (uint8, or float32 when f32)."""
    from mlx_data_amd import capi

    if isinstance(filters, str):
        filters = [filters] * len(images)
    elem = 4 if f32 else 1
    pitches, offs, total = [], [], 0
    for img in images:
        h, w, c = img.shape
        p = (w * c + 15) // 16 * 16
        pitches.append(p)
        offs.append(total + base_shift)
        total += (p * h + 255) // 256 * 256
    src = capi.DeviceBuffer(total + 256, device)
    host = np.zeros(total + 256, np.uint8)
    for img, p, o in zip(images, pitches, offs):
        h, w, c = img.shape
        host[o:o + p * h].reshape(h, p)[:, :w * c] = img.reshape(h, w * c)
    src.upload(host)
    dsts, entries = [], []
    for img, g, p, o, f in zip(images, geoms, pitches, offs, filters):
        rw, rh, cx, cy, cw, ch, flip = g
        c = img.shape[2]
        dpitch = cw * c * elem
        d = capi.DeviceBuffer(dpitch * ch, device)
        d.memset(0)
        dsts.append((d, dpitch))
        entries.append(dict(src=src.ptr + o, src_stride=p, src_w=img.shape[1], src_h=img.shape[0], channels=c,
                            resize_w=rw, resize_h=rh, crop_x=cx, crop_y=cy, crop_w=cw, crop_h=ch, flip=int(flip),
                            dst=d.ptr, dst_stride=dpitch, rgba_weighted=int(rgba_weighted),
                            filter=capi.FILTERS[f]))
    arr, n = capi.make_images(entries)
    capi.resize_crop_batch(arr, n, capi.MXD_F32_DIV255 if f32 else capi.MXD_U8, device, None)
    outs = []
    for (d, dpitch), g, img in zip(dsts, geoms, images):
        cw, ch = g[4], g[5]
        c = img.shape[2]
        row = d.download((ch, dpitch), np.uint8)
        outs.append(row.view(np.float32).reshape(ch, cw, c) if f32 else row.reshape(ch, cw, c))
        d.free()
    src.free()
    return outs


def plan_of(img_shape, g, filter, f32=False, base_shift=0):
    """mxd_describe_plan of the image run_device would launch."""
    from mlx_data_amd import capi

    h, w, c = img_shape
    rw, rh, cx, cy, cw, ch, flip = g
    elem = 4 if f32 else 1
    e = dict(src=256 + base_shift, src_stride=(w * c + 15) // 16 * 16, src_w=w, src_h=h, channels=c, resize_w=rw,
             resize_h=rh, crop_x=cx, crop_y=cy, crop_w=cw, crop_h=ch, flip=int(flip), dst=256,
             dst_stride=cw * c * elem, filter=capi.FILTERS[filter])
    return capi.describe_plan(e, capi.MXD_F32_DIV255 if f32 else capi.MXD_U8)
