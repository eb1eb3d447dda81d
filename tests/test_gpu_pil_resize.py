"""GPU: Pillow's 8-bit resize filters (pil_resize_rows) against Pillow itself,
byte for byte -- every geometry of pil_resize_cases in both output modes and
three memory layouts, beside a float-filter image, from host memory, in front
of the stage chain, and from the operator surface."""
import ctypes

import numpy as np
import pytest
from PIL import Image, ImageFilter

import pil_resize_cases as P
from mlx_data_amd import capi

pytestmark = pytest.mark.gpu

# source base shift, source row padding past 4-byte rows, destination shift in elements (rows then 3 elements longer)
LAYOUTS = {"aligned": (0, 0, 0), "shifted": (1, 4, 1), "odd_stride": (1, 5, 1)}


def launch(images, geoms, filters, f32=False, layout="aligned"):
    """mxd_resize_crop_batch of (H, W, C) images; every destination is checked
    to keep its bytes outside the window's elements."""
    shift, pad, dshift = LAYOUTS[layout]
    elem = 4 if f32 else 1
    bufs, entries = [], []
    for a, g, f in zip(images, geoms, filters):
        h, w, c = a.shape
        stride = (w * c + 3) // 4 * 4 + pad
        host = np.zeros(shift + stride * h, np.uint8)
        host[shift:].reshape(h, stride)[:, :w * c] = a.reshape(h, w * c)
        src = capi.DeviceBuffer(host.size)
        src.upload(host)
        x, y, cw, ch = g[4] or (0, 0, g[2], g[3])
        dstride = (cw * c + (3 if dshift else 0)) * elem
        dst = capi.DeviceBuffer(dshift * elem + dstride * ch)
        dst.memset(0xEE)
        bufs.append((src, dst, dstride, (ch, cw, c)))
        entries.append(dict(src=src.ptr + shift, src_stride=stride, src_w=w, src_h=h, channels=c, resize_w=g[2],
                            resize_h=g[3], crop_x=x, crop_y=y, crop_w=cw, crop_h=ch, flip=g[5], dst=dst.ptr + dshift * elem,
                            dst_stride=dstride, filter=capi.FILTERS[f]))
    arr, n = capi.make_images(entries)
    capi.resize_crop_batch(arr, n, capi.MXD_F32_DIV255 if f32 else capi.MXD_U8, 0, None)
    outs = []
    for src, dst, dstride, (ch, cw, c) in bufs:
        raw = dst.download((dst.nbytes,), np.uint8)
        rows = raw[dshift * elem:].reshape(ch, dstride)
        assert (raw[:dshift * elem] == 0xEE).all() and (rows[:, cw * c * elem:] == 0xEE).all()
        body = rows[:, :cw * c * elem].copy()
        outs.append(body.view(np.float32).reshape(ch, cw, c) if f32 else body.reshape(ch, cw, c))
        src.free()
        dst.free()
    return outs


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("geom,filter", P.CASES, ids=P.IDS)
def test_device_call_is_pillow(geom, filter, channels, layout):
    a = P.image(geom[0], geom[1], channels)
    want = P.pillow(a, geom, filter)
    assert np.array_equal(launch([a], [geom], [filter], layout=layout)[0], want)
    f32 = launch([a], [geom], [filter], f32=True, layout=layout)[0]
    assert np.array_equal(f32.view(np.uint32), (want.astype(np.float32) / np.float32(255)).view(np.uint32))


def test_one_call_mixes_float_and_pillow_filters():
    import filter_ref as R

    a, b, c = P.image(70, 90, 3, 1), P.image(105, 207, 3, 2), P.image(24, 320, 3, 3)
    ga, gb, gc = P.GEOMS[0], P.GEOMS[8], P.GEOMS[7]
    # (the 97-tap image widens the launch's staged entries past the last image's own 32-word entries)
    tri, pil, wide, pil2 = launch([a, b, c, a], [ga, gb, gc, ga], ["triangle", "pil_lanczos", "pil_lanczos", "pil_bicubic"])
    assert np.array_equal(tri, R.run_device([a], [(24, 19, 0, 0, 24, 19, 0)], "triangle")[0])
    assert np.array_equal(pil, P.pillow(b, gb, "pil_lanczos")) and np.array_equal(wide, P.pillow(c, gc, "pil_lanczos"))
    assert np.array_equal(pil2, P.pillow(a, ga, "pil_bicubic"))


@pytest.mark.parametrize("f32", [False, True])
def test_host_path_equals_the_device_call(f32):
    geoms = [P.GEOMS[9], P.GEOMS[10], P.GEOMS[1]]  # the windowed geometry (a staged footprint), flipped too
    imgs = [P.image(g[0], g[1], 3, k) for k, g in enumerate(geoms)]
    filters = ["pil_bicubic", "pil_lanczos", "pil_bilinear"]
    want = launch(imgs, geoms, filters, f32=f32)
    elem = 4 if f32 else 1
    entries, dsts = [], []
    for a, g, f, w_ in zip(imgs, geoms, filters, want):
        x, y, cw, ch = g[4] or (0, 0, g[2], g[3])
        dsts.append(np.zeros((ch, cw * 3 * elem), np.uint8))
        entries.append(dict(src=a.ctypes.data, src_stride=a.strides[0], src_w=g[1], src_h=g[0], channels=3,
                            resize_w=g[2], resize_h=g[3], crop_x=x, crop_y=y, crop_w=cw, crop_h=ch, flip=g[5],
                            dst=dsts[-1].ctypes.data, dst_stride=cw * 3 * elem, filter=capi.FILTERS[f]))
    arr, n = capi.make_images(entries)
    capi.resize_crop_host(arr, n, capi.MXD_F32_DIV255 if f32 else capi.MXD_U8, 0)
    bits = np.uint32 if f32 else np.uint8
    for d, w_ in zip(dsts, want):
        assert np.array_equal(d.view(bits).reshape(w_.shape), w_.view(bits))


def test_chain_behind_the_resize():
    """pil_bicubic resize -> Pillow's GaussianBlur -> ImageNet-normalised bfloat16
    CHW: scratch rows A and B and the two-pass format route."""
    from out_format_util import IMAGENET_MEAN, IMAGENET_STD, FmtRun, expect, expected_table

    geoms = [P.GEOMS[0], P.GEOMS[9]]
    imgs = [P.image(g[0], g[1], 3, 5 + k) for k, g in enumerate(geoms)]
    run = FmtRun(imgs, [(g[2], g[3]) + (g[4] or (0, 0, g[2], g[3])) + (g[5],) for g in geoms], "bfloat16", "chw")
    try:
        for i in range(run.n):
            run.arr[i].filter = capi.FILTERS["pil_bicubic"]
        for d, _, _ in run.dsts:
            d.memset(0xFF)
        capi.resize_crop_batch_enhance(run.arr, None, capi.make_enhances([(capi.MXD_ENHANCE_PIL_GAUSSIAN_BLUR, 1.5)] * 2),
                                       None, None, run.n, capi.MXD_U8, run.fmt(IMAGENET_MEAN, IMAGENET_STD))
        capi.check(capi.lib().mxd_device_synchronize(0))
        outs, clean = run.read()
        plain, plain_clean = run.launch(IMAGENET_MEAN, IMAGENET_STD)  # the format alone: format_rows
    finally:
        run.free()
    table = expected_table("bfloat16", 3, IMAGENET_MEAN, IMAGENET_STD)
    for a, g, o, ok, po, pok in zip(imgs, geoms, outs, clean, plain, plain_clean):
        blurred = np.asarray(Image.fromarray(P.pillow(a, g, "pil_bicubic")).filter(ImageFilter.GaussianBlur(1.5)))
        assert ok and np.array_equal(o, expect(table, blurred))
        assert pok and np.array_equal(po, expect(table, P.pillow(a, g, "pil_bicubic")))


@pytest.mark.parametrize("seed", [3, 4])
def test_surface_is_the_pil_training_transform(seed):
    from mlx_data_amd import _pipeline
    from mlx_data_amd import data as dx

    a = P.image(150, 200, 3, seed)
    ds = (dx.buffer_from_vector([dict(image=a)]).image_random_area_crop("image", (0.3, 1.0), (0.75, 1.33))
          .image_resize("image", 64, 48, filter="pil_bicubic").image_random_h_flip("image", 0.5))
    dx.set_state(seed)
    p = _pipeline._plan(ds, 0, "image")
    dx.set_state(seed)
    got = ds.batch(1, device=0)[0]["image"].numpy()[0]
    x, y, w, h = p["window"]
    want = np.asarray(Image.fromarray(a).crop((x, y, x + w, y + h)).resize((64, 48), Image.BICUBIC))
    assert p["filter"] == "pil_bicubic" and (w, h) != (200, 150)
    assert np.array_equal(got, want[:, ::-1] if p["flip"] else want)


def test_jpeg_source_takes_the_rgb_frame_route(tmp_path):
    import os

    from mlx_data_amd import data as dx

    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz"))
    path = tmp_path / "caltech.jpg"
    path.write_bytes(gold["caltech_300x200_jpg"].tobytes())
    got = (dx.buffer_from_vector([dict(image=str(path).encode())] * 2).load_image("image")
           .image_resize("image", 96, 80, filter="pil_lanczos").batch(2)[0]["image"])
    want = np.asarray(Image.fromarray(gold["caltech_300x200_rgb"]).resize((96, 80), Image.LANCZOS))
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
