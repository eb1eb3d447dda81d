"""GPU: formatted outputs of the fused launch (mxd_resize_crop_batch_fmt and
its host-source / JPEG counterparts): normalised float32 / float16 / bfloat16
elements, HWC or CHW, written by the wave kernels' own store epilogue
(wave_fmt.hip) or, for images the band and general kernels resize, by the
format_rows pass behind them.

Expected values never come from the code under test: they are
table[oracle bytes], the oracle being the kernel-order restatement
O.resize_crop_vfirst (O.resize_crop_vfirst_rgba for weighted RGBA) and the
table the NumPy / torch expression of out_format_util.expected_table
(tests/test_out_format.py pins the library's own table to it).  Everything is
compared as integer bits, and every byte of a destination buffer outside the
image's elements must keep the 0xff it was filled with."""
import io

import numpy as np
import pytest

import oracle as O
from gpu_util import center_geom, synth
from mlx_data_amd import capi
from out_format_util import ELEMS, IMAGENET_MEAN, IMAGENET_STD, LAYOUTS, FmtRun, expect, expected_table

pytestmark = pytest.mark.gpu

FORMATS = [(e, l) for e in sorted(ELEMS) for l in sorted(LAYOUTS)]
# the formats a wave form or route is run in: both element sizes in both layouts
FOUR = [("bfloat16", "chw"), ("float32", "chw"), ("float16", "hwc"), ("float32", "hwc")]


def _norm(c):
    return (IMAGENET_MEAN + (0.5,))[:c], (IMAGENET_STD + (0.25,))[:c]


def _check(run, wants, mean=None, std=None, stream=None, tag=None):
    outs, clean = run.launch(mean, std, stream)
    for k, (o, w, ok) in enumerate(zip(outs, wants, clean)):
        c = w.shape[2]
        cut = (lambda v: v[:c] if isinstance(v, tuple) else v)
        table = expected_table(run.elem, c, cut(mean), cut(std))
        e = expect(table, w)
        assert o.shape == e.shape and o.dtype == e.dtype, (tag, k)
        bad = int((o != e).sum())
        assert bad == 0, (tag, run.elem, run.layout, k, run.geoms[k], bad, np.argwhere(o != e)[:3])
        assert ok, (tag, run.elem, run.layout, k, "bytes outside the image were written")


def _run_case(imgs, geoms, formats, tag, normalise=True, rgba_weighted=0, **kw):
    flags = rgba_weighted if isinstance(rgba_weighted, list) else [rgba_weighted] * len(imgs)
    wants = [O.resize_crop_vfirst_rgba(i, g) if wt else O.resize_crop_vfirst(i, g)
             for i, g, wt in zip(imgs, geoms, flags)]
    for elem, layout in formats:
        if layout == "chw" and len({i.shape[2] for i in imgs}) > 1:
            continue  # one channel count per CHW call
        run = FmtRun(imgs, geoms, elem, layout, rgba_weighted=rgba_weighted, **kw)
        try:
            mean, std = _norm(max(i.shape[2] for i in imgs)) if normalise else (None, None)
            _check(run, wants, mean, std, tag=tag)
        finally:
            run.free()


# ---- every table entry -------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_every_table_entry_in_every_format(channels):
    """Identity resizes of 16x16 images holding all 256 values in each
    channel (a different permutation per channel): every entry of every
    channel's table reaches the output, in all three element types and both
    layouts; 4 channels run the two-pass route."""
    rng = np.random.default_rng(channels)
    img = np.stack([rng.permutation(256).astype(np.uint8).reshape(16, 16) for _ in range(channels)], axis=2)
    g = (16, 16, 0, 0, 16, 16, 0)
    assert np.array_equal(O.resize_crop_vfirst(img, g), img)
    mean, std = _norm(channels)
    for elem, layout in FORMATS:
        run = FmtRun([img, img[::-1].copy()], [g, g], elem, layout)
        try:
            _check(run, [img, img[::-1]], mean, std, tag="normalised")
            _check(run, [img, img[::-1]], tag="div255")
            # a mean one float16 denormal below 1: denormal float16 results
            m = float(np.float32(1.0) - np.float32(2.0 ** -16))
            _check(run, [img, img[::-1]], m, 1.0, tag="denormal")
        finally:
            run.free()


# ---- partial lanes and offsets ----------------------------------------------

@pytest.mark.parametrize("elem,layout", FORMATS)
def test_partial_lanes_strides_and_offsets(elem, layout):
    """RGB crops of width 1, 63, 65, 224 and height 1, 7, plain and mirrored,
    rows 3 elements longer than the pixels, planes 5 elements longer than the
    rows, destinations one element past a 256-byte boundary (an odd multiple
    of the element size)."""
    img = synth(300, 400, 3, 5)
    rw, rh = 341, 256
    imgs, geoms = [], []
    for cw in (1, 63, 65, 224):
        for ch in (1, 7):
            for flip in (0, 1):
                imgs.append(img)
                geoms.append((rw, rh, 17 if cw < 224 else 58, 11, cw, ch, flip))
    wants = [O.resize_crop_vfirst(i, g) for i, g in zip(imgs, geoms)]
    mean, std = _norm(3)
    for pad, ppad, shift in ((0, 0, 0), (3, 5, 1)):
        run = FmtRun(imgs, geoms, elem, layout, dst_pad=pad, plane_pad=ppad, dst_shift=shift)
        try:
            _check(run, wants, mean, std, tag=(pad, ppad, shift))
        finally:
            run.free()


# ---- each wave form ------------------------------------------------------------

def _plan(img, g, policy=0):
    e = dict(src_w=img.shape[1], src_h=img.shape[0], src_stride=(img.shape[1] * img.shape[2] + 15) // 16 * 16,
             channels=img.shape[2], resize_w=g[0], resize_h=g[1], crop_x=g[2], crop_y=g[3], crop_w=g[4], crop_h=g[5],
             flip=g[6], dst_stride=g[4] * img.shape[2] * 4)
    prev = capi.set_kernel_policy(policy)
    try:
        return capi.describe_plan(e, capi.MXD_U8)
    finally:
        capi.set_kernel_policy(prev)


def _with_policy(policy, f):
    prev = capi.set_kernel_policy(policy)
    try:
        return f()
    finally:
        capi.set_kernel_policy(prev)


C4_SHAPES = [(375, 500), (500, 375), (333, 500), (200, 300)]


def _c4():
    imgs = [synth(h, w, 3, 70 + k) for k, (h, w) in enumerate(C4_SHAPES)]
    return imgs, [center_geom(i) for i in imgs]


def _c2():
    imgs = [synth(960, 1280, 3, s) for s in range(2)]
    return imgs, [center_geom(i) for i in imgs]


def test_scatter_and_upsampling_kernels():
    imgs, geoms = _c4()
    plans = [_plan(i, g) for i, g in zip(imgs, geoms)]
    assert all(p["wave"] == 1 and p["kind"] == 2 for p in plans), plans
    assert plans[3]["s"] == 3 and plans[3]["dmax"] == 1, plans[3]  # 200 -> 256: the upsampling schedule
    _run_case(imgs, geoms, FOUR, "c4")
    img = synth(480, 640, 3, 9)
    g = center_geom(img)
    p = _plan(img, g)
    assert (p["wave"], p["kind"], p["dmax"]) == (1, 2, 2), p
    _run_case([img], [g], FOUR, "480p")


@pytest.mark.parametrize("name,policy,p,nstrips", [
    ("default", capi.MXD_POLICY_AUTO, 8, 2), ("bytes", capi.MXD_POLICY_BYTES, 16, 3),
    ("narrow", capi.MXD_POLICY_NARROW, 4, None)])
def test_c2_kernels_with_several_strips_per_row(name, policy, p, nstrips):
    """Two 960x1280 -> 256 -> 224^2 images: C2's kernel, two strips per row
    (three with byte lanes) -- where a wrong CHW strip offset shows."""
    imgs, geoms = _c2()
    plan = _plan(imgs[0], geoms[0], policy)
    assert plan["wave"] == 1 and plan["kind"] == 2 and plan["p"] == p, plan
    assert plan["nstrips"] >= 2 and (nstrips is None or plan["nstrips"] == nstrips), plan
    _with_policy(policy, lambda: _run_case(imgs, geoms, FOUR, name))


def test_gather_kernels():
    """MXD_POLICY_NO_SCATTER (RGB) and 1- / 2-channel 300x200 images."""
    imgs, geoms = _c2()
    plan = _plan(imgs[0], geoms[0], capi.MXD_POLICY_NO_SCATTER)
    assert plan["wave"] == 1 and plan["kind"] == 0, plan
    _with_policy(capi.MXD_POLICY_NO_SCATTER, lambda: _run_case(imgs[:1], geoms[:1], FOUR, "no_scatter"))
    for c in (1, 2):
        img = synth(200, 300, c, 20 + c)
        g = center_geom(img)
        plan = _plan(img, g)
        assert plan["wave"] == 1 and plan["kind"] == 0, (c, plan)
        _run_case([img, img], [g, g[:6] + (1,)], FOUR, f"gather{c}")


# ---- the two-pass route --------------------------------------------------------

@pytest.mark.parametrize("name,policy", [("band", capi.MXD_POLICY_PREFER_BAND), ("general", capi.MXD_POLICY_NO_WAVE)])
def test_two_pass_route_behind_band_and_general_kernels(name, policy):
    imgs, geoms = _c4()
    if name == "band":
        e = dict(src_w=500, src_h=375, src_stride=1504, channels=3, resize_w=geoms[0][0], resize_h=geoms[0][1],
                 crop_x=geoms[0][2], crop_y=geoms[0][3], crop_w=224, crop_h=224, flip=0, dst_stride=224 * 3)
        plan = _with_policy(policy, lambda: capi.describe_band_plan(e, capi.MXD_U8))
        assert plan["band"] == 1, plan
    _with_policy(policy, lambda: _run_case(imgs, geoms, FOUR, name, dst_pad=1, plane_pad=3, dst_shift=1))


def test_two_pass_route_weighted_rgba_and_unaligned_rows():
    img = synth(90, 120, 4, 31)
    g = (64, 48, 0, 0, 64, 48, 0)
    _run_case([img, img], [g, g[:6] + (1,)], FOUR, "rgba", rgba_weighted=1)
    # tightly packed RGB rows (not 4-byte aligned): no wave kernel takes them
    img = synth(99, 101, 3, 32)
    g = (75, 70, 3, 2, 61, 33, 1)
    _run_case([img], [g], FOUR, "packed", src_align=1)


# ---- a mixed batch -----------------------------------------------------------

@pytest.mark.parametrize("streams", [1, 2])
def test_mixed_batch_of_every_route(streams):
    """The shapes of the wave-form and two-pass groups in one call (HWC: 1, 2,
    3 and 4 channels together, the weighted RGBA 120x90 -> 64x48 among them;
    CHW: the RGB ones), its launches over one and two streams."""
    imgs, geoms = _c4()
    a, b = _c2()
    imgs, geoms = imgs + a, geoms + b
    imgs.append(synth(480, 640, 3, 9))
    geoms.append(center_geom(imgs[-1]))
    imgs.append(synth(99, 101, 3, 32))  # a small mirrored window
    geoms.append((75, 70, 3, 2, 61, 33, 1))
    rgb = (list(imgs), list(geoms))
    for c in (1, 2, 4):
        imgs.append(synth(200, 300, c, 20 + c))
        geoms.append(center_geom(imgs[-1]))
    weighted = [0] * len(imgs) + [1]
    imgs.append(synth(90, 120, 4, 31))  # alpha-weighted: the rgba_weighted sub-batch of the call
    geoms.append((64, 48, 0, 0, 64, 48, 0))
    ps = capi.set_tuning(capi.MXD_TUNE_STREAMS, streams)
    try:
        _run_case(imgs, geoms, [("float16", "hwc"), ("float32", "hwc")], "mixed", src_align=4,
                  rgba_weighted=weighted)
        _run_case(rgb[0], rgb[1], [("bfloat16", "chw"), ("float32", "chw")], "mixed_rgb", src_align=4)
    finally:
        capi.set_tuning(capi.MXD_TUNE_STREAMS, ps)


# ---- cache hazards -----------------------------------------------------------

@pytest.mark.parametrize("two_pass", [False, True])
def test_same_descriptors_with_two_formats(two_pass):
    """The same descriptor array and destinations launched on one stream
    with two formats (the descriptor slot of the first launch is a cache hit
    for the second): each launch's output is its own format's, also when the
    two alternate over 40 calls."""
    imgs, geoms = _c4()
    policy = capi.MXD_POLICY_NO_WAVE if two_pass else capi.MXD_POLICY_AUTO
    wants = [O.resize_crop_vfirst(i, g) for i, g in zip(imgs, geoms)]
    stream = capi.Stream(0)
    run = FmtRun(imgs, geoms, "float16", "chw")
    prev = capi.set_kernel_policy(policy)
    try:
        formats = [("float16", IMAGENET_MEAN, IMAGENET_STD), ("bfloat16", None, None)]
        for k in range(2):
            run.elem = formats[k][0]
            _check(run, wants, formats[k][1], formats[k][2], stream=stream, tag=("first", k))
        for k in range(40):
            run.elem, mean, std = formats[k % 2]
            capi.resize_crop_batch_fmt(run.arr, run.n, run.fmt(mean, std), 0, stream.handle)
            if k >= 38:
                stream.synchronize()
                outs, _ = run.read()
                for o, w in zip(outs, wants):
                    assert np.array_equal(o, expect(expected_table(run.elem, 3, mean, std), w)), k
        stream.synchronize()
    finally:
        capi.set_kernel_policy(prev)
        run.free()
        stream.close()


# ---- host sources and JPEG plane sources ---------------------------------------

def _device_dsts(geoms, c, es, chw):
    plane = max(g[4] * es * g[5] for g in geoms) if chw else 0
    bufs = []
    for g in geoms:
        cw, ch = g[4], g[5]
        row = cw * (1 if chw else c) * es
        d = capi.DeviceBuffer(plane * c if chw else row * ch, 0)
        d.memset(0xFF)
        bufs.append((d, row))
    capi.check(capi.lib().mxd_device_synchronize(0))
    return bufs, plane


def _read_dsts(bufs, geoms, c, es, chw, plane):
    ut = np.uint32 if es == 4 else np.uint16
    outs = []
    for (d, row), g in zip(bufs, geoms):
        cw, ch = g[4], g[5]
        if chw:
            raw = d.download((c, plane), np.uint8)
            outs.append(np.stack([raw[k, : row * ch].reshape(ch, row).copy().view(ut) for k in range(c)], axis=2))
        else:
            outs.append(d.download((ch, row), np.uint8).view(ut).reshape(ch, cw, c))
        d.free()
    return outs


@pytest.mark.parametrize("elem,layout", FOUR)
def test_host_sources_to_formatted_device_destinations(elem, layout):
    """mxd_resize_crop_to_device_fmt: pageable host sources, the chunk
    driver's launches write the format (wave and two-pass images together)."""
    imgs, geoms = _c4()
    imgs.append(synth(99, 101, 3, 32))
    geoms.append((75, 70, 3, 2, 61, 33, 1))
    es, chw = (4 if elem == "float32" else 2), layout == "chw"
    bufs, plane = _device_dsts(geoms, 3, es, chw)
    entries = []
    for img, g, (d, row) in zip(imgs, geoms, bufs):
        entries.append(dict(src=img.ctypes.data, src_stride=img.shape[1] * 3, src_w=img.shape[1], src_h=img.shape[0],
                            channels=3, resize_w=g[0], resize_h=g[1], crop_x=g[2], crop_y=g[3], crop_w=g[4],
                            crop_h=g[5], flip=g[6], dst=d.ptr, dst_stride=row))
    arr, n = capi.make_images(entries)
    mean, std = _norm(3)
    capi.resize_crop_to_device_fmt(arr, n, capi.make_out_format(ELEMS[elem], LAYOUTS[layout], mean, std, plane), 0)
    outs = _read_dsts(bufs, geoms, 3, es, chw, plane)
    table = expected_table(elem, 3, mean, std)
    for img, g, o in zip(imgs, geoms, outs):
        assert np.array_equal(o, expect(table, O.resize_crop_vfirst(img, g))), g


@pytest.mark.parametrize("elem,layout", [("bfloat16", "chw"), ("float32", "hwc")])
def test_jpeg_plane_sources_write_the_format(elem, layout):
    """4:2:0 JPEGs of 375x500 and 500x375 through
    mxd_jpeg_resize_crop_to_device_fmt: resized straight from their sample
    planes (mxd_jpeg_plane_sources counts both) into the formatted batch; the
    expectation is the oracle on Pillow's decode."""
    from PIL import Image

    datas, pixels, geoms = [], [], []
    for k, (h, w) in enumerate(((375, 500), (500, 375))):
        b = io.BytesIO()
        Image.fromarray(synth(h, w, 3, 40 + k)).save(b, "JPEG", quality=90, subsampling=2)
        datas.append(b.getvalue())
        pixels.append(np.asarray(Image.open(io.BytesIO(datas[-1])).convert("RGB")))
        geoms.append(center_geom(pixels[-1]))
    coefs = [capi.JpegCoefs(d) for d in datas]
    es, chw = (4 if elem == "float32" else 2), layout == "chw"
    bufs, plane = _device_dsts(geoms, 3, es, chw)
    entries = [dict(coefs=c, resize_w=g[0], resize_h=g[1], crop_x=g[2], crop_y=g[3], crop_w=g[4], crop_h=g[5],
                    flip=g[6], dst=d.ptr, dst_stride=row) for c, g, (d, row) in zip(coefs, geoms, bufs)]
    arr, n = capi.make_jpeg_images(entries)
    mean, std = _norm(3)
    capi.jpeg_plane_sources(reset=True)
    capi.jpeg_resize_crop_to_device_fmt(arr, n, capi.make_out_format(ELEMS[elem], LAYOUTS[layout], mean, std, plane), 0)
    assert capi.jpeg_plane_sources(reset=True) == 2
    outs = _read_dsts(bufs, geoms, 3, es, chw, plane)
    table = expected_table(elem, 3, mean, std)
    for px, g, o in zip(pixels, geoms, outs):
        assert np.array_equal(o, expect(table, O.resize_crop_vfirst(px, g))), g
    for c in coefs:
        c.close()


def test_existing_dtype_calls_are_unchanged_beside_formatted_ones():
    """A formatted launch between two MXD_F32_DIV255 launches of the same
    descriptors leaves theirs as they were: q / 255 of the oracle's bytes."""
    from gpu_util import run_device

    imgs, geoms = _c4()
    lut = (np.arange(256, dtype=np.uint8).astype("float32") / 255).view(np.uint32)
    wants = [O.resize_crop_vfirst(i, g) for i, g in zip(imgs, geoms)]
    for _ in range(2):
        for o, w in zip(run_device(imgs, geoms, f32=True), wants):
            assert np.array_equal(o.view(np.uint32), lut[w])
        _run_case(imgs, geoms, [("float32", "hwc")], "between")
