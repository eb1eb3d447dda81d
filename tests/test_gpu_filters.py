"""GPU: the cubic resize filters (Catmull-Rom, Mitchell, cubic B-spline).

Every scatter wave kernel wave_cubic.hip instantiates is reached by the
smallest whole-frame image its ratio needs (the route is confirmed with
mxd_describe_plan), in one and in two strips, over three bands of output rows
with a short last band, with crop windows that touch x = 0, y = 0 and the far
edges, mirrored or not, and from an unaligned base; then the clamp, the
fallback routes (4-tap upsampling, ratios past the largest tap bucket, 1 / 2 /
4 channels, a mixed batch), formatted output, a 4:2:0 JPEG source and the host
path.  The u8 result must be bit-equal to the C restatement in kernel order
over the product's tap tables (tests/filter_ref.py vfirst), f32 exactly
LUT[u8], and frames of 64 x 64 and more within the +-1 / 2e-3 gate of the
float64 restatement.  Nothing expected comes from the code under test."""
import ctypes
import os

import numpy as np
import pytest

import filter_ref as R
from gpu_util import synth
from mlx_data_amd import capi

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz")


def whole(cw, ch, flip=0):
    return (cw, ch, 0, 0, cw, ch, flip)


def check(imgs, geoms, filters, base_shift=0, f32=True, rgba_weighted=0, float64_gate=True):
    """Runs the batch as u8 (and f32) and holds every image to the references."""
    if isinstance(filters, str):
        filters = [filters] * len(imgs)
    u8 = R.run_device(imgs, geoms, filters, base_shift=base_shift, rgba_weighted=rgba_weighted)
    for img, g, f, out in zip(imgs, geoms, filters, u8):
        assert np.array_equal(out, R.vfirst(img, g, f)), (img.shape, g, f)
        if float64_gate and g[4] >= 64 and g[5] >= 64:
            R.gate(R.resize_crop(img, g, f), out)
    if f32:
        for a, b in zip(R.run_device(imgs, geoms, filters, f32=True, base_shift=base_shift,
                                     rgba_weighted=rgba_weighted), u8):
            assert np.array_equal(a.view(np.uint32), R.F32_LUT[b])
    return u8


# (DMAX, taps, Q, P) -> (src w, src h, out w) of a whole-frame resize that takes
# it in one strip (or the fewest it ever takes) and one that takes it in two
SHAPES = {
    (2, 6, 2, 4): ((100, 29, 68), (258, 100, 176)),
    (2, 6, 4, 8): ((563, 29, 384), (563, 100, 384)),
    (2, 8, 2, 4): ((128, 38, 68), (262, 128, 140)),
    (2, 8, 4, 8): ((510, 38, 272), (510, 128, 272)),
    (3, 12, 2, 4): ((191, 56, 68), (371, 191, 132)),
    (3, 12, 2, 8): ((518, 56, 184), (518, 191, 184)),
    (4, 17, 1, 4): ((60, 75, 16), (270, 255, 72)),
    (4, 17, 2, 8): ((525, 75, 140), (525, 255, 140)),
    (5, 17, 1, 4): ((68, 84, 16), (270, 287, 64)),
    (5, 17, 2, 8): ((506, 84, 120), (557, 287, 132)),
    (6, 24, 1, 4): ((90, 112, 16), (270, 383, 48)),
    (6, 24, 2, 8): ((495, 112, 88), (742, 383, 132)),
}


def _out_h(sw, sh, cw):
    return max(1, round(sh * cw / sw))


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("filter", ["catmullrom"])
def test_every_cubic_scatter_kernel(shape, filter):
    dmax, taps, q, p = shape
    imgs, geoms, shifts = [], [], []
    for k, (sw, sh, cw) in enumerate(SHAPES[shape]):
        ch = _out_h(sw, sh, cw)  # 20 rows: bands of 8, 8 and 4; 68 rows: the float64 gate applies
        for shift in ((0, 1) if k else (0,)):  # (the one-strip sources' row pitch has no room for a shifted base)
            for f32 in (False, True):
                pf = R.plan_of((sh, sw, 3), whole(cw, ch), filter, f32=f32, base_shift=shift)
                assert (pf["wave"], pf["kind"], pf["s"], pf["dmax"], pf["taps"], pf["q"], pf["p"]) == \
                    (1, 2, 4, dmax, taps, q, p), (shape, sw, sh, cw, pf)
        assert ch % 8 != 0 and ch > 16
        plan = R.plan_of((sh, sw, 3), whole(cw, ch), filter)
        assert plan["nstrips"] == 2 if k else plan["nstrips"] <= 2
        img = synth(sh, sw, 3, 7 * k + dmax)
        # the whole frame, the whole frame mirrored, and an inner window at odd offsets, mirrored
        imgs += [img, img, img]
        geoms += [whole(cw, ch), whole(cw, ch, 1), (cw, ch, 3, 2, cw - 5, ch - 3, 1)]
    check(imgs, geoms, filter)
    check(imgs[3:5], geoms[3:5], filter, base_shift=1)  # an unaligned base: the realigning kernels


@pytest.mark.parametrize("filter", ["mitchell", "cubicbspline"])
def test_other_cubics_on_the_flagship_shapes(filter):
    """C2 and C4 (resize_smallest_side 256 -> center_crop 224) for the other two
    cubic filters: the same kernels with other weights."""
    imgs = [synth(960, 1280, 3, 0), synth(375, 500, 3, 1), synth(500, 333, 3, 2)]
    geoms = [(341, 256, 58, 16, 224, 224, 0), (341, 256, 58, 16, 224, 224, 1), (256, 384, 16, 80, 224, 224, 0)]
    for img, g in zip(imgs, geoms):
        p = R.plan_of(img.shape, g, filter)
        assert (p["wave"], p["kind"], p["s"]) == (1, 2, 4)
    check(imgs, geoms, filter)


def test_clamp_never_wraps():
    """A 0 / 255 checkerboard and a bright two-pixel border stripe under
    Catmull-Rom: the negative lobes overshoot below 0 and above 255 and the
    encode clamps."""
    yy, xx = np.mgrid[0:150, 0:270]
    board = np.repeat(((((yy // 5) + (xx // 5)) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    stripe = np.zeros((150, 270, 3), np.uint8)
    stripe[:, :2] = 255
    stripe[:2] = 255
    for img, both in ((board, True), (stripe, False)):
        for g in (whole(72, 40), (384, 213, 0, 0, 200, 100, 0)):  # a downscale on a cubic kernel, an upscale
            v = R.resize_float(img, g[0], g[1], "catmullrom")[g[3]:g[3] + g[5], g[2]:g[2] + g[4]]
            assert v.min() < -2 and (v.max() > 257 or not both)  # the input does overshoot (the stripe below 0 only)
            # (two-level images put many sums next to a rounding boundary, where f32 and f64 part by
            # one level: the differing fraction is not held to 2e-3 here, the distance below is)
            out = check([img], [g], "catmullrom", float64_gate=False)[0]
            assert (out[v < -0.01] == 0).all() and (out[v > 255.01] == 255).all()
            assert np.abs(out.astype(np.float64) - np.clip(v, 0, 255)).max() < 1.01


def test_fallback_routes():
    up = synth(40, 50, 3, 1)  # 4-tap upsampling: the gather kernel
    g_up = whole(64, 51)
    p = R.plan_of(up.shape, g_up, "catmullrom")
    assert (p["wave"], p["kind"], p["taps"]) == (1, 0, 4)
    far = synth(272, 544, 3, 2)  # 8.5 : 1, 34 taps: past the largest bucket
    g_far = whole(64, 32)
    assert R.plan_of(far.shape, g_far, "catmullrom")["wave"] == 0
    assert capi.axis_taps(544, 64, filter="catmullrom")[2].shape[1] > 32
    check([up], [g_up], "catmullrom")
    check([far], [g_far], "catmullrom")
    for c in (1, 2):
        img = synth(150, 270, c, c)
        check([img, img], [whole(72, 40), (72, 40, 5, 3, 60, 30, 1)], "mitchell")
    # one call holding triangle and Catmull-Rom images of one geometry, and an identity (crop-only) plan
    img = synth(255, 270, 3, 9)
    check([img, img, img, img], [whole(72, 68)] * 3 + [(270, 255, 7, 9, 100, 70, 1)],
          ["triangle", "catmullrom", "triangle", "cubicbspline"])


@pytest.mark.parametrize("weighted", [0, 1])
def test_four_channels(weighted):
    """Alpha 255 everywhere: the weighted and the unweighted form are both the
    per-channel resize, within +-1 of the float64 restatement."""
    img = synth(150, 270, 4, 3)
    img[:, :, 3] = 255
    for g in (whole(72, 40), whole(96, 100)):
        assert R.plan_of(img.shape, g, "catmullrom")["wave"] == 0
        out = R.run_device([img], [g], "catmullrom", rgba_weighted=weighted)[0]
        m, _ = R.stats(R.resize_crop(img, g, "catmullrom"), out)
        assert m <= 1
        assert (out[:, :, 3] == 255).all()


def test_formatted_output_from_the_surface():
    from mlx_data_amd import data as dx
    from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expected_table

    shapes = [(375, 500), (255, 270), (200, 300), (500, 375)]
    imgs = [dict(image=synth(*shapes[i % 4], 3, 20 + i)) for i in range(4)]
    b = (dx.buffer_from_vector(imgs).image_resize_smallest_side("image", 96, filter="catmullrom")
         .image_center_crop("image", 80, 80))
    u8 = b.batch(4)[0]["image"]
    for k, s in enumerate(imgs):
        h, w = s["image"].shape[:2]
        rw, rh = capi.resize_smallest_side_dims(w, h, 96)
        g = (rw, rh, (rw - 80) // 2, (rh - 80) // 2, 80, 80, 0)
        assert np.array_equal(u8[k], R.vfirst(s["image"], g, "catmullrom"))
    dev = (b.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="bfloat16", layout="chw")
           .batch(4, device=0)[0]["image"])
    table = expected_table("bfloat16", 3, IMAGENET_MEAN, IMAGENET_STD)
    want = np.stack([table[k][u8[..., k]] for k in range(3)], axis=1)  # (B, C, H, W) bits
    got = np.zeros(want.shape, np.uint16)
    capi.check(capi.lib().mxd_memcpy_d2h(ctypes.c_void_p(got.ctypes.data), ctypes.c_void_p(dev.data_ptr),
                                         ctypes.c_size_t(got.nbytes), 0))
    assert np.array_equal(got, want)


def test_jpeg_source(tmp_path):
    """A 4:2:0 file through load_image: the cubic resize of the device-decoded
    image equals the same chain on the decoded array."""
    from mlx_data_amd import data as dx

    gold = np.load(GOLD)
    path = tmp_path / "caltech.jpg"
    path.write_bytes(gold["caltech_300x200_jpg"].tobytes())
    rgb = gold["caltech_300x200_rgb"]

    def chain(b):
        return (b.image_resize_smallest_side("image", 128, filter="catmullrom").image_center_crop("image", 112, 112)
                .batch(2)[0]["image"])

    files = chain(dx.buffer_from_vector([dict(image=str(path).encode())] * 2).load_image("image"))
    arrays = chain(dx.buffer_from_vector([dict(image=rgb)] * 2))
    assert np.array_equal(files, arrays)
    assert np.array_equal(arrays[0], R.vfirst(rgb, (192, 128, 40, 8, 112, 112, 0), "catmullrom"))


@pytest.mark.parametrize("f32", [False, True])
def test_host_path_equals_the_device_call(f32):
    imgs = [synth(255, 270, 3, 1), synth(375, 500, 3, 2), synth(40, 50, 3, 3)]
    geoms = [(72, 68, 4, 2, 64, 64, 1), (128, 96, 20, 10, 80, 70, 0), whole(64, 51)]
    filters = ["catmullrom", "mitchell", "cubicbspline"]
    want = R.run_device(imgs, geoms, filters, f32=f32)
    elem = 4 if f32 else 1
    entries, dsts, keep = [], [], []
    for im, g, f in zip(imgs, geoms, filters):
        h, w, c = im.shape
        src = np.ascontiguousarray(im)  # pageable
        dst = np.zeros((g[5], g[4] * c * elem), np.uint8)
        keep.append(src)
        dsts.append(dst)
        entries.append(dict(src=src.ctypes.data, src_stride=w * c, src_w=w, src_h=h, channels=c, resize_w=g[0],
                            resize_h=g[1], crop_x=g[2], crop_y=g[3], crop_w=g[4], crop_h=g[5], flip=g[6],
                            dst=dst.ctypes.data, dst_stride=dst.shape[1], filter=capi.FILTERS[f]))
    arr, n = capi.make_images(entries)
    capi.resize_crop_host(arr, n, capi.MXD_F32_DIV255 if f32 else capi.MXD_U8, 0)
    for d, w_, g, im in zip(dsts, want, geoms, imgs):
        got = d.view(np.float32 if f32 else np.uint8).reshape(g[5], g[4], 3)
        assert np.array_equal(got.view(np.uint32) if f32 else got, w_.view(np.uint32) if f32 else w_)
    # the cubic footprint of the same window is wider than the triangle's
    for f in R.CUBICS:
        first, cnt, _ = capi.axis_taps(255, 68, 2, 64, filter=f)
        t_first, t_cnt, _ = capi.axis_taps(255, 68, 2, 64)
        assert first.min() < t_first.min() and (first + cnt).max() > (t_first + t_cnt).max()
