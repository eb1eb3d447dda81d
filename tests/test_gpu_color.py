"""GPU: the colour calls of the C ABI (mxd_resize_crop_batch_color and its
host-source / JPEG counterparts).  The expectation is always the NumPy
expression of the colour map (tests/color_ref.py) applied to the u8 result of
the same call without colour, then the format table (the NumPy / torch
statement of out_format_util.expected_table).  Everything is compared as
integer bits, and every byte of a destination buffer outside the image's
elements must keep the 0xff it was filled with."""
import ctypes
import os

import numpy as np
import pytest

import color_ref as R
from gpu_util import synth
from mlx_data_amd import capi
from out_format_util import ELEMS, IMAGENET_MEAN, IMAGENET_STD, LAYOUTS, expect, expected_table

pytestmark = pytest.mark.gpu

# (name, elem or None, layout, normalise): the output forms of a colour call
U8 = ("u8", None, "hwc", False)
F32 = ("f32", "float32", "hwc", False)
FORMATTED = [(f"{e}-{l}", e, l, True) for e in ("float32", "float16", "bfloat16") for l in ("hwc", "chw")]
MODES = [U8, F32] + FORMATTED


def _es(mode):
    return 1 if mode[1] is None else 4 if mode[1] == "float32" else 2


def _expected(mode, q, m):
    """What the call must write for u8 result bytes q under matrix m."""
    p = R.apply_ref(q, m)
    if mode[1] is None:
        return p
    mean, std = (IMAGENET_MEAN, IMAGENET_STD) if mode[3] else (None, None)
    return expect(expected_table(mode[1], 3, mean, std), p)


class Sources:
    """RGB images in one device buffer (row pitch rounded to src_align[i]
    bytes; 1 = packed) and the geometry of each: (rw, rh, cx, cy, cw, ch, flip)."""

    def __init__(self, images, geoms, filters=None, src_align=16):
        self.images, self.geoms = images, geoms
        self.filters = filters or [0] * len(images)
        aligns = src_align if isinstance(src_align, list) else [src_align] * len(images)
        self.pitches, self.offs, total = [], [], 0
        for img, a in zip(images, aligns):
            h, w, c = img.shape
            self.pitches.append((w * c + a - 1) // a * a)
            self.offs.append(total)
            total += (self.pitches[-1] * h + 255) // 256 * 256
        self.total = total + 256
        self.src = capi.DeviceBuffer(self.total, 0)
        self.upload(images)

    def upload(self, images):
        host = np.zeros(self.total, np.uint8)
        for img, p, o in zip(images, self.pitches, self.offs):
            h, w, c = img.shape
            host[o: o + p * h].reshape(h, p)[:, : w * c] = img.reshape(h, w * c)
        self.src.upload(host)

    def entries(self, dsts):
        out = []
        for img, g, p, o, f, (dp, dpitch) in zip(self.images, self.geoms, self.pitches, self.offs, self.filters, dsts):
            out.append(dict(src=self.src.ptr + o, src_stride=p, src_w=img.shape[1], src_h=img.shape[0], channels=3,
                            resize_w=g[0], resize_h=g[1], crop_x=g[2], crop_y=g[3], crop_w=g[4], crop_h=g[5],
                            flip=int(g[6]), dst=dp, dst_stride=dpitch, filter=f))
        return out

    def plain_u8(self):
        """The u8 results of mxd_resize_crop_batch on the same images."""
        bufs = [capi.DeviceBuffer(g[4] * 3 * g[5], 0) for g in self.geoms]
        arr, n = capi.make_images(self.entries([(b.ptr, g[4] * 3) for b, g in zip(bufs, self.geoms)]))
        capi.resize_crop_batch(arr, n, capi.MXD_U8, 0, None)
        outs = [b.download((g[5], g[4], 3), np.uint8) for b, g in zip(bufs, self.geoms)]
        for b in bufs:
            b.free()
        return outs

    def free(self):
        self.src.free()


class Dsts:
    """Destinations of one output form for a list of geometries: rows dst_pad
    elements longer than the pixels, planes plane_pad elements longer than
    crop_h rows, each base dst_shift elements past a 256-byte boundary."""

    def __init__(self, geoms, mode, dst_pad=0, plane_pad=0, dst_shift=0):
        self.geoms, self.mode, self.es, self.chw, self.shift = geoms, mode, _es(mode), mode[2] == "chw", dst_shift
        es = self.es
        self.plane = max((g[4] + dst_pad) * es * g[5] for g in geoms) + plane_pad * es if self.chw else 0
        self.bufs = []
        for g in geoms:
            dpitch = (g[4] * (1 if self.chw else 3) + dst_pad) * es
            size = self.plane * 3 if self.chw else dpitch * g[5]
            self.bufs.append((capi.DeviceBuffer(size + 256 + dst_shift * es, 0), dpitch, size))

    def pairs(self):
        return [(d.ptr + self.shift * self.es, dpitch) for d, dpitch, _ in self.bufs]

    def fmt(self):
        _, elem, layout, norm = self.mode
        if elem is None or self.mode is F32:
            return None
        mean, std = (IMAGENET_MEAN, IMAGENET_STD) if norm else (None, None)
        return capi.make_out_format(ELEMS[elem], LAYOUTS[layout], mean, std, self.plane)

    def dtype(self):
        return capi.MXD_F32_DIV255 if self.mode is F32 else capi.MXD_U8

    def clear(self):
        for d, _, _ in self.bufs:
            d.memset(0xFF)
        capi.check(capi.lib().mxd_device_synchronize(0))

    def read(self):
        """Per image: (H, W, 3) integer bits, and whether every byte outside them kept 0xff."""
        es, sh = self.es, self.shift * self.es
        ut = {1: np.uint8, 2: np.uint16, 4: np.uint32}[es]
        outs, clean = [], []
        for (d, dpitch, size), g in zip(self.bufs, self.geoms):
            cw, ch = g[4], g[5]
            raw = d.download((size + 256 + sh,), np.uint8)
            mask = np.ones(raw.shape, bool)
            if self.chw:
                planes = []
                for k in range(3):
                    at = sh + k * self.plane
                    planes.append(raw[at: at + dpitch * ch].reshape(ch, dpitch)[:, : cw * es].copy().view(ut))
                    mask[at: at + dpitch * ch].reshape(ch, dpitch)[:, : cw * es] = False
                outs.append(np.stack(planes, axis=2))
            else:
                rows = raw[sh: sh + dpitch * ch].reshape(ch, dpitch)
                outs.append(rows[:, : cw * 3 * es].copy().view(ut).reshape(ch, cw, 3))
                mask[sh: sh + dpitch * ch].reshape(ch, dpitch)[:, : cw * 3 * es] = False
            clean.append(bool((raw[mask] == 0xFF).all()))
        return outs, clean

    def free(self):
        for d, _, _ in self.bufs:
            d.free()


def _launch(src, dsts, mats, stream=None):
    arr, n = capi.make_images(src.entries(dsts.pairs()))
    capi.resize_crop_batch_color(arr, capi.make_colors(mats), n, dsts.dtype(), dsts.fmt(), 0,
                                 stream.handle if stream else None)
    if stream:
        stream.synchronize()


def _check(src, plain, mats, mode, tag, **kw):
    dsts = Dsts(src.geoms, mode, **kw)
    try:
        dsts.clear()
        _launch(src, dsts, mats)
        capi.check(capi.lib().mxd_device_synchronize(0))
        outs, clean = dsts.read()
    finally:
        dsts.free()
    for k, (o, q, m, ok) in enumerate(zip(outs, plain, mats, clean)):
        e = _expected(mode, q, m)
        assert o.shape == e.shape and o.dtype == e.dtype, (tag, mode[0], k)
        bad = int((o != e).sum())
        assert bad == 0, (tag, mode[0], k, bad, np.argwhere(o != e)[:3])
        assert ok, (tag, mode[0], k, "bytes outside the image were written")
    return outs


# ---- eight device-resident images, every output form ---------------------------------

@pytest.fixture(scope="module")
def eight():
    """97x61 -> 40x36, crop 33x29 at odd origins (a one-pixel tail of the
    four-pixel lanes, rows that are no 16-byte multiple), image 5 mirrored."""
    imgs = [synth(61, 97, 3, 100 + k) for k in range(8)]
    geoms = [(40, 36, 1 + 2 * (k % 3), 3 + 2 * (k % 2), 33, 29, 1 if k == 5 else 0) for k in range(8)]
    src = Sources(imgs, geoms)
    plain = src.plain_u8()
    assert all(p.any() for p in plain)
    yield src, plain
    src.free()


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_eight_images_with_eight_matrices(eight, mode):
    src, plain = eight
    mats = R.eight_matrices()
    assert len({m.tobytes() for m in mats}) == 8
    outs = _check(src, plain, mats, mode, "eight")
    if mode is U8:
        assert np.array_equal(outs[0], plain[0])  # the identity
        assert (outs[1] == 0).any() and (outs[1] == 255).any()  # saturating at both ends
        assert not np.array_equal(outs[5], plain[5])


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_destinations_that_force_element_stores(eight, mode):
    """Bases one element past a 256-byte boundary, dst_stride and plane_stride
    odd multiples of the element size."""
    src, plain = eight
    dsts = Dsts(src.geoms, mode, dst_pad=2, plane_pad=2, dst_shift=1)
    es = dsts.es
    for p, dpitch in dsts.pairs():
        assert p % 256 == es and (dpitch // es) % 2 == 1
    assert not dsts.chw or (dsts.plane // es) % 2 == 1
    dsts.free()
    _check(src, plain, R.eight_matrices()[::-1], mode, "odd", dst_pad=2, plane_pad=2, dst_shift=1)


# ---- every resize route in one call --------------------------------------------------

def _plan_entry(img, g, pitch, filter=0):
    return dict(src_w=img.shape[1], src_h=img.shape[0], src_stride=pitch, channels=3, resize_w=g[0], resize_h=g[1],
                crop_x=g[2], crop_y=g[3], crop_w=g[4], crop_h=g[5], flip=g[6], dst_stride=(g[4] * 3 + 15) // 16 * 16,
                filter=filter)


@pytest.mark.parametrize("policy", [capi.MXD_POLICY_AUTO, capi.MXD_POLICY_PREFER_BAND], ids=["auto", "prefer-band"])
@pytest.mark.parametrize("mode", [U8, FORMATTED[5]], ids=["u8", "bfloat16-chw"])
def test_mixed_routes_keep_each_matrix_with_its_image(mode, policy):
    """A wave image, a Catmull-Rom image, a 680x680 -> 40x40 image (34 taps:
    past every wave bucket and band class, so the planner gives it to the
    general kernel), an image whose source rows are not 4-byte aligned (the
    general kernel) and a 600x600 -> 40x40 image (a wave kernel, or the band
    kernel under MXD_POLICY_PREFER_BAND), with distinct matrices: the launch
    reorders the images by kernel, and a matrix must follow its image."""
    imgs = [synth(150, 200, 3, 1), synth(150, 200, 3, 2), synth(680, 680, 3, 3), synth(99, 101, 3, 4),
            synth(600, 600, 3, 5)]
    geoms = [(120, 90, 7, 3, 101, 80, 0), (120, 90, 7, 3, 101, 80, 1), (40, 40, 0, 0, 40, 40, 0),
             (75, 70, 3, 2, 61, 33, 1), (40, 40, 0, 0, 40, 40, 0)]
    filters = [0, 1, 0, 0, 0]
    src = Sources(imgs, geoms, filters, src_align=[16, 16, 16, 1, 16])
    prev = capi.set_kernel_policy(policy)
    try:
        plans = [capi.describe_plan(_plan_entry(i, g, p, f)) for i, g, p, f in zip(imgs, geoms, src.pitches, filters)]
        bands = [capi.describe_band_plan(_plan_entry(i, g, p, f))["band"]
                 for i, g, p, f in zip(imgs, geoms, src.pitches, filters)]
        assert plans[0]["wave"] == 1 and plans[1]["wave"] == 1 and plans[1]["s"] == 4 and plans[4]["wave"] == 1, plans
        assert plans[2]["wave"] == 0 and plans[3]["wave"] == 0 and bands[2] == 0 and bands[3] == 0, (plans, bands)
        assert bands[4] == 1, bands  # (taken first only under MXD_POLICY_PREFER_BAND)
        plain = src.plain_u8()
        mats = [R.NEGATIVE, R.SWAP, R.IDENTITY, R.CLAMPING, R.to_bytes_units(R.twist_ref(1.1, 1.4, 0.2, 70.0))]
        outs = _check(src, plain, mats, mode, "mixed")
        if mode is U8:
            assert np.array_equal(outs[2], plain[2])
    finally:
        capi.set_kernel_policy(prev)
        src.free()


# ---- the cached descriptor slot ------------------------------------------------------

def test_cached_descriptors_follow_the_matrices_and_the_sources(eight):
    """The same images and destinations twice with different matrices (the
    uploads differ in the matrices only), then different images with the same
    matrices (the same upload: a cache hit that must read the new sources)."""
    src, plain = eight
    mode = FORMATTED[4]  # bfloat16 hwc
    dsts = Dsts(src.geoms, mode)
    stream = capi.Stream(0)
    try:
        a, b = R.eight_matrices(), R.eight_matrices()[3:] + R.eight_matrices()[:3]
        for tag, mats in (("a", a), ("b", b), ("a again", a)):
            dsts.clear()
            _launch(src, dsts, mats, stream)
            for k, (o, q, m) in enumerate(zip(dsts.read()[0], plain, mats)):
                assert np.array_equal(o, _expected(mode, q, m)), (tag, k)
        other = [synth(61, 97, 3, 300 + k) for k in range(8)]
        src.upload(other)
        plain2 = src.plain_u8()
        assert not np.array_equal(plain2[0], plain[0])
        dsts.clear()
        _launch(src, dsts, a, stream)
        for k, (o, q, m) in enumerate(zip(dsts.read()[0], plain2, a)):
            assert np.array_equal(o, _expected(mode, q, m)), ("other images", k)
    finally:
        src.upload(src.images)
        stream.close()
        dsts.free()


# ---- host sources: more than one chunk ------------------------------------------------

@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "page-locked"])
def test_host_sources_spanning_three_chunks(pinned):
    """Nine 1200x1600 images resized to 400x300 whole, as
    test_gpu_host_path.py::test_raw_call_spanning_three_chunks sizes them
    (5,798,400 B staged per image: chunks of 4, 4 and 1), each with its own
    matrix: a chunk's launch must get its slice of the matrices."""
    n, h, w = 9, 1200, 1600
    rng = np.random.default_rng(11)
    L = capi.lib()
    pin = ctypes.c_void_p()
    if pinned:
        capi.check(L.mxd_malloc_pinned(ctypes.byref(pin), ctypes.c_size_t(n * h * w * 3)))
        store = np.ctypeslib.as_array(ctypes.cast(pin, ctypes.POINTER(ctypes.c_uint8)), (n, h, w, 3))
    else:
        store = np.empty((n, h, w, 3), np.uint8)
    small = rng.integers(0, 256, (n, h // 8, w // 8, 3), dtype=np.uint8)
    store[:] = np.repeat(np.repeat(small, 8, axis=1), 8, axis=2)
    geoms = [(400, 300, 0, 0, 400, 300, k % 2) for k in range(n)]
    mats = [R.to_bytes_units(R.twist_ref(0.6 + 0.1 * k, 1.0 + 0.05 * k, 0.3 * k, 20.0 * k)) for k in range(n)]
    mode = FORMATTED[5] if not pinned else U8

    def entries(pairs):
        return [dict(src=store[k].ctypes.data, src_stride=w * 3, src_w=w, src_h=h, channels=3, resize_w=400,
                     resize_h=300, crop_x=0, crop_y=0, crop_w=400, crop_h=300, flip=geoms[k][6], dst=p, dst_stride=dp)
                for k, (p, dp) in enumerate(pairs)]

    plain_d = Dsts(geoms, U8)
    dsts = Dsts(geoms, mode)
    try:
        arr, cnt = capi.make_images(entries(plain_d.pairs()))
        capi.resize_crop_to_device(arr, cnt, capi.MXD_U8, 0)
        plain = plain_d.read()[0]
        dsts.clear()
        arr, cnt = capi.make_images(entries(dsts.pairs()))
        capi.resize_crop_to_device_color(arr, capi.make_colors(mats), cnt, dsts.dtype(), dsts.fmt(), 0)
        outs, clean = dsts.read()
        for k in range(n):
            assert plain[k].any()
            assert np.array_equal(outs[k], _expected(mode, plain[k], mats[k])), k
            assert clean[k], k
    finally:
        plain_d.free()
        dsts.free()
        if pinned:
            del store
            capi.check(L.mxd_free_pinned(pin))


# ---- JPEG sources -----------------------------------------------------------------------

@pytest.mark.parametrize("mode", [U8, F32, FORMATTED[3]], ids=["u8", "f32", "float16-chw"])
def test_jpeg_sources(mode):
    """A 4:2:0 and a 4:4:4 fixture (83x61) and the 300x200 4:2:0 photograph
    (resized straight from its sample planes where the plain call does so)."""
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg.npz"))
    names = ["sub2_prog0_jpg", "sub0_prog0_jpg", "caltech_300x200_jpg"]
    geoms = [(60, 44, 3, 1, 53, 41, 0), (60, 44, 3, 1, 53, 41, 1), (341 * 3 // 4, 171, 11, 5, 224, 160, 0)]
    coefs = [capi.JpegCoefs(gold[k]) for k in names]
    mats = [R.NEGATIVE, R.to_bytes_units(R.twist_ref(1.2, 0.8, 1.5, -40.0)), R.CLAMPING]
    plain_d, dsts = Dsts(geoms, U8), Dsts(geoms, mode)

    def entries(pairs):
        return [dict(coefs=c, resize_w=g[0], resize_h=g[1], crop_x=g[2], crop_y=g[3], crop_w=g[4], crop_h=g[5],
                     flip=g[6], dst=p, dst_stride=dp) for c, g, (p, dp) in zip(coefs, geoms, pairs)]

    try:
        arr, n = capi.make_jpeg_images(entries(plain_d.pairs()))
        capi.jpeg_resize_crop_to_device(arr, n, capi.MXD_U8, 0)
        plain = plain_d.read()[0]
        dsts.clear()
        arr, n = capi.make_jpeg_images(entries(dsts.pairs()))
        capi.jpeg_resize_crop_to_device_color(arr, capi.make_colors(mats), n, dsts.dtype(), dsts.fmt(), 0)
        outs, clean = dsts.read()
        for k in range(n):
            assert plain[k].any()
            assert np.array_equal(outs[k], _expected(mode, plain[k], mats[k])), k
            assert clean[k], k
    finally:
        plain_d.free()
        dsts.free()
        for c in coefs:
            c.close()
