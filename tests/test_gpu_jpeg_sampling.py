"""GPU: the device JPEG decode on every sampling layout (tests/jpeg_layouts.py;
the host side is tests/test_jpeg_sampling.py).  Pillow writes only 4:4:4,
4:2:2 and 4:2:0 (CMYK: 1x1), so before these files the device had only seen
1, 3, 4 or 6 blocks per MCU.  Here:

* csrc/jpeghuff.hip: the block cursor (set / next / advance, block_addr,
  Dec::step's wrap) at 2, 5, 7, 8, 9 and 10 blocks per MCU, four DC
  predictors, scans naming eight distinct Huffman tables, subsequences
  shorter than an MCU (MXD_TUNE_HUFF_BITS = 32: synchronisation lands in
  every block phase), jobs cut inside an image (MXD_TUNE_HUFF_JOB), both word
  sources;
* csrc/jpegdev.hip: sample_at's h1v2 branch, replication by 3 and 4,
  jpeg_color's per-pixel path for mixed modes (luma not full size, Cb and Cr
  with different factors, subsampled YCCK / CMYK);
* csrc/hostjpeg.cpp: jpeg_planes' footprint-to-block range at factors 3 and
  4 (windows), and jpeg_bind_image's plane-source gate, which must stay shut
  for files that look like 4:2:0 and are not YCbCr.

Everything is byte-exact, and the expected bytes always come from the host
decoder (pinned to libjpeg-turbo by the host tests) or the committed fixture
tests/golden/jpeg_sampling.npz, never from the device."""
import functools
import io

import numpy as np
import pytest

import jpeg_layouts as L
from mlx_data_amd import capi

pytestmark = pytest.mark.gpu


def _encode(a, **kw):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(a if a.shape[2] == 3 else a[:, :, 0]).save(b, "JPEG", **kw)
    return b.getvalue()


def _identity(c):
    return (0, 0, c.width, c.height, c.width, c.height, 0, 0, c.width, c.height, 0)


def _gpu(coefs, geoms=None, f32=False, device_dst=False):
    """mxd_jpeg_resize_crop_host / _to_device over coefficient handles;
    geoms default to identity (the decoded image)."""
    if geoms is None:
        geoms = [_identity(c) for c in coefs]
    elem = 4 if f32 else 1
    outs, entries, bufs = [], [], []
    for c, (wx, wy, ww, wh, rw, rh, cx, cy, cw, ch, flip) in zip(coefs, geoms):
        row = cw * 3 * elem
        if device_dst:
            d = capi.DeviceBuffer(row * ch, 0)
            d.memset(0)
            bufs.append((d, row, ch))
            ptr = d.ptr
        else:
            o = np.zeros((ch, row), np.uint8)
            outs.append(o)
            ptr = o.ctypes.data
        entries.append(dict(coefs=c, win_x=wx, win_y=wy, win_w=ww, win_h=wh, resize_w=rw, resize_h=rh, crop_x=cx,
                            crop_y=cy, crop_w=cw, crop_h=ch, flip=flip, dst=ptr, dst_stride=row))
    arr, n = capi.make_jpeg_images(entries)
    dt = capi.MXD_F32_DIV255 if f32 else capi.MXD_U8
    if device_dst:
        capi.jpeg_resize_crop_to_device(arr, n, dt, 0)
        for d, row, ch in bufs:
            outs.append(d.download((ch, row), np.uint8))
            d.free()
    else:
        capi.jpeg_resize_crop_host(arr, n, dt, 0)
    return outs


def _host_ref(pixels, geoms, f32):
    """mxd_resize_crop_host on host-decoded pixels: the expected bytes."""
    elem = 4 if f32 else 1
    outs, entries, keep = [], [], []
    for im, (wx, wy, ww, wh, rw, rh, cx, cy, cw, ch, flip) in zip(pixels, geoms):
        win = np.ascontiguousarray(im[wy:wy + wh, wx:wx + ww])
        o = np.zeros((ch, cw * 3 * elem), np.uint8)
        outs.append(o)
        keep.append(win)
        entries.append(dict(src=win.ctypes.data, src_stride=ww * 3, src_w=ww, src_h=wh, channels=3, resize_w=rw,
                            resize_h=rh, crop_x=cx, crop_y=cy, crop_w=cw, crop_h=ch, flip=flip, dst=o.ctypes.data,
                            dst_stride=cw * 3 * elem))
    arr, n = capi.make_images(entries)
    capi.resize_crop_host(arr, n, capi.MXD_F32_DIV255 if f32 else capi.MXD_U8, 0)
    return outs


@functools.lru_cache(maxsize=None)
def _files():
    """(id, file, expected pixels, fixture pixels or None): every layout x
    size x restart interval, then the committed fixture's files.  The
    expected pixels are the host decoder's, computed once."""
    out = [(c.id, c.data, capi.jpeg_decode(c.data), None) for c in L.cases()]
    out += [("golden_" + k, d, capi.jpeg_decode(d), rgb) for k, d, rgb in L.golden()]
    return out


def _check(files, coefs, got):
    assert len(got) == len(files) == len(coefs)
    for (name, _, want, gold), g, c in zip(files, got, coefs):
        img = g.reshape(c.height, c.width, 3)
        assert np.array_equal(img, want), name
        if gold is not None:
            assert np.array_equal(img, gold), name


def _identity_in_two_calls(files, device_entropy):
    half = len(files) // 2
    for part in (files[:half], files[half:]):
        coefs = [capi.JpegCoefs(d, device_entropy=device_entropy) for _, d, _, _ in part]
        assert all(c.device_ok for c in coefs)
        if device_entropy:
            pending = [c.entropy_pending for c in coefs]
            assert all(pending), part[pending.index(False)][0]
        else:
            assert not any(c.entropy_pending for c in coefs)
        _check(part, coefs, _gpu(coefs))


@pytest.fixture(params=[0, 1], ids=["lds_words", "global_words"])
def word_source(request):
    prev = capi.set_tuning(capi.MXD_TUNE_HUFF_GLOBAL, request.param)
    yield request.param
    capi.set_tuning(capi.MXD_TUNE_HUFF_GLOBAL, prev)


@pytest.mark.parametrize("bits", [0, 32, 96], ids=["default_bits", "32_bits", "96_bits"])
def test_identity_device_entropy(bits, word_source):
    """Every layout x size x restart interval and the fixture files, Huffman
    decode on the device.  32-bit subsequences are shorter than one MCU of any
    layout here, so subsequences start in every block of the MCU."""
    prev = capi.set_tuning(capi.MXD_TUNE_HUFF_BITS, bits)
    try:
        _identity_in_two_calls(_files(), True)
    finally:
        capi.set_tuning(capi.MXD_TUNE_HUFF_BITS, prev)


def test_identity_jobs_cut_inside_the_image(word_source):
    """MXD_TUNE_HUFF_JOB = 8 with 96-bit subsequences: every 100x129 file is
    more than 8 subsequences per restart interval or in all, so its jobs are
    cut inside segments and take their start state (block of the MCU
    included) from the job before."""
    files = [f for f, c in zip(_files(), L.cases()) if (c.w, c.h) == (100, 129)]
    assert len(files) == len(L.LAYOUTS) * len(L.RESTARTS)
    for c, (_, d, _, _) in zip([c for c in L.cases() if (c.w, c.h) == (100, 129)], files):
        if c.restart == 0:  # one segment of more than three jobs' subsequences
            assert (len(d) - d.find(b"\xff\xda")) * 8 > 3 * 8 * 96, c.id
    prev = capi.set_tuning(capi.MXD_TUNE_HUFF_BITS, 96), capi.set_tuning(capi.MXD_TUNE_HUFF_JOB, 8)
    try:
        coefs = [capi.JpegCoefs(d, device_entropy=True) for _, d, _, _ in files]
        assert all(c.entropy_pending for c in coefs)
        _check(files, coefs, _gpu(coefs))
    finally:
        capi.set_tuning(capi.MXD_TUNE_HUFF_BITS, prev[0])
        capi.set_tuning(capi.MXD_TUNE_HUFF_JOB, prev[1])


def test_identity_host_decoded_coefficients():
    """The same files entropy-decoded on the host (natural-order coefficient
    planes): the device's IDCT, upsampling and colour step alone."""
    _identity_in_two_calls(_files(), False)


def test_mixed_batch_with_ordinary_files():
    """The layouts between ordinary Pillow 4:2:0 / 4:4:4 / grey files in one
    call: blocks per MCU, table sets and upsampling modes change from image
    to image inside one launch."""
    rng = np.random.default_rng(61)
    files = []
    picked = [f for f, c in zip(_files(), L.cases()) if (c.w, c.h) in ((61, 83), (17, 2), (2, 17)) and c.restart != 1]
    for i, f in enumerate(picked):
        files.append(f)
        if i % 2 == 0:
            h, w = int(rng.integers(1, 130)), int(rng.integers(1, 130))
            grey = i % 6 == 4
            kw = dict(quality=int(rng.integers(40, 100)))
            if not grey:
                kw["subsampling"] = (0, 2)[i // 2 % 2]
            if i % 10 == 0:
                kw["restart_marker_blocks"] = 2
            d = _encode(L.smooth(rng, h, w, 1 if grey else 3), **kw)
            files.append((f"pillow_{i}", d, capi.jpeg_decode(d), L.pillow_pixels(d)))
    coefs = [capi.JpegCoefs(d, device_entropy=True) for _, d, _, _ in files]
    assert all(c.device_ok and c.entropy_pending for c in coefs)
    _check(files, coefs, _gpu(coefs))


def _windows(rng, w, h):
    """Windows of a w x h image: the four corners, the same one pixel inside
    each edge, the whole image less its outermost pixels, two random ones."""
    s, t = int(rng.integers(8, 25)), int(rng.integers(8, 25))
    out = [(0, 0, s, t), (w - s, 0, s, t), (0, h - t, s, t), (w - s, h - t, s, t),
           (1, 1, s, t), (w - 1 - s, 1, s, t), (1, h - 1 - t, s, t), (w - 1 - s, h - 1 - t, s, t),
           (1, 1, w - 2, h - 2)]
    for _ in range(2):
        ww, wh = int(rng.integers(8, w + 1)), int(rng.integers(8, h + 1))
        out.append((int(rng.integers(0, w - ww + 1)), int(rng.integers(0, h - wh + 1)), ww, wh))
    return out


@pytest.mark.parametrize("variant,f32,device_dst", [(0, False, False), (1, True, False), (2, False, True),
                                                    (3, True, True)], ids=["u8", "f32", "u8_device", "f32_device"])
def test_windows_resize_crop_flip(variant, f32, device_dst):
    """Resize + crop + mirror of windows of the 61x83 and 100x129 files equal
    mxd_resize_crop_host on the host-decoded pixels.  Only the blocks under a
    window's footprint are decoded (hostjpeg.cpp jpeg_planes), so a range too
    small by one shows as stale samples.  The pictures are this variant's own
    (their seed), never decoded whole on the device, and every window has its
    own planes in the call: nothing an earlier decode left in the staging
    buffers can stand in for a block that was not decoded."""
    rng = np.random.default_rng(900 + variant)
    datas, pixels, index, geoms = [], [], [], []
    for li, (name, sampling, adobe) in enumerate(L.LAYOUTS):
        for si, (w, h) in enumerate([(61, 83), (100, 129)]):
            d = L.write(L.image(name, w, h, seed=1000 + variant), sampling, adobe, L.RESTARTS[(li + si + variant) % 3],
                        distinct=(li + si) % 2 == 1)
            datas.append(d)
            pixels.append(capi.jpeg_decode(d))
            for k, (wx, wy, ww, wh) in enumerate(_windows(rng, w, h)):
                rw, rh = int(rng.integers(16, 65)), int(rng.integers(16, 65))
                cw, ch = int(rng.integers(1, rw + 1)), int(rng.integers(1, rh + 1))
                cx, cy = int(rng.integers(0, rw - cw + 1)), int(rng.integers(0, rh - ch + 1))
                index.append(len(datas) - 1)
                geoms.append((wx, wy, ww, wh, rw, rh, cx, cy, cw, ch, (k + li) % 2))
    # host-decoded coefficients in every third image: the same block ranges on natural-order planes
    handles = [capi.JpegCoefs(d, device_entropy=i % 3 != 2) for i, d in enumerate(datas)]
    assert all(c.entropy_pending == (i % 3 != 2) for i, c in enumerate(handles))
    want = _host_ref([pixels[i] for i in index], geoms, f32)
    got = _gpu([handles[i] for i in index], geoms, f32, device_dst)
    for n, (g, w_) in enumerate(zip(got, want)):
        assert np.array_equal(g, w_), (L.LAYOUTS[index[n] // 2][0], geoms[n])


def test_plane_source_gate_stays_shut_for_what_is_not_ycbcr_420():
    """jpeg_bind_image resizes true 4:2:0 YCbCr straight from the sample
    planes.  Files that share its factors in the first three components but
    are YCCK, CMYK or RGB as stored (Adobe transform 2 / 0), and the layout
    with luma subsampled, must take the RGB frame: the counter stays 0 and
    the bytes equal the host reference, at the geometry that takes the plane
    source for real 4:2:0 (smallest side to 64, centre crop) -- which the true
    4:2:0 files of the same encoder in the same call show: they are counted."""
    names = {"c4_22111122_ycck", "c4_22111122_cmyk", "c4_22111111_ycck", "c4_22111111_cmyk", "c3_lumasub_ycc",
             "c3_lumasub_rgb"}
    sizes = [(100, 129), (129, 100), (61, 83), (128, 128)]
    closed, opened = [], []
    for name, sampling, adobe in L.LAYOUTS:
        if name in names:
            closed += [L.write(L.image(name, w, h, seed=50), sampling, adobe, r) for (w, h), r in zip(sizes, (0, 3, 1, 0))]
    s420 = [(2, 2), (1, 1), (1, 1)]
    closed += [L.write(L.image("c3_420_rgb", w, h, seed=50), s420, 0, r) for (w, h), r in zip(sizes, (3, 0, 0, 1))]
    opened += [L.write(L.image("c3_420_ycc", w, h, seed=50), s420, None, r) for (w, h), r in zip(sizes, (0, 1, 3, 0))]
    assert len(closed) == 7 * 4

    def run(datas):
        coefs = [capi.JpegCoefs(d, device_entropy=True) for d in datas]
        assert all(c.device_ok and c.entropy_pending for c in coefs)
        geoms = []
        for i, c in enumerate(coefs):
            rw, rh = capi.resize_smallest_side_dims(c.width, c.height, 64)
            cw, ch = min(rw, 56), min(rh, 56)
            cx, cy = capi.center_crop_origin(rw, rh, cw, ch)
            geoms.append((0, 0, c.width, c.height, rw, rh, cx, cy, cw, ch, i % 2))
        for f32 in (False, True):
            want = _host_ref([capi.jpeg_decode(d) for d in datas], geoms, f32)
            for i, (g, w_) in enumerate(zip(_gpu(coefs, geoms, f32), want)):
                assert np.array_equal(g, w_), (i, f32)

    capi.jpeg_plane_sources(reset=True)
    run(closed)
    assert capi.jpeg_plane_sources(reset=True) == 0
    # one call with both: only the true 4:2:0 files are counted (twice: u8 and f32)
    run(closed[::3] + opened + closed[1::3])
    n = capi.jpeg_plane_sources(reset=True)
    assert 1 <= n <= 2 * len(opened), n


@pytest.mark.parametrize("to_float", [False, True], ids=["u8", "f32"])
def test_operator_surface_device_decode_on_off(to_float, tmp_path):
    """load_image -> image_resize -> image_center_crop -> batch(8) over files
    of these layouts on disk: the batches with the device decode on equal
    those with it off (the host decoder)."""
    from mlx_data_amd import data as dx

    picked = [c for c in L.cases() if (c.w, c.h) in ((61, 83), (100, 129)) and c.restart == (0, 1, 3)[len(c.name) % 3]]
    picked = picked[::6] + picked[-1:]
    assert len(picked) == 16 and {c.ncomp for c in picked} == {1, 3, 4}
    samples = []
    for i, c in enumerate(picked):
        (tmp_path / f"{i}.jpg").write_bytes(c.data)
        samples.append(dict(image=str(tmp_path / f"{i}.jpg").encode(), label=i))

    def run(on):
        before = dx.device_decode()
        dx.set_device_decode(on)
        try:
            d = dx.buffer_from_vector(samples).load_image("image").image_resize("image", 72, 60).image_center_crop(
                "image", 48, 40)
            d = d.image_to_float("image") if to_float else d
            d = d.batch(8)
            return [np.asarray(d[i]["image"]) for i in range(len(d))]
        finally:
            dx.set_device_decode(before)

    on, off = run(True), run(False)
    assert len(on) == len(off) == 2
    for a, b in zip(on, off):
        assert a.shape == b.shape and a.shape[0] == 8 and a.dtype == b.dtype and np.array_equal(a, b)
