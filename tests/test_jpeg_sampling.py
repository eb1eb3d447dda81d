"""The host JPEG decoder on every sampling layout (tests/jpeg_layouts.py): the
integral layouts up to 10 blocks per MCU that Pillow's encoder cannot write --
4:4:0, 4:1:1, 4:1:0, factors of 3 and 4, components with different factors,
subsampled luma, subsampled CMYK / YCCK with K among or below the maxima,
one-component files with any factors -- written by tests/jpeg_enc.py, at the
sizes where the upsamplers change path, with and without restart intervals,
with one table set and with tables of their own per component.

* bit-exact to libjpeg-turbo through Pillow, live and through the committed
  fixture tests/golden/jpeg_sampling.npz (generator
  make_jpeg_sampling_golden.py), by all three host routes: jpeg_decode, the
  coefficient handle decoded on the host, and the markers-only handle the
  device would entropy-decode (every layout qualifies) finished on the host;
* what libjpeg refuses is refused with its message by every entry point:
  more than 10 blocks in an interleaved MCU, and a factor that does not divide
  the largest in any component, a CMYK file's K included;
* the encoder's default output is what it was before it learnt sampling."""
import hashlib

import numpy as np
import pytest

import jpeg_enc as J
import jpeg_layouts as L
from mlx_data_amd import capi


def test_encoder_defaults_are_byte_identical():
    """SHA-256 of the encoder's output before `sampling` / `tables` existed
    (one grey, one three-component file with restarts and an Adobe marker),
    and the explicit spelling of the defaults gives the same bytes."""
    rng = np.random.default_rng(2024)
    g = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    c = rng.integers(0, 256, (29, 43, 3), dtype=np.uint8)
    dg, dc = J.encode(g), J.encode(c, q=3, restart_mcus=4, adobe=0)
    assert hashlib.sha256(dg).hexdigest() == "adc0f6cd75d1295bdcc49f942ff812c1b283f332800a6b04c792b209597a4f68"
    assert hashlib.sha256(dc).hexdigest() == "f6a8cb8b76e2016efa09d191a843f5b99845b8639777ece1a7a68c40ccabe731"
    assert hashlib.sha256(J.encode_lossless(c, psv=4)).hexdigest() == \
        "931a50f5b18646aed51ebb32b6e8b9c07606892706cf3838496caad375316c9f"
    assert J.encode(g, sampling=[(1, 1)]) == dg
    assert J.encode(c, q=[3], dc=[J.DEEP_DC], ac=[J.DEEP_AC], restart_mcus=4, adobe=0, sampling=[(1, 1)] * 3,
                    tables=[(0, 0, 0)] * 3) == dc


def test_layout_list_is_what_it_claims():
    """Every blocks-per-MCU count from 2 to 10 occurs, every file's factors
    are integral, and files with eight distinct Huffman tables exist."""
    assert len(L.LAYOUTS) == 2 * 11 + 2 * 8 + 5 and len(L.cases()) == len(L.LAYOUTS) * 6 * 3
    assert {L.blocks_per_mcu(s) for _, s, _ in L.LAYOUTS} >= set(range(4, 11)) | {1}
    for _, s, _ in L.LAYOUTS:
        mh, mv = max(h for h, _ in s), max(v for _, v in s)
        assert all(mh % h == 0 and mv % v == 0 for h, v in s) and L.blocks_per_mcu(s) <= 10
    for nc in (1, 3, 4):
        assert any(c.distinct and c.ncomp == nc for c in L.cases())
    for t in J.DC_TABLES + J.AC_TABLES:  # complete, and pairwise distinct
        assert sum(t[0]) == len(t[1]) == len(set(t[1]))
    assert len({str(t) for t in J.DC_TABLES}) == 4 and len({str(t) for t in J.AC_TABLES}) == 4


def test_every_layout_decodes_like_libjpeg():
    pytest.importorskip("PIL.Image")
    for c in L.cases():
        want = L.pillow_pixels(c.data)
        assert want.shape == (c.h, c.w, 3), c.id
        assert np.array_equal(capi.jpeg_decode(c.data), want), c.id
        k = capi.JpegCoefs(c.data, device_entropy=True)
        assert k.device_ok and k.entropy_pending, c.id  # the device route takes every one of them
        assert (k.width, k.height) == (c.w, c.h)
        assert np.array_equal(k.finish(), want), c.id
        k = capi.JpegCoefs(c.data)
        assert k.device_ok and not k.entropy_pending, c.id
        assert np.array_equal(k.finish(), want), c.id


def test_committed_fixture_pins_the_host_decoder():
    gold = L.golden()
    assert len(gold) == len(L.LAYOUTS) * len(L.GOLDEN_SIZES)
    for key, data, rgb in gold:
        assert np.array_equal(capi.jpeg_decode(data), rgb), key
        assert np.array_equal(capi.JpegCoefs(data, device_entropy=True).finish(), rgb), key
        assert np.array_equal(capi.JpegCoefs(data).finish(), rgb), key


def test_fixture_matches_the_installed_libjpeg():
    pytest.importorskip("PIL.Image")
    for key, data, rgb in L.golden():
        assert np.array_equal(L.pillow_pixels(data), rgb), key


def test_what_libjpeg_refuses_is_refused_with_its_message(tmp_path):
    """More than 10 blocks per interleaved MCU (jdinput.c per_scan_setup) and
    fractional factors in any component (jdsample.c jinit_upsampler checks
    all of them, a CMYK file's K too): libjpeg's message from jpeg_decode,
    from both kinds of coefficient handle and from load_image (memory and
    file, host decode and deferred device decode).  Pillow refuses them too."""
    Image = pytest.importorskip("PIL.Image")
    import io
    import re

    from mlx_data_amd import data as dx

    files = L.refused_files()
    assert {m for _, m, _ in files} == {L.TOO_LARGE, L.FRACTIONAL}
    # the MCU size is checked when any interleaved scan is set up: progressive and
    # arithmetic-coded 4:4:4 files with their frame's factors overwritten by 2x2 (12 blocks)
    import jpeg_arith_enc as A

    px = L.image("c3_patched", 24, 24)
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, "JPEG", progressive=True, subsampling=0)
    for name, d, sof in [("progressive", buf.getvalue(), 0xC2), ("arithmetic", A.encode(px, q=3), 0xC9),
                         ("arithmetic_progressive", A.encode_progressive(px, q=3), 0xCA)]:
        at = d.index(bytes([0xFF, sof]))
        d = bytearray(d)
        assert d[at + 9] == 3 and [d[at + 11 + 3 * i] for i in range(3)] == [0x11] * 3
        for i in range(3):
            d[at + 11 + 3 * i] = 0x22
        files.append((name + "_12_blocks", L.TOO_LARGE, bytes(d)))
    before = dx.device_decode()
    try:
        for name, msg, d in files:
            with pytest.raises(Exception):
                Image.open(io.BytesIO(d)).load()
            with pytest.raises(capi.MxdError, match=msg):
                capi.jpeg_decode(d)
            with pytest.raises(capi.MxdError, match=msg):
                capi.JpegCoefs(d)
            with pytest.raises(capi.MxdError, match=msg):
                capi.JpegCoefs(d, device_entropy=True)
            (tmp_path / f"{name}.jpg").write_bytes(d)
            for entropy in (False, True):
                with pytest.raises(capi.MxdError, match=msg):
                    capi.JpegCoefs.load(str(tmp_path / f"{name}.jpg"), device_entropy=entropy)
            b = dx.buffer_from_vector([dict(f=f"{name}.jpg".encode(), m=np.frombuffer(d, np.uint8))])
            for on in (False, True):
                dx.set_device_decode(on)
                with pytest.raises(RuntimeError, match=r"load_jpeg: could not load from memory \(" + re.escape(msg)):
                    b.load_image("m", from_memory=True)[0]
                with pytest.raises(RuntimeError, match=r"load_jpeg: could not load <.*> \(" + re.escape(msg)):
                    b.load_image("f", prefix=str(tmp_path))[0]
    finally:
        dx.set_device_decode(before)
