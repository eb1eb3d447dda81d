"""MixUp and CutMix on the CPU (no device): the CPU statement of the C ABI
(mxd_mix_apply_u8) byte-equal to timm's NumPy expression (tests/mix_ref.py) on
every byte pair, CutMix boxes at every edge, the refusals of the C ABI with
their messages, the header and the exported symbols.  (The layout of a mix
call: tests/test_mix_chain.py.)"""
import ctypes
import os

import numpy as np
import pytest

import mix_ref as M
from mlx_data_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the CPU statement against the NumPy expression -----------------------------------------

def _variants(q, r, lam):
    """What other arithmetic would give: a fused multiply-add, half-up rounding, double arithmetic."""
    q64, r64 = q.astype(np.float64), r.astype(np.float64)
    ws, wo = np.float64(np.float32(lam)), np.float64(np.float32(1.0 - lam))
    prod = (r.astype(np.float32) * np.float32(1.0 - lam)).astype(np.float64)
    fused = np.rint((q64 * ws + prod).astype(np.float32)).astype(np.uint8)  # one rounding of q * ws + (r * wo)
    x = q.astype(np.float32) * np.float32(lam) + r.astype(np.float32) * np.float32(1.0 - lam)
    half_up = np.floor(x + np.float32(0.5)).astype(np.uint8)
    double = np.rint(q64 * lam + r64 * (1.0 - lam)).astype(np.uint8)
    return fused, half_up, double


@pytest.mark.parametrize("lam", [0, 0.3, 0.5, 1])
def test_apply_u8_equals_numpy_on_every_byte_pair(lam):
    q, r = M.byte_pair_grid()
    want = M.mixup(q, r, lam)
    got = capi.mix_apply_u8(q, r, M.entry_mixup(0, lam))
    assert np.array_equal(got, want), int((got != want).sum())
    # the two values that pin the contract: none of the cheaper arithmetics passes both
    fused, half_up, double = _variants(q[:, :, 0], r[:, :, 0], lam)
    w = want[:, :, 0]
    if lam == 0.3:
        assert (int((fused != w).sum()), int((half_up != w).sum()), int((double != w).sum())) == (153, 3133, 777)
    if lam == 0.5:
        assert int((half_up != w).sum()) == 16384
    if lam == 1:
        assert np.array_equal(got, q)
    if lam == 0:
        assert np.array_equal(got, r)


def test_apply_u8_takes_strided_images_and_writes_in_place():
    rng = np.random.default_rng(5)
    h, w = 7, 13
    a, b = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    wide_a, wide_b = np.full((h, w + 3, 3), 0xEE, np.uint8), np.full((h, w + 6, 3), 0xCC, np.uint8)
    wide_a[:, 1:w + 1], wide_b[:, 4:w + 4] = a, b
    out = np.full((h, w + 5, 3), 0xDD, np.uint8)
    for entry, want in ((M.entry_mixup(0, 0.3), M.mixup(a, b, 0.3)), (M.entry_cutmix(0, 2, 1, 9, 6), M.cutmix(a, b, 2, 1, 9, 6)),
                        ((M.NONE,), a)):
        out[:] = 0xDD
        capi.mix_apply_u8(wide_a[:, 1:w + 1], wide_b[:, 4:w + 4], entry, out[:, 2:w + 2])
        assert np.array_equal(out[:, 2:w + 2], want), entry
        assert (out[:, :2] == 0xDD).all() and (out[:, w + 2:] == 0xDD).all()
        own = a.copy()
        capi.mix_apply_u8(own, b, entry, own)  # out may be own
        assert np.array_equal(own, want), entry
    assert np.array_equal(capi.mix_apply_u8(a, None, (M.NONE,)), a)
    # its own partner: the arithmetic as written, no special case
    assert np.array_equal(capi.mix_apply_u8(a, a, M.entry_mixup(0, 0.3)), M.mixup(a, a, 0.3))


BOXES = {  # on a 9 x 6 (w x h) window
    "empty": (4, 2, 4, 5), "empty rows": (1, 3, 8, 3), "full": (0, 0, 9, 6), "one pixel": (5, 3, 6, 4),
    "left edge": (0, 1, 3, 4), "right edge": (6, 2, 9, 5), "top edge": (2, 0, 7, 2), "bottom edge": (1, 4, 5, 6),
    "corner pixel": (8, 5, 9, 6),
}


@pytest.mark.parametrize("name", list(BOXES))
def test_cutmix_boxes(name):
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, 128, (6, 9, 3), dtype=np.uint8), rng.integers(128, 256, (6, 9, 3), dtype=np.uint8)
    x0, y0, x1, y1 = BOXES[name]
    got = capi.mix_apply_u8(a, b, M.entry_cutmix(0, x0, y0, x1, y1))
    assert np.array_equal(got, M.cutmix(a, b, x0, y0, x1, y1))
    assert int((got >= 128).all(axis=2).sum()) == (x1 - x0) * (y1 - y0)
    if name == "full":
        assert np.array_equal(got, b)
    if name.startswith("empty"):
        assert np.array_equal(got, a)


# ---- refusals ----------------------------------------------------------------------------

def _entry(**kw):
    e = dict(src=4096, dst=4096, src_stride=64 * 3, src_w=64, src_h=64, channels=3, resize_w=32, resize_h=32, crop_x=0,
             crop_y=0, crop_w=32, crop_h=32, dst_stride=32 * 3 * 4)
    e.update(kw)
    return e


def _calls(arr, mixes, n, out_dtype=capi.MXD_U8, fmt=None, warps=None, enhances=None, tones=None, colors=None):
    """The status of the two calls that take mxd_image and of mxd_mix_validate, and the last message."""
    L = capi.lib()
    f = ctypes.byref(fmt) if fmt is not None else None
    rcs = (L.mxd_resize_crop_batch_mix(arr, warps, enhances, tones, colors, mixes, n, out_dtype, f, 0, None),
           L.mxd_resize_crop_to_device_mix(arr, warps, enhances, tones, colors, mixes, n, out_dtype, f, 0))
    return rcs, L.mxd_last_error().decode()


def _reserved(k):
    m = capi.MxdMix()
    m.op, m.partner, m.w_self, m.w_other = M.MIXUP, 0, 0.5, 0.5
    m.reserved[k] = 1
    return m


NAN, INF = float("nan"), float("inf")
W_SELF, W_OTHER = "w_self must be finite and in 0..1", "w_other must be finite and in 0..1"
BAD_MIXES = [  # as image 1 of two 32 x 32 images
    ((3, 0), "unknown op 3"), ((-1, 0), "unknown op -1"),
    ((M.MIXUP, 2, 0.5, 0.5), "partner 2 outside 0..1"), ((M.CUTMIX, -1, 0, 0, 1, 1), "partner -1 outside 0..1"),
    ((M.MIXUP, 0, -0.1, 0.5), W_SELF), ((M.MIXUP, 0, 1.5, 0.5), W_SELF), ((M.MIXUP, 0, NAN, 0.5), W_SELF),
    ((M.MIXUP, 0, 0.5, INF), W_OTHER), ((M.MIXUP, 0, 0.5, -1e-9), W_OTHER), ((M.MIXUP, 0, 0.5, NAN), W_OTHER),
    ((M.CUTMIX, 0, -1, 0, 4, 4), "box needs 0 <= x0 <= x1 <= crop_w, got x0 -1 x1 4 crop_w 32"),
    ((M.CUTMIX, 0, 5, 0, 4, 4), "box needs 0 <= x0 <= x1 <= crop_w, got x0 5 x1 4 crop_w 32"),
    ((M.CUTMIX, 0, 0, 0, 33, 4), "box needs 0 <= x0 <= x1 <= crop_w, got x0 0 x1 33 crop_w 32"),
    ((M.CUTMIX, 0, 0, -2, 4, 4), "box needs 0 <= y0 <= y1 <= crop_h, got y0 -2 y1 4 crop_h 32"),
    ((M.CUTMIX, 0, 0, 9, 4, 8), "box needs 0 <= y0 <= y1 <= crop_h, got y0 9 y1 8 crop_h 32"),
    ((M.CUTMIX, 0, 0, 0, 4, 40), "box needs 0 <= y0 <= y1 <= crop_h, got y0 0 y1 40 crop_h 32"),
    (_reserved(0), "reserved must be 0"), (_reserved(1), "reserved must be 0"),
]


def test_call_refusals_name_the_image_and_the_field():
    import enhance_ref
    import tone_ref

    L = capi.lib()
    bad = (capi.MXD_ERR_INVALID,) * 2
    arr, n = capi.make_images([_entry(), _entry()])
    good = capi.make_mixes([M.entry_mixup(1, 0.3), M.entry_cutmix(0, 0, 0, 32, 32)])
    assert L.mxd_mix_validate(arr, good, n) == capi.MXD_OK
    rcs, msg = _calls(arr, None, n)
    assert rcs == bad and msg == "mxd: null mixes"
    assert L.mxd_mix_validate(arr, None, n) == capi.MXD_ERR_INVALID and L.mxd_last_error() == b"mxd: null mixes"
    for m, what in BAD_MIXES:
        mixes = capi.make_mixes([(M.NONE,), m])
        rcs, msg = _calls(arr, mixes, n)
        assert rcs == bad, (what, rcs)
        assert msg == f"mxd_mix: {what} (image 1)", msg
        assert L.mxd_mix_validate(arr, mixes, n) == capi.MXD_ERR_INVALID
        assert L.mxd_last_error().decode() == f"mxd_mix: {what} (image 1)"
    # a partner of another size, in either dimension
    for kw, size in ((dict(crop_w=31), "31 x 32"), (dict(crop_h=30), "32 x 30")):
        arr2, _ = capi.make_images([_entry(**kw), _entry()])
        rcs, msg = _calls(arr2, capi.make_mixes([(M.NONE,), M.entry_mixup(0, 0.5)]), n)
        assert rcs == bad and msg == f"mxd_mix: partner 0's crop size {size} differs from 32 x 32 (image 1)", msg
        # (NONE reads no partner, and an image nobody mixes with may have any size)
        assert L.mxd_mix_validate(arr2, capi.make_mixes([(M.NONE, 1), (M.NONE, 7)]), n) == capi.MXD_OK
    # MXD_MIX_NONE reads nothing but op and reserved
    none = capi.MxdMix()
    none.partner, none.w_self, none.w_other, none.x0, none.x1 = 99, NAN, -3.0, 50, -50
    assert L.mxd_mix_validate(arr, capi.make_mixes([none, none]), n) == capi.MXD_OK
    # its own partner is allowed
    assert L.mxd_mix_validate(arr, capi.make_mixes([M.entry_mixup(0, 0.3), M.entry_cutmix(1, 1, 1, 2, 2)]), n) == capi.MXD_OK
    # without images: the entries alone
    assert L.mxd_mix_validate(None, capi.make_mixes([M.entry_cutmix(1, 0, 0, 999, 999), M.entry_mixup(0, 1.0)]), n) == capi.MXD_OK
    assert L.mxd_mix_validate(None, capi.make_mixes([M.entry_cutmix(1, 3, 0, 2, 9)]), 1) == capi.MXD_ERR_INVALID
    assert L.mxd_last_error() == b"mxd_mix: box needs 0 <= x0 <= x1 <= crop_w, got x0 3 x1 2 (image 0)"
    arr4, _ = capi.make_images([_entry(), _entry(channels=4, src_stride=256)])
    rcs, msg = _calls(arr4, good, n)
    assert rcs == bad and msg == "mxd_mix: channels must be 3 (image 1)", msg
    # the other members' checks when there are some, and the output form's
    rcs, msg = _calls(arr, good, n, enhances=capi.make_enhances([(enhance_ref.NONE, 0.0), (5, 1.0)]))
    assert rcs == bad and msg == "mxd_enhance: unknown op 5 (image 1)", msg
    rcs, msg = _calls(arr, good, n, tones=capi.make_tones([(tone_ref.EQUALIZE, 0, 0.0), (tone_ref.POSTERIZE, 9, 0.0)]))
    assert rcs == bad and "posterize bits" in msg and "(image 1)" in msg, msg
    rcs, msg = _calls(arr, good, n, out_dtype=7)
    assert rcs == bad and msg == "mxd: bad out_dtype"
    rcs, msg = _calls(arr, good, n, fmt=capi.make_out_format(elem=9))
    assert rcs == bad and "unknown elem" in msg
    # an empty call is one
    assert L.mxd_resize_crop_to_device_mix(arr, None, None, None, None, None, 0, capi.MXD_U8, None, 0) == capi.MXD_OK


def test_jpeg_call_and_cpu_statement_refusals():
    gold = np.load(os.path.join(HERE, "golden", "jpeg.npz"))
    coefs = capi.JpegCoefs(gold["caltech_300x200_jpg"])
    L = capi.lib()
    try:
        arr, n = capi.make_jpeg_images([dict(coefs=coefs, resize_w=150, resize_h=100, crop_x=0, crop_y=0, crop_w=150,
                                             crop_h=100, dst=4096, dst_stride=450)])
        assert L.mxd_jpeg_resize_crop_to_device_mix(arr, None, None, None, None, None, n, capi.MXD_U8, None,
                                                    0) == capi.MXD_ERR_INVALID
        assert L.mxd_last_error() == b"mxd: null mixes"
        assert L.mxd_jpeg_resize_crop_to_device_mix(arr, None, None, None, None, capi.make_mixes([(M.MIXUP, 1, 0.5, 0.5)]),
                                                    n, capi.MXD_U8, None, 0) == capi.MXD_ERR_INVALID
        assert L.mxd_last_error() == b"mxd_mix: partner 1 outside 0..0 (image 0)"
        assert L.mxd_jpeg_resize_crop_to_device_mix(arr, None, None, None, None,
                                                    capi.make_mixes([M.entry_cutmix(0, 0, 0, 151, 100)]), n, capi.MXD_U8,
                                                    None, 0) == capi.MXD_ERR_INVALID
        assert L.mxd_last_error() == b"mxd_mix: box needs 0 <= x0 <= x1 <= crop_w, got x0 0 x1 151 crop_w 150 (image 0)"
    finally:
        coefs.close()
    px, other, out = (np.zeros((4, 4, 3), np.uint8) for _ in range(3))
    p, r, o = (ctypes.c_void_p(a.ctypes.data) for a in (px, other, out))
    ok = capi.make_mixes([M.entry_mixup(0, 0.3)])
    s12, s11 = ctypes.c_int64(12), ctypes.c_int64(11)
    assert L.mxd_mix_apply_u8(p, s12, r, s12, 4, 4, None, o, s12) == capi.MXD_ERR_INVALID
    assert L.mxd_last_error() == b"mxd: null mixes"
    assert L.mxd_mix_apply_u8(None, s12, r, s12, 4, 4, ok, o, s12) == capi.MXD_ERR_INVALID
    assert L.mxd_mix_apply_u8(p, s12, None, s12, 4, 4, ok, o, s12) == capi.MXD_ERR_INVALID
    assert L.mxd_last_error() == b"mxd: null pixels"
    assert L.mxd_mix_apply_u8(p, s12, r, s11, 4, 4, ok, o, s12) == capi.MXD_ERR_INVALID
    assert L.mxd_last_error() == b"mxd: stride smaller than a row"
    assert L.mxd_mix_apply_u8(p, s12, r, s12, -1, 4, ok, o, s12) == capi.MXD_ERR_INVALID
    assert L.mxd_mix_apply_u8(p, s12, r, s12, 4, 4, ok, o, s12) == capi.MXD_OK
    assert L.mxd_mix_apply_u8(p, s12, r, s12, 4, 4, capi.make_mixes([M.entry_cutmix(0, 0, 0, 5, 4)]), o, s12) == capi.MXD_ERR_INVALID
    assert L.mxd_last_error() == b"mxd_mix: box needs 0 <= x0 <= x1 <= crop_w, got x0 0 x1 5 crop_w 4 (image 0)"
    # (the statement reads no partner index)
    assert L.mxd_mix_apply_u8(p, s12, r, s12, 4, 4, capi.make_mixes([(M.MIXUP, 77, 0.5, 0.5)]), o, s12) == capi.MXD_OK


def test_every_declared_symbol_is_exported():
    L = capi.lib()
    header = open(os.path.join(os.path.dirname(HERE), "include", "mxd_amd.h")).read()
    assert "#define MXD_HAS_MIX 1" in header and "#define MXD_ABI_VERSION 7" in header
    assert L.mxd_abi_version() == 7
    for name in ("mxd_mix_validate", "mxd_mix_apply_u8", "mxd_resize_crop_batch_mix", "mxd_resize_crop_to_device_mix",
                 "mxd_jpeg_resize_crop_to_device_mix"):
        assert name + "(" in header and name in capi.EXPORTS
        assert getattr(L, name) is not None
    assert ctypes.sizeof(capi.MxdMix) == 40
    assert "MXD_MIX_NONE = 0, MXD_MIX_MIXUP = 1, MXD_MIX_CUTMIX = 2" in header
    assert (capi.MXD_MIX_NONE, capi.MXD_MIX_MIXUP, capi.MXD_MIX_CUTMIX) == (0, 1, 2)
    assert capi.mixup(3, 0.3) == (1, 3, 0.3, 1.0 - 0.3) and capi.cutmix(2, 1, 2, 3, 4) == (2, 2, 1, 2, 3, 4)


def test_weights_that_do_not_sum_to_one_saturate_at_255():
    """The header's min(rint(x), 255): only weights a lam never gives reach it."""
    q, r = M.byte_pair_grid()
    got = capi.mix_apply_u8(q, r, (M.MIXUP, 0, 1.0, 1.0))
    assert np.array_equal(got, np.minimum(q.astype(np.int32) + r, 255).astype(np.uint8))
    got = capi.mix_apply_u8(q, r, (M.MIXUP, 0, 1.0, 0.5))
    x = q.astype(np.float32) + r.astype(np.float32) * np.float32(0.5)
    assert np.array_equal(got, np.minimum(np.rint(x), 255).astype(np.uint8))


# ---- operator surface: arguments, the draw stream -------------------------------------------

def _buf(n=4):
    from mlx_data_amd import data as dx

    return dx.buffer_from_vector([dict(image=np.zeros((8, 10, 3), np.uint8)) for _ in range(n)])


@pytest.mark.parametrize("kw,word", [
    (dict(), "one of mixup_alpha and cutmix_alpha must be > 0"),
    (dict(mixup_alpha=-1.0), "mixup_alpha must be finite and >= 0"),
    (dict(mixup_alpha=NAN), "mixup_alpha must be finite and >= 0"),
    (dict(cutmix_alpha=INF), "cutmix_alpha must be finite and >= 0"),
    (dict(cutmix_alpha=-0.5, mixup_alpha=1.0), "cutmix_alpha must be finite and >= 0"),
    (dict(mixup_alpha=1.0, prob=1.5), "prob must be in 0..1"),
    (dict(mixup_alpha=1.0, prob=NAN), "prob must be in 0..1"),
    (dict(mixup_alpha=1.0, switch_prob=-0.1), "switch_prob must be in 0..1"),
    (dict(mixup_alpha=1.0, mode="sample"), "unknown mode 'sample'"),
    (dict(mixup_alpha=1.0, lam_key="x", partner_key="x"), "key, lam_key and partner_key must differ"),
    (dict(mixup_alpha=1.0, lam_key="image"), "key, lam_key and partner_key must differ"),
    (dict(mixup_alpha=1.0, lam_key=""), "lam_key and partner_key must not be empty"),
    (dict(mixup_alpha=1.0, partner_key=""), "lam_key and partner_key must not be empty"),
])
def test_surface_refuses_bad_arguments_when_the_op_is_made(kw, word):
    for b in (_buf(), _buf().to_stream()):
        with pytest.raises(ValueError) as err:
            b.batch_mix(2, "image", **kw)
        assert "batch_mix: " in str(err.value) and word in str(err.value), str(err.value)


def test_the_compat_package_carries_the_op():
    import sys

    compat = os.path.join(os.path.dirname(HERE), "mlx-data_amd", "compat")
    sys.path.insert(0, compat)
    try:
        import mlx.data as md
    finally:
        sys.path.remove(compat)
    assert callable(md.Buffer.batch_mix) and callable(md.Stream.batch_mix)


class Words:
    """std::mt19937(seed)'s 32-bit outputs, and libstdc++'s distributions over
    them: generate_canonical<double, 53> takes two words, low word first;
    uniform_int_distribution<int>(0, n - 1) is Lemire's multiply-and-reject."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)  # the same mt19937 seeding as std::mt19937(seed)

    def word(self):
        return int(self.rs.randint(0, 2 ** 32, dtype=np.uint64))

    def uniform(self):
        r0, r1 = self.word(), self.word()
        return (float(r0) + float(r1) * 4294967296.0) / 18446744073709551616.0

    def below(self, n):
        product = self.word() * n
        if (product & 0xFFFFFFFF) < n:
            threshold = (2 ** 32 - n) % n
            while (product & 0xFFFFFFFF) < threshold:
                product = self.word() * n
        return product >> 32


def _restated(words, n, h, w, mode, prob=1.0, cut=False):
    """The entries of a batch for alpha == 1 (MixUp, or CutMix with cut), restated."""
    def one():
        if not words.uniform() < prob:
            return (0, None, 0.0, 0.0, 0, 0, 0, 0, 1.0)
        lam = words.uniform()
        if not cut:
            return (1, None, float(np.float32(lam)), float(np.float32(1.0 - lam)), 0, 0, 0, 0, float(np.float32(lam)))
        ratio = np.sqrt(1.0 - lam)
        cut_h, cut_w = int(h * ratio), int(w * ratio)
        cy = words.below(h)
        cx = words.below(w)
        y0, y1 = (int(np.clip(cy + s * (cut_h // 2), 0, h)) for s in (-1, 1))
        x0, x1 = (int(np.clip(cx + s * (cut_w // 2), 0, w)) for s in (-1, 1))
        return (2, None, 0.0, 0.0, x0, y0, x1, y1, float(np.float32(1.0 - (y1 - y0) * (x1 - x0) / (h * w))))

    out = [None] * n
    if mode == "batch":
        out = [one()] * n
    elif mode == "pair":
        for k in range((n + 1) // 2):
            out[k] = out[n - 1 - k] = one()
    else:
        out = [one() for _ in range(n)]
    return [(e[0], i if e[0] == 0 else n - 1 - i) + e[2:] for i, e in enumerate(out)]


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_the_draw_stream_for_alpha_one_restated_from_mt19937_words(mode):
    from mlx_data_amd import _pipeline
    from mlx_data_amd import data as dx

    for seed, n, prob, cut in ((11, 5, 1.0, False), (12, 6, 0.5, False), (13, 7, 1.0, True), (14, 4, 0.6, True)):
        dx.set_state(seed)
        kw = dict(cutmix_alpha=1.0) if cut else dict(mixup_alpha=1.0)
        got = _pipeline._batch_mix_draws(n, 29, 33, mode=mode, prob=prob, **kw)
        want = _restated(Words(seed), n, 29, 33, mode, prob, cut)
        assert got == want, (seed, mode, got, want)
        if cut:
            for e in got:
                assert e[0] == 0 or (0 <= e[4] <= e[6] <= 33 and 0 <= e[5] <= e[7] <= 29)
    # with both alphas one more draw picks the op: < switch_prob is CutMix
    dx.set_state(15)
    got = _pipeline._batch_mix_draws(64, 29, 33, mixup_alpha=1.0, cutmix_alpha=1.0, mode="elem", switch_prob=0.25)
    words = Words(15)
    for e in got:
        assert words.uniform() < 1.0
        cut = words.uniform() < 0.25
        assert e[0] == (2 if cut else 1)
        lam = words.uniform()
        if cut:
            words.below(29), words.below(33)
        else:
            assert e[8] == float(np.float32(lam))
    assert {e[0] for e in got} == {1, 2}
    # a set that is not applied: NONE, lam 1, its own partner
    dx.set_state(16)
    assert _pipeline._batch_mix_draws(3, 8, 8, mixup_alpha=1.0, prob=0.0, mode=mode) == [
        (0, i, 0.0, 0.0, 0, 0, 0, 0, 1.0) for i in range(3)]


@pytest.mark.parametrize("alpha", [0.2, 0.8, 2.0])
def test_gamma_draws_are_reproducible_bounded_and_centred(alpha):
    from mlx_data_amd import _pipeline
    from mlx_data_amd import data as dx

    def lams(seed):
        dx.set_state(seed)
        return [e[8] for e in _pipeline._batch_mix_draws(4000, 16, 16, mixup_alpha=alpha, mode="elem")]

    one, again, other = lams(3), lams(3), lams(4)
    assert one == again and one != other
    assert all(0.0 <= v <= 1.0 for v in one)
    assert abs(float(np.mean(one)) - 0.5) < 0.05
