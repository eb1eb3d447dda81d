"""GPU: every triangle-filter wave kernel of mlx-data_amd/csrc/wave.hip at its
smallest shape (tests/wave_shapes.py), route asserted and bit exact.

One parametrized case per instantiation key.  The key's two whole-frame shapes
-- one strip at about 20 rows, two strips at 64 rows and columns or more --
are each submitted whole, mirrored, as an inner window at odd offsets mirrored
and as a window on the far right and bottom edges, all in one batch per launch
configuration: u8, q/255 f32, float16 HWC unnormalised and ImageNet-normalised
bfloat16 CHW; both source-load policies (the nt form of every scatter kernel);
and, for the second shape, every source base offset the key has a form for.
mxd_describe_plan must name the key for every whole frame before it runs.
4:2:0 JPEGs of the P = 4 scatter shapes go through the plane-source form,
counted by mxd_jpeg_plane_sources.  The named cases of wave_shapes.EXTRA
(deeper schedules, larger tap buckets) run the same way.

Expected: u8 bit-equal to the kernel-order restatement O.resize_crop_vfirst,
f32 exactly LUT[u8], formatted output the NumPy / torch table of the oracle's
bytes, frames of 64 x 64 and more within +-1 / 2e-3 of the stbir-order oracle.
Every destination has padded rows, a head and a tail, filled with 0xA5 before
the launch; afterwards every byte outside the image's elements (CHW: the gaps
between the planes too) must still be 0xA5.  Nothing expected comes from the
library's kernels."""
import io

import numpy as np
import pytest

import oracle as O
import wave_shapes as W
from gpu_util import compare, oracle_out, synth
from mlx_data_amd import capi
from out_format_util import ELEMS, IMAGENET_MEAN, IMAGENET_STD, LAYOUTS, expect, expected_table

pytestmark = pytest.mark.gpu

GUARD = 0xA5
HEAD = 64   # guard bytes before a destination's first element
TAIL = 96   # ... and after its last row (plane)
LUT = (np.arange(256, dtype=np.uint8).astype("float32") / 255).view(np.uint32)
MAX_FRAC = 2e-3

# name -> (element bytes, channel planes, element type or None, mean, std)
MODES = {
    "u8": (1, False, None, None, None),
    "f32": (4, False, None, None, None),
    "f16_hwc": (2, False, "float16", None, None),
    "bf16_chw": (2, True, "bfloat16", IMAGENET_MEAN, IMAGENET_STD),
}

# every (key, shift, nt, output mode, source kind) the cases of this process launched
LAUNCHED = set()


class Dsts:
    """Guarded destinations of a batch in one output mode: rows a few bytes
    (u8: 5, f32: 8, formatted: 3 elements) longer than the pixels, CHW planes 5
    elements longer than their rows, HEAD / TAIL bytes around, all 0xA5 until
    the launch."""

    def __init__(self, geoms, channels, mode):
        self.es, self.chw, self.elem, self.mean, self.std = MODES[mode]
        self.mode, self.geoms, self.channels = mode, geoms, channels
        es = self.es
        pad = W.dst_pad(mode == "f32") if self.elem is None else 3 * es
        self.pitch = [g[4] * (1 if self.chw else c) * es + pad for g, c in zip(geoms, channels)]
        self.plane = max(p * g[5] for p, g in zip(self.pitch, geoms)) + 5 * es if self.chw else 0
        self.size = [self.plane * c if self.chw else p * g[5] for p, g, c in zip(self.pitch, geoms, channels)]
        self.bufs = [capi.DeviceBuffer(HEAD + s + TAIL) for s in self.size]
        for b in self.bufs:
            b.memset(GUARD)
        capi.check(capi.lib().mxd_device_synchronize(0))

    def ptr(self, k):
        return self.bufs[k].ptr + HEAD

    def fmt(self, c):
        cut = (lambda v: None if v is None else v[:c])
        return capi.make_out_format(ELEMS[self.elem], LAYOUTS["chw" if self.chw else "hwc"], cut(self.mean),
                                    cut(self.std), self.plane)

    def read(self):
        """The images as (H, W, C) integer bits; asserts the guard bytes."""
        es = self.es
        ut = {1: np.uint8, 2: np.uint16, 4: np.uint32}[es]
        outs = []
        for k, (b, g, c, pitch, size) in enumerate(zip(self.bufs, self.geoms, self.channels, self.pitch, self.size)):
            cw, ch = g[4], g[5]
            raw = b.download((HEAD + size + TAIL,), np.uint8)
            outside = np.ones(raw.shape, bool)
            if self.chw:
                planes = []
                for j in range(c):
                    lo = HEAD + j * self.plane
                    planes.append(raw[lo:lo + pitch * ch].reshape(ch, pitch)[:, :cw * es].copy().view(ut))
                    outside[lo:lo + pitch * ch].reshape(ch, pitch)[:, :cw * es] = False
                out = np.stack(planes, axis=2)
            else:
                out = raw[HEAD:HEAD + size].reshape(ch, pitch)[:, :cw * c * es].copy().view(ut).reshape(ch, cw, c)
                outside[HEAD:HEAD + size].reshape(ch, pitch)[:, :cw * c * es] = False
            bad = np.flatnonzero(outside & (raw != GUARD))
            assert bad.size == 0, (self.mode, k, g, "bytes outside the image were written, first at",
                                   bad[:4] - HEAD, "pitch", pitch, "plane", self.plane)
            outs.append(out)
        return outs

    def free(self):
        for b in self.bufs:
            b.free()

    def check(self, wants, tag):
        """The outputs against the expected bytes `wants` in this mode."""
        for k, (o, w) in enumerate(zip(self.read(), wants)):
            if self.elem is not None:
                c = w.shape[2]
                cut = (lambda v: None if v is None else v[:c])
                w = expect(expected_table(self.elem, c, cut(self.mean), cut(self.std)), w)
            elif self.mode == "f32":
                w = LUT[w]
            assert o.shape == w.shape, (tag, self.mode, k)
            diff = np.argwhere(o != w)
            assert diff.size == 0, (tag, self.mode, k, self.geoms[k], len(diff), "first (y, x, c)", diff[:3].tolist())


def launch(imgs, geoms, mode, shift=0):
    """One mxd_resize_crop_batch (/ _fmt) call over device copies of imgs, each
    `shift` bytes past a 256-byte boundary with rows of W.src_stride; returns
    the guarded destinations."""
    pitches, offs, total = [], [], 0
    for img in imgs:
        h, w, c = img.shape
        pitches.append(W.src_stride(w, c, shift))
        offs.append(total + shift)
        total += (pitches[-1] * h + 255) // 256 * 256
    host = np.zeros(total + 256, np.uint8)
    for img, p, o in zip(imgs, pitches, offs):
        h, w, c = img.shape
        host[o:o + p * h].reshape(h, p)[:, :w * c] = img.reshape(h, w * c)
    src = capi.DeviceBuffer(total + 256)
    src.upload(host)
    d = Dsts(geoms, [i.shape[2] for i in imgs], mode)
    try:
        entries = []
        for k, (img, g, p, o) in enumerate(zip(imgs, geoms, pitches, offs)):
            e = W.entry(img.shape, g, shift)
            entries.append(dict(e, src=src.ptr + o, src_stride=p, dst=d.ptr(k), dst_stride=d.pitch[k]))
        arr, n = capi.make_images(entries)
        if d.elem is None:
            capi.resize_crop_batch(arr, n, capi.MXD_F32_DIV255 if mode == "f32" else capi.MXD_U8, 0, None)
        else:
            capi.resize_crop_batch_fmt(arr, n, d.fmt(imgs[0].shape[2]), 0, None)
        capi.check(capi.lib().mxd_device_synchronize(0))
    except BaseException:
        d.free()
        raise
    finally:
        src.free()
    return d


def with_knobs(policy, load, f):
    prev_p = capi.set_kernel_policy(policy)
    prev_l = capi.set_tuning(capi.MXD_TUNE_LOAD_POLICY, load)
    try:
        return f()
    finally:
        capi.set_tuning(capi.MXD_TUNE_LOAD_POLICY, prev_l)
        capi.set_kernel_policy(prev_p)


def gate(got, img, g):
    if g[4] >= 64 and g[5] >= 64:
        m, frac = compare(got, oracle_out(img, g))
        assert m <= 1 and frac < MAX_FRAC, (g, m, frac)


def run_frames(key, policy, frames, tag):
    """frames: [(image, (out w, out h), shifted too)].  Asserts the plan of every
    whole frame, then runs every window of every frame in every configuration."""
    c = frames[0][0].shape[2]
    sets = {}  # shift -> (images, geometries)
    for img, (cw, ch), shifted in frames:
        assert ch % 8 != 0 and ch > 16
        for shift in (W.shifts_of(key) if shifted else (0,)):
            ok, _ = W.planned(key, img.shape, W.whole(cw, ch), (shift,))
            assert ok, (tag, key, img.shape, (cw, ch), shift, W.plan(img.shape, W.whole(cw, ch), policy, shift))
            imgs, geoms = sets.setdefault(shift, ([], []))
            for g in W.windows(cw, ch):
                imgs.append(img)
                geoms.append(g)
    wants = {}
    for shift, (imgs, geoms) in sets.items():
        for img, g in zip(imgs, geoms):
            if (id(img), g) not in wants:
                wants[id(img), g] = O.resize_crop_vfirst(img, g)
                gate(wants[id(img), g], img, g)  # (the bytes the device must give, so this is its gate too)
    for shift, (imgs, geoms) in sorted(sets.items()):
        for load in ((1,) if W.is_gather(key) else (1, 2)):  # (gather kernels have one load form)
            for mode in MODES:
                d = with_knobs(policy, load, lambda: launch(imgs, geoms, mode, shift))
                try:
                    d.check([wants[id(i), g] for i, g in zip(imgs, geoms)], (tag, key, "shift", shift, "load", load))
                finally:
                    d.free()
                LAUNCHED.add((key, shift, load == 2, mode, "rgb" if c == 3 else "c%d" % c))


def encode_420(a):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=90, subsampling=2)
    return b.getvalue()


def run_planes(key):
    """4:2:0 JPEGs of the key's two shapes resized from their sample planes (the
    count is the route assertion) in u8, f32 and bfloat16 CHW: the whole frame,
    mirrored too, and those of the other windows that plan the same key.
    Expected: the oracle on the host decode of the same files."""
    datas, pixels, geoms = [], [], []
    for k, (sw, sh, cw, ch, _) in enumerate(W.SHAPES[key]):
        data = encode_420(synth(sh, sw, 3, W.seed_of(key, k)))
        px = capi.jpeg_decode(data)
        assert px.shape == (sh, sw, 3)
        for j, g in enumerate(W.windows(cw, ch)):
            ok, _ = W.planned(key, px.shape, g, (0,))
            assert ok or j >= 2, (key, px.shape, g)
            if ok:
                datas.append(data)
                pixels.append(px)
                geoms.append(g)
    wants = [O.resize_crop_vfirst(px, g) for px, g in zip(pixels, geoms)]
    coefs = [capi.JpegCoefs(x) for x in datas]
    try:
        for mode in ("u8", "f32", "bf16_chw"):
            d = Dsts(geoms, [3] * len(geoms), mode)
            try:
                entries = [dict(coefs=co, resize_w=g[0], resize_h=g[1], crop_x=g[2], crop_y=g[3], crop_w=g[4],
                                crop_h=g[5], flip=g[6], dst=d.ptr(k), dst_stride=d.pitch[k])
                           for k, (co, g) in enumerate(zip(coefs, geoms))]
                arr, n = capi.make_jpeg_images(entries)
                capi.jpeg_plane_sources(reset=True)

                def call():
                    if d.elem is None:
                        capi.jpeg_resize_crop_to_device(arr, n, capi.MXD_F32_DIV255 if mode == "f32" else capi.MXD_U8, 0)
                    else:
                        capi.jpeg_resize_crop_to_device_fmt(arr, n, d.fmt(3), 0)

                with_knobs(W.policy_of(key), 0, call)
                capi.check(capi.lib().mxd_device_synchronize(0))
                assert capi.jpeg_plane_sources(reset=True) == n, (key, mode)
                d.check(wants, ("planes", key))
            finally:
                d.free()
            LAUNCHED.add((key, 0, False, mode, "ycc"))
    finally:
        for co in coefs:
            co.close()


def frames_of(key):
    c = W.channels_of(key)
    out = []
    for k, shape in enumerate(W.SHAPES[key]):
        if shape is None:
            continue
        sw, sh, cw, ch, _ = shape
        out.append((synth(sh, sw, c, W.seed_of(key, k)), (cw, ch), k == 1))
    return out


SCATTER = sorted(k for k in W.SHAPES if not W.is_gather(k))
GATHER = sorted(k for k in W.SHAPES if W.is_gather(k))


@pytest.mark.parametrize("key", SCATTER, ids=lambda k: "s%d_d%d_t%d_q%d_p%d" % k)
def test_every_scatter_kernel(key):
    run_frames(key, W.policy_of(key), frames_of(key), "scatter")
    if key[4] == 4:
        run_planes(key)


@pytest.mark.parametrize("key", GATHER, ids=lambda k: "c%d_t%d_q%d" % k)
def test_every_gather_kernel(key):
    run_frames(key, W.policy_of(key), frames_of(key), "gather")


@pytest.mark.parametrize("name", sorted(W.EXTRA))
def test_deeper_schedules_and_larger_tap_buckets(name):
    """Shapes between the instantiated ones: a vertical ratio run on the next
    deeper schedule (bubble iterations fill the gap), horizontal taps run in
    the next larger bucket (zero weights fill it)."""
    key, (sw, sh), (cw, ch) = W.EXTRA[name]
    img = synth(sh, sw, 3, W.seed_of(key, name))
    run_frames(key, W.policy_of(key), [(img, (cw, ch), True)], name)

