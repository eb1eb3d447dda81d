"""GPU: every instantiation of the general tile kernel (mlx-data_amd/csrc/
resample.hip) at its smallest shape (tests/general_shapes.py), route asserted
and bit exact.

Every launch runs under MXD_POLICY_NO_WAVE; before it runs, mxd_describe_plan
and mxd_describe_band_plan must both decline every image (the general kernel is
what is left).  How general_group tiles each launch -- strips, bands, row
group, vec, LDS bytes -- is asserted on the host by tests/test_general_shapes.py
over the same table.

* one parametrized case per (VEC, C, ALPHA): both frames of the key as the four
  windows of wave_shapes.windows, in u8 and f32, one batch per source layout
  (VEC = 1: packed rows, and padded rows from a base 1 byte past a 16-byte
  boundary) and destination layout;
* the named launches of general_shapes.EXTRA: vertical tap counts of every
  remainder of the 4-way unrolled loop, the store paths (row ends of 1, 2 and 3
  elements, destinations off and on the vector stores' alignment), a mixed
  launch (LDS strides are the launch's maxima; one unaligned image makes the
  whole launch VEC = 1), launches of 1, 7, 8, 9 and 15 tiles, deep ratios (up
  to 64 KiB of LDS, 64 to 160 KiB, the refusal past 160 KiB, a row group of one
  row through kLdsBudget), the weighted RGBA form with exactly transparent
  output pixels and, over Catmull-Rom tables, with pixels of negative filtered
  alpha (the kTinyAlpha branch), cubic tables.

Expected: u8 bit-equal to the kernel-order restatements O.resize_crop_vfirst /
O.resize_crop_vfirst_rgba (cubic tables: filter_ref.vfirst and its weighted form), f32 exactly
LUT[u8] as bits; everything is compared as integers.  Frames of 64 x 64 and
more are within +-1 / 2e-3 of the stbir-order oracle.  Destinations are guarded
as test_gpu_wave_shapes.Dsts guards them: padded rows, a head and a tail, 0xA5
before the launch and outside the image's elements afterwards.  Sources have
0xFF in every byte that is no pixel (row tails, head, tail).  Nothing expected
comes from the library's kernels."""
import numpy as np
import pytest

import filter_ref
import general_shapes as G
import oracle as O
import test_gpu_wave_shapes as T
import wave_shapes as W
from gpu_util import synth
from mlx_data_amd import capi

pytestmark = pytest.mark.gpu

FILL = 0xFF
SRC_HEAD = 64   # 0xFF bytes before an image's first pixel (+ the base offset)
SRC_TAIL = 64   # ... and after its last row, at least

# every (VEC, C, F32, ALPHA) the cases of this process launched
LAUNCHED = set()


def dst_layout(name, row_bytes, f32):
    """(bytes the base is past a 64-byte boundary, row pitch) of a destination layout:
    odd -- test_gpu_wave_shapes' (rows 5 / 8 bytes longer than the pixels);
    vec -- base and pitch on the vector stores' alignment (16 bytes);
    off -- u8: base 1 byte off, pitch no multiple of 4; f32: base 4 bytes past a 16-byte
           boundary, pitch a multiple of 4 and not of 16."""
    if name == "odd":
        return 0, row_bytes + W.dst_pad(f32)
    if name == "vec":
        return 0, (row_bytes + 15) // 16 * 16 + 16
    assert name == "off"
    if f32:
        pitch = row_bytes + 8
        return 4, pitch if pitch % 16 else pitch + 4
    pitch = row_bytes + 5
    return 1, pitch if pitch % 4 else pitch + 1


class Dsts:
    """Guarded u8 / f32 destinations of a batch, one layout each."""

    def __init__(self, geoms, channels, f32, layouts):
        self.f32, self.geoms, self.channels = f32, geoms, channels
        es = 4 if f32 else 1
        self.head, self.pitch = zip(*[dst_layout(name, g[4] * c * es, f32) for g, c, name in zip(geoms, channels, layouts)])
        self.size = [p * g[5] for p, g in zip(self.pitch, geoms)]
        self.bufs = [capi.DeviceBuffer(T.HEAD + h + s + T.TAIL) for h, s in zip(self.head, self.size)]
        for b in self.bufs:
            b.memset(T.GUARD)
        capi.check(capi.lib().mxd_device_synchronize(0))

    def ptr(self, k):
        return self.bufs[k].ptr + T.HEAD + self.head[k]

    def read(self, untouched=False):
        """The images as (H, W, C) integer bits; asserts the guard bytes (untouched: every byte)."""
        es, ut = (4, np.uint32) if self.f32 else (1, np.uint8)
        outs = []
        for k, (b, g, c) in enumerate(zip(self.bufs, self.geoms, self.channels)):
            cw, ch = g[4], g[5]
            lo, pitch, size = T.HEAD + self.head[k], self.pitch[k], self.size[k]
            raw = b.download((lo + size + T.TAIL,), np.uint8)
            outside = np.ones(raw.shape, bool)
            rows = raw[lo:lo + size].reshape(ch, pitch)[:, :cw * c * es]
            if not untouched:
                outside[lo:lo + size].reshape(ch, pitch)[:, :cw * c * es] = False
            bad = np.flatnonzero(outside & (raw != T.GUARD))
            assert bad.size == 0, ("f32" if self.f32 else "u8", k, g, "bytes outside the image were written, first at",
                                   bad[:4] - lo, "pitch", pitch)
            outs.append(np.ascontiguousarray(rows).view(ut).reshape(ch, cw, c))
        return outs

    def check(self, wants, tag):
        for k, (o, w) in enumerate(zip(self.read(), wants)):
            w = T.LUT[w] if self.f32 else w
            assert o.shape == w.shape and o.dtype == w.dtype, (tag, k)
            diff = np.argwhere(o != w)
            assert diff.size == 0, (tag, "f32" if self.f32 else "u8", k, self.geoms[k], len(diff), "first (y, x, c)",
                                    diff[:3].tolist())

    def free(self):
        for b in self.bufs:
            b.free()


def submit(imgs, geoms, layouts, f32, dsts, weighted=None, filters=None):
    """One mxd_resize_crop_batch call under G.POLICY; every distinct (image,
    source layout) is stored once.  Returns the guarded destinations (the call's
    error, if any, is raised after they are made: the caller frees them)."""
    off, total = {}, 0
    for img, lay in zip(imgs, layouts):
        if (id(img), lay) not in off:
            h, w, c = img.shape
            off[id(img), lay] = total + SRC_HEAD + G.LAYOUTS[lay][0]
            total += (SRC_HEAD + 16 + G.src_stride(w, c, lay) * h + SRC_TAIL + 255) // 256 * 256
    host = np.full(total, FILL, np.uint8)
    for img, lay in zip(imgs, layouts):
        h, w, c = img.shape
        p, o = G.src_stride(w, c, lay), off[id(img), lay]
        host[o:o + p * h].reshape(h, p)[:, :w * c] = img.reshape(h, w * c)
    entries = []
    for k, (img, g, lay) in enumerate(zip(imgs, geoms, layouts)):
        flt = filters[k] if filters else 0
        assert G.is_general(img.shape, g, lay, f32, flt), ("not the general kernel's", img.shape, g, lay)
        entries.append(G.entry(img.shape, g, lay, f32, flt, weighted[k] if weighted else 0))
    src = capi.DeviceBuffer(total)
    src.upload(host)
    d = Dsts(geoms, [i.shape[2] for i in imgs], f32, dsts)
    try:
        for k, (img, lay) in enumerate(zip(imgs, layouts)):
            entries[k] = dict(entries[k], src=src.ptr + off[id(img), lay], dst=d.ptr(k), dst_stride=d.pitch[k])
            assert entries[k]["src"] % 16 == G.LAYOUTS[lay][0]
        arr, n = capi.make_images(entries)
        prev = capi.set_kernel_policy(G.POLICY)
        try:
            capi.resize_crop_batch(arr, n, capi.MXD_F32_DIV255 if f32 else capi.MXD_U8, 0, None)
        finally:
            capi.set_kernel_policy(prev)
        capi.check(capi.lib().mxd_device_synchronize(0))
    except capi.MxdError as e:
        d.error = e
    except BaseException:
        d.free()
        raise
    else:
        d.error = None
    finally:
        src.free()
    return d


_wants = {}


def want(img, g, weighted=0, flt=0):
    """The expected bytes (computed once per image and geometry; frames of
    64 x 64 and more pass the project's gate against the stbir-order oracle)."""
    key = (id(img), g, weighted, flt)
    if key not in _wants:
        if flt:
            w = filter_ref.vfirst(img, g, flt, bool(weighted))
        elif weighted:
            w = O.resize_crop_vfirst_rgba(img, g)
            T.gate(w, img, g)
        else:
            w = O.resize_crop_vfirst(img, g)
            if img.shape[2] < 4:  # (the stbir-order oracle's 4-channel form is the weighted one)
                T.gate(w, img, g)
        _wants[key] = (img, w)  # (the image is kept: its id stays its own)
    return _wants[key][1]


def run(imgs, geoms, layouts, tag, weighted=None, filters=None, dst_names=("odd", "vec"), modes=(False, True)):
    """The launch in every output mode and destination layout; returns the (VEC, C,
    F32, ALPHA) keys it ran.  The library does not report what it launched:
    the keys are what general_shapes says of the launch (vec_of over the source
    layouts, the weighted flags), which holds through `submit`'s assertion on
    every source address and tests/test_general_shapes.py's on the vec, alpha
    and f32 that build_layout gives the same entries.  A call of weighted and
    unweighted images counts for both alpha keys: that split_batch makes two
    launches of it is asserted there too, on the sub-batches, not here."""
    c = imgs[0].shape[2]
    vec = 16 if all(G.vec_of(i.shape[1], c, lay) == 16 for i, lay in zip(imgs, layouts)) else 1
    wants = [want(i, g, weighted[k] if weighted else 0, filters[k] if filters else 0)
             for k, (i, g) in enumerate(zip(imgs, geoms))]
    keys = set()
    for f32 in modes:
        for name in dst_names:
            d = submit(imgs, geoms, layouts, f32, [name] * len(imgs), weighted, filters)
            try:
                if d.error is not None:
                    raise d.error
                d.check(wants, (tag, "vec", vec, "dst", name))
            finally:
                d.free()
        alphas = set(weighted) if weighted and c == 4 else {0}
        keys |= {(vec, c, f32, bool(a)) for a in alphas}
    LAUNCHED.update(keys)
    return keys


def image_of(key, which, sw, sh, c, plane):
    """plane: the alpha plane of a weighted image (a name of G.ALPHA_PLANES), or nothing."""
    img = synth(sh, sw, c, G.seed_of(key, which))
    return G.ALPHA_PLANES[plane](img) if plane else img


KEYS = sorted(G.SHAPES)


@pytest.mark.parametrize("key", KEYS, ids=G.key_id)
def test_every_general_kernel(key):
    vec, c, alpha = key
    frames = [(image_of(key, k, sw, sh, c, "holes" if alpha else None), cw, ch) for k, (sw, sh, cw, ch) in enumerate(G.SHAPES[key])]
    imgs, geoms = zip(*[(img, g) for img, cw, ch in frames for g in W.windows(cw, ch)])
    for layout in G.layouts_of(vec):
        ran = run(imgs, geoms, [layout] * len(imgs), (G.key_id(key), layout), weighted=[int(alpha)] * len(imgs))
        assert ran == {(vec, c, f32, alpha) for f32 in (False, True)}, (key, layout, ran)


def extra_images(name):
    case = G.EXTRA[name]
    c = case["c"]
    weighted = case.get("weighted") or [0] * len(case["images"])
    imgs, geoms, cache = [], [], {}
    for k, ((sw, sh), g) in enumerate(case["images"]):
        if (sw, sh, weighted[k]) not in cache:
            cache[sw, sh, weighted[k]] = image_of(name, len(cache), sw, sh, c, weighted[k] and case.get("plane", "holes"))
        imgs.append(cache[sw, sh, weighted[k]])
        geoms.append(tuple(g))
    return case, imgs, geoms, weighted


def transparent_outputs(img, g):
    """Output pixels (y, x) of geometry g all of whose taps have alpha 0: their
    filtered alpha is exactly 0, below kTinyAlpha."""
    rw, rh, cx, cy, cw, ch, flip = g
    h, w = img.shape[:2]
    xf, xn, _ = capi.axis_taps(w, rw)
    yf, yn, _ = capi.axis_taps(h, rh)
    clear = img[:, :, 3] == 0
    hits = []
    for y in range(ch):
        for x in range(cw):
            ox = cx + (cw - 1 - x if flip else x)
            oy = cy + y
            if clear[yf[oy]:yf[oy] + yn[oy], xf[ox]:xf[ox] + xn[ox]].all():
                hits.append((y, x))
    return hits


@pytest.mark.parametrize("name", sorted(G.EXTRA))
def test_named_launches(name):
    case, imgs, geoms, weighted = extra_images(name)
    filters = [case["filter"]] * len(imgs) if case.get("filter") else None
    if case.get("transparent"):
        # whole output pixels under kTinyAlpha: the oracle leaves them premultiplied, i.e. all zero
        found = 0
        for k, (img, g, a) in enumerate(zip(imgs, geoms, weighted)):
            if a:
                hits = transparent_outputs(img, g)
                assert len(hits) >= 4 or k >= 2, (name, g)  # (the whole frame and its mirror image have them)
                w = want(img, g, 1)
                assert all((w[y, x] == 0).all() for y, x in hits), (name, g)
                found += len(hits)
        assert found >= 8, (name, found)
    if case.get("negative_alpha"):
        # whole output pixels whose filtered alpha is negative: below kTinyAlpha and not 0
        for img, g in list(zip(imgs, geoms))[:2]:
            neg = G.filtered_alpha(img, g, case["filter"]) < -1.0 / 255
            assert neg.sum() >= 16, (name, g, int(neg.sum()))
            assert (want(img, g, 1, case["filter"])[neg][:, 3] == 0).all(), (name, g)
    for layouts in case["layouts"]:
        layouts = [layouts] * len(imgs) if isinstance(layouts, str) else list(layouts)
        if case.get("refused"):
            for f32 in (False, True):
                d = submit(imgs, geoms, layouts, f32, ["odd"] * len(imgs))
                try:
                    assert d.error is not None and d.error.code == capi.MXD_ERR_UNSUPPORTED, (name, d.error)
                    assert "tile does not fit in LDS" in str(d.error), str(d.error)
                    d.read(untouched=True)
                finally:
                    d.free()
            continue
        run(imgs, geoms, layouts, (name, layouts[0]), weighted=weighted if case["c"] == 4 else None, filters=filters,
            dst_names=case.get("dsts", ("odd", "vec")))


def test_every_instantiation_was_launched():
    missing = G.instantiations() - LAUNCHED
    assert not missing, sorted(missing)
