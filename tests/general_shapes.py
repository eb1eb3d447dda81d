"""The general tile kernel of mlx-data_amd/csrc/resample.hip, one shape each.

``instantiations()`` reads the kernel list out of resample.hip: a key is
``(VEC, C, F32, ALPHA)`` -- the ``launch_v`` cases (channels and output mode),
the two ``cfg.vec`` values of ``launch_resample`` and the ``ALPHA`` launch of
``launch_t`` for ``C == 4``.  ``SHAPES`` holds, per ``(VEC, C, ALPHA)`` (u8 and
f32 share the frames), two whole frames ``(src_w, src_h, out_w, out_h)``:

(a) one tile: one strip, 20 output rows;
(b) two strips or more with a short last strip, and two bands with a short
    last one (37 rows = 32 + 5), the row group shorter than the band.

``find(key, which)`` is the search that gave them (``python
tests/general_shapes.py`` prints the entries again): source rows fixed at
``2 * out_h + 1`` (five- and six-tap rows: the 4-way unrolled loop and its
remainder), source columns ascending -- the smallest source area first -- and
for each the output widths that make the horizontal ratio 2 : 1 to 3 : 1,
ascending.  Shape (b) also has a row of ``out_w * C`` elements that is no
multiple of 4 where ``C`` allows one (``C`` < 4: the last strip's rows then end
in a store of 1 to 3 elements).  ``VEC = 1`` frames have packed rows that are
no multiple of 16 bytes; tests/test_gpu_general_shapes.py runs them from a
16-byte aligned base and, with rows padded to 16 bytes, from a base 1 byte past
one.  ``VEC = 16`` frames have base and rows 16-byte aligned.  ``EXTRA`` holds
named launches with the property each was committed for (its ``props``).

``tiling()`` / ``launch_cfg()`` restate ``general_group``
(csrc/batch_layout.cpp) and ``resample_smem_bytes`` over the product's tap
tables (``capi.axis_taps``); tests/test_general_shapes.py holds them to what
``build_layout`` itself gives (tests/cpp/general_layout_unit.cpp), so the
table's properties are the planner's, not this module's.

Everything here is host only.
"""
import functools
import os
import re
import sys

if __name__ == "__main__":  # (run as a script: the package is found from the repository tree)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlx-data_amd"))

from mlx_data_amd import capi
from wave_shapes import dst_pad, whole, windows  # noqa: F401  (windows: the four entries every frame is run as)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlx-data_amd", "csrc")
RESAMPLE_HIP = os.path.join(CSRC, "resample.hip")
INTERNAL_H = os.path.join(CSRC, "capi_internal.h")
RESAMPLE_H = os.path.join(CSRC, "resample.h")
LAYOUT_CPP = os.path.join(CSRC, "batch_layout.cpp")

POLICY = capi.MXD_POLICY_NO_WAVE  # neither a wave nor a band kernel: every image is the general kernel's

# ---- search bounds -----------------------------------------------------------
ROWS = (20, 37)    # output rows of shape (a) / (b)
MAX_SRC_W = 2048   # source columns


def instantiations(path=RESAMPLE_HIP):
    """The (VEC, C, F32, ALPHA) keys resample.hip instantiates."""
    text = open(path).read()
    cases = re.findall(r"case (\d+): return launch_t<VEC, (\d), (true|false)>\(cfg", text)
    assert cases and "switch (cfg.channels * 2 + (cfg.f32 ? 1 : 0))" in text, (
        "resample.hip: launch_v no longer reads as launch_t cases")
    for n, c, f in cases:
        assert int(n) == int(c) * 2 + (f == "true"), ("resample.hip: launch_v case", n, c, f)
    vecs = [int(a) for a, b in re.findall(r"if \(cfg\.vec == (\d+)\) return launch_v<(\d+)>\(cfg", text) if a == b]
    assert vecs, "resample.hip: launch_resample no longer reads as cfg.vec cases"
    alpha = re.search(r"if constexpr \(C == (\d)\) \{\s*if \(cfg\.alpha\) \{\s*hipLaunchKernelGGL\(\(resample_tiles<VEC, "
                      r"C, F32, true>\)", text)
    assert alpha and text.count("resample_tiles<VEC, C, F32, true>") == 1 and \
        text.count("resample_tiles<VEC, C, F32, false>") == 1, "resample.hip: launch_t no longer reads as expected"
    keys = {(v, int(c), f == "true", False) for v in vecs for _, c, f in cases}
    keys |= {(v, int(alpha.group(1)), f, True) for v in vecs for f in (False, True)}
    return keys


@functools.lru_cache(None)
def constants():
    """kTileRows, kStripBytes, kLdsBudget, kTapHeader, kMinTabWidth and the LDS
    bound of general_group (bytes), read out of the sources."""
    out = {}
    for path, names in ((INTERNAL_H, ("kTileRows", "kStripBytes", "kLdsBudget")),
                        (RESAMPLE_H, ("kTapHeader", "kMinTabWidth"))):
        text = open(path).read()
        for name in names:
            m = re.search(r"constexpr int(?:32_t)? %s = ([0-9* ]+);" % name, text)
            assert m, (path, name)
            out[name] = eval(m.group(1))
    m = re.search(r"resample_smem_bytes\(cfg\) > ([0-9* ]+)\) return fail\(MXD_ERR_UNSUPPORTED, "
                  r"\"mxd: tile does not fit in LDS\"\)", open(LAYOUT_CPP).read())
    assert m, "batch_layout.cpp: general_group's LDS bound no longer reads as expected"
    out["kLdsMax"] = eval(m.group(1))
    return out


@functools.lru_cache(256)
def taps(n_in, n_out, filter=0):
    """(first, count, padded width) of the whole axis, as TableCache keeps them."""
    if n_in == n_out:
        filter = 0
    first, cnt, w = capi.axis_taps(n_in, n_out, filter=filter)
    return first, cnt, max(w.shape[1], constants()["kMinTabWidth"])


def strip_chunks(first, cnt, cx, cw, ox0, ox1, flip, c, vec):
    xa = cw - ox1 if flip else ox0
    xb = cw - 1 - ox0 if flip else ox1 - 1
    lo = int(first[cx + xa])
    hi = int(first[cx + xb] + cnt[cx + xb]) - 1
    fb0 = (lo * c) & ~(vec - 1)
    return ((hi + 1) * c - fb0 + vec - 1) // vec


def tiling(shape, g, vec, filter=0):
    """general_group's tiling of geometry g on an (h, w, c) source."""
    k = constants()
    h, w, c = shape
    rw, rh, cx, cy, cw, ch, flip = g
    first, cnt, xw = taps(w, rw, filter)
    _, _, yw = taps(h, rh, filter)
    full = strip_chunks(first, cnt, cx, cw, 0, cw, flip, c, 1)
    nstrips = max(1, -(-full // k["kStripBytes"]))
    tx = -(-cw // nstrips)
    tx = min(cw, (tx + 3) & ~3)
    nstrips = -(-cw // tx)
    chunks = max(strip_chunks(first, cnt, cx, cw, s * tx, min(s * tx + tx, cw), flip, c, vec) for s in range(nstrips))
    vw = (chunks * vec + 3) & ~3
    ty = min(k["kTileRows"], ch)
    group = max(1, min(8, 512 // max(1, chunks)))
    by_budget = k["kLdsBudget"] // (vw * 4)
    group = min(max(1, min(group, by_budget)), ty)
    nbands = -(-ch // ty)
    return dict(nstrips=nstrips, tx=tx, ty=ty, group=group, vw=vw, nbands=nbands, ntiles=nbands * nstrips, xw=xw, yw=yw,
                by_budget=by_budget, last_tx=cw - (nstrips - 1) * tx, last_ty=ch - (nbands - 1) * ty)


def launch_cfg(tilings):
    """ntiles, tile_begin of every image and resample_smem_bytes of a launch."""
    k = constants()
    mx = {f: max(t[f] for t in tilings) for f in ("tx", "ty", "xw", "yw", "vw", "group")}
    xs, ys = k["kTapHeader"] + mx["xw"], k["kTapHeader"] + mx["yw"]
    x_off = mx["group"] * mx["vw"]
    y_off = x_off + ((mx["tx"] * xs + 3) & ~3)
    begins, n = [], 0
    for t in tilings:
        begins.append(n)
        n += t["ntiles"]
    return dict(ntiles=n, tile_begin=begins, smem=(y_off + mx["ty"] * ys) * 4)


# ---- source layouts ----------------------------------------------------------
# name -> (base bytes past a 16-byte boundary, rows padded to 16 bytes); the VEC each gives is vec_of
LAYOUTS = {"aligned": (0, True), "packed": (0, False), "base1": (1, True)}


def src_stride(w, c, layout):
    return (w * c + 15) // 16 * 16 if LAYOUTS[layout][1] else w * c


def vec_of(w, c, layout):
    return 16 if (LAYOUTS[layout][0] | src_stride(w, c, layout)) % 16 == 0 else 1


def layouts_of(vec):
    return ("aligned",) if vec == 16 else ("packed", "base1")


def entry(shape, g, layout="aligned", f32=False, filter=0, rgba_weighted=0):
    """The mxd_image fields of geometry g on an (h, w, c) source (addresses are placeholders)."""
    h, w, c = shape
    rw, rh, cx, cy, cw, ch, flip = g
    return dict(src=4096 + LAYOUTS[layout][0], src_stride=src_stride(w, c, layout), src_w=w, src_h=h, channels=c,
                resize_w=rw, resize_h=rh, crop_x=cx, crop_y=cy, crop_w=cw, crop_h=ch, flip=int(flip), dst=4096,
                dst_stride=cw * c * (4 if f32 else 1) + dst_pad(f32), filter=capi.FILTERS.get(filter, filter),
                rgba_weighted=int(rgba_weighted))


def is_general(shape, g, layout="aligned", f32=False, filter=0):
    """Under POLICY neither mxd_describe_plan nor mxd_describe_band_plan takes the image."""
    prev = capi.set_kernel_policy(POLICY)
    try:
        e = entry(shape, g, layout, f32, filter)
        dt = capi.MXD_F32_DIV255 if f32 else capi.MXD_U8
        return capi.describe_plan(e, dt)["wave"] == 0 and capi.describe_band_plan(e, dt)["band"] == 0
    finally:
        capi.set_kernel_policy(prev)


# ---- the search --------------------------------------------------------------
def fits(key, which, frame):
    """Whether the whole frame has the property shape `which` (0: a, 1: b) of `key` is committed for."""
    vec, c, _ = key
    sw, sh, cw, ch = frame
    if ch != ROWS[which] or sh != 2 * ch + 1 or not 2 * cw < sw <= 3 * cw:
        return False
    if vec == 1 and (sw * c) % 16 == 0:
        return False
    for layout in layouts_of(vec):
        if vec_of(sw, c, layout) != vec:
            return False
        for flip in (0, 1):
            t = tiling((sh, sw, c), whole(cw, ch, flip), vec)
            if which == 0:
                ok = t["ntiles"] == 1
            else:
                ok = (t["nstrips"] >= 2 and t["last_tx"] < t["tx"] and t["nbands"] == 2 and 0 < t["last_ty"] < t["ty"]
                      and t["group"] < t["ty"] and (c == 4 or (cw * c) % 4 != 0))
            if not ok:
                return False
    return True


def find(key, which):
    """The first frame that fits, by source columns, then output columns."""
    ch = ROWS[which]
    c = key[1]
    lo = 17 if which == 0 else constants()["kStripBytes"] // c
    for sw in range(lo, MAX_SRC_W + 1):
        for cw in range(-(-sw // 3), (sw - 1) // 2 + 1):
            if cw >= 8 and fits(key, which, (sw, 2 * ch + 1, cw, ch)):
                return (sw, 2 * ch + 1, cw, ch)
    return None


# (VEC, C, ALPHA) -> the two whole frames (src w, src h, out w, out h)
SHAPES = {
    (1, 1, False): ((17, 41, 8, 20), (1537, 75, 513, 37)),
    (1, 2, False): ((17, 41, 8, 20), (769, 75, 257, 37)),
    (1, 3, False): ((17, 41, 8, 20), (513, 75, 171, 37)),
    (1, 4, False): ((17, 41, 8, 20), (385, 75, 129, 37)),
    (1, 4, True): ((17, 41, 8, 20), (385, 75, 129, 37)),
    (16, 1, False): ((17, 41, 8, 20), (1537, 75, 513, 37)),
    (16, 2, False): ((17, 41, 8, 20), (769, 75, 257, 37)),
    (16, 3, False): ((17, 41, 8, 20), (513, 75, 171, 37)),
    (16, 4, False): ((17, 41, 8, 20), (385, 75, 129, 37)),
    (16, 4, True): ((17, 41, 8, 20), (385, 75, 129, 37)),
}

def key_id(key):
    return "v%d_c%d%s" % (key[0], key[1], "_alpha" if key[2] else "")


def seed_of(key, which):
    """The gpu_util.synth seed of a key's first (0) / second (1) shape or of an EXTRA image."""
    if (key, which) in SEEDS:
        return SEEDS[key, which]
    base = 200 + key[0] + 10 * key[1] + (5 if key[2] else 0) if isinstance(key, tuple) else 300 + 3 * len(key)
    return base + 7 * which


def alpha_holes(img):
    """tests/test_gpu_rgba.rgba's alpha plane on an (h, w, 4) image: a fully
    transparent block, a faint region, opaque columns."""
    h, w = img.shape[:2]
    a = img[:, :, 3]
    a[: h // 3, : w // 3] = 0
    a[h // 2:, w // 2:] //= 4
    a[:, ::7] = 255
    return img


def alpha_edges(img):
    """An alpha plane of hard edges on an (h, w, 4) image: opaque, with a fully
    transparent rectangle in the middle.  Under a filter with negative lobes
    the output pixels just inside the rectangle get a negative filtered alpha."""
    h, w = img.shape[:2]
    img[:, :, 3] = 255
    img[h // 4:h - h // 4, w // 4:w - w // 4, 3] = 0
    return img


ALPHA_PLANES = {"holes": alpha_holes, "edges": alpha_edges}


def filtered_alpha(img, g, filter=0):
    """The filtered alpha (float64, 1 = opaque) of every output pixel of geometry g."""
    import numpy as np

    rw, rh, cx, cy, cw, ch, flip = g
    h, w = img.shape[:2]

    def dense(n_in, n_out, off, length):
        first, cnt, wt = capi.axis_taps(n_in, n_out, filter=filter)
        m = np.zeros((length, n_in))
        for j in range(length):
            o = off + j
            m[j, first[o]:first[o] + cnt[o]] = wt[o, :cnt[o]]
        return m

    a = dense(h, rh, cy, ch) @ (img[:, :, 3].astype(np.float64) / 255.0) @ dense(w, rw, cx, cw).T
    return a[:, ::-1] if flip else a


# ---- the named launches --------------------------------------------------------
def _both(sw, sh, cw, ch):
    """The whole frame and its mirror image."""
    return [((sw, sh), whole(cw, ch)), ((sw, sh), whole(cw, ch, 1))]


def _windows(sw, sh, cw, ch):
    return [((sw, sh), g) for g in windows(cw, ch)]


def _taps(sw):
    """16 columns at 2.5 : 1 (sw = 41) over vertical tables of 1 tap (a crop-only axis), 1 and 2 (upsampling),
    3 and 4, 5 to 7, 7 to 9 taps."""
    return [((sw, sh), (16, 20, 0, 0, 16, 20, k % 2)) for k, sh in enumerate((20, 9, 30, 50, 70))]


_ALIGNED_AND_NOT = {"aligned": 16, "packed": 1, "base1": 1}
_MIX = [((1400, 1260), whole(80, 70)), ((41, 41), (16, 20, 0, 0, 16, 20, 1)), ((2000, 1400), (100, 70, 3, 20, 95, 27, 0))]
_TILES = {1: ((41, 41), whole(16, 20)), 2: ((43, 75), whole(16, 37, 1)), 3: ((170, 150), whole(64, 70))}
_KIB = 1024

# name -> the launch: `c` channels; `images` [((src w, src h), geometry)] in batch order, geometries (resize w,
# resize h, crop x, crop y, crop w, crop h, flip); `layouts`, one launch each: a source layout for every image or
# one per image; `props`, what tests/test_general_shapes.py asserts of its tiling; and, where they apply,
# `weighted` (rgba_weighted per image), `plane` (the alpha plane of the weighted images, a name of ALPHA_PLANES;
# "holes" without one), `filter`, `dsts` (destination layouts of tests/test_gpu_general_shapes.py), `refused`,
# `transparent`, `negative_alpha`, `deep`.
EXTRA = {
    # vertical tap counts: every remainder of the 4-way unrolled loop
    "taps_c1": dict(c=1, images=_taps(41), layouts=("aligned", "packed"),
                    props=dict(ytaps_mod4=(1, 2, 3, 5), vec=_ALIGNED_AND_NOT)),
    "taps_c4": dict(c=4, images=_taps(41), layouts=("aligned", "packed"),
                    props=dict(ytaps_mod4=(1, 2, 3, 5), vec=_ALIGNED_AND_NOT)),
    # rows that end in 1, 2, 3 and 4 elements, destinations off and on the vector stores' alignment
    "stores_c1": dict(c=1, images=[((sw, 41), whole(cw, 20, cw % 2)) for sw, cw in ((33, 13), (35, 14), (38, 15), (41, 16))],
                      layouts=("aligned",), dsts=("off", "vec", "odd"), props=dict(row_end=(0, 1, 2, 3))),
    "stores_c3": dict(c=3, images=[((sw, 41), whole(cw, 20, cw % 2)) for sw, cw in ((13, 5), (15, 6), (18, 7), (20, 8))],
                      layouts=("aligned", "packed"), dsts=("off", "vec", "odd"), props=dict(row_end=(0, 1, 2, 3))),
    # images whose tx, ty, xwidth, ywidth, vw and group all differ; then one image of them unaligned
    "mixed_c2": dict(c=2, images=_MIX, layouts=("aligned", ("base1", "aligned", "aligned"), ("aligned", "aligned", "base1")),
                     props=dict(all_differ=("tx", "ty", "xw", "yw", "vw", "group"), vec=_ALIGNED_AND_NOT)),
    "mixed_c2_reversed": dict(c=2, images=_MIX[::-1],
                              layouts=("aligned", ("aligned", "base1", "aligned")),
                              props=dict(all_differ=("tx", "ty", "xw", "yw", "vw", "group"), vec=_ALIGNED_AND_NOT)),
    # tile counts below, at and off a multiple of the 8 XCDs
    "tiles_1": dict(c=1, images=[_TILES[1]], layouts=("aligned", "packed"), props=dict(ntiles=1)),
    "tiles_7": dict(c=1, images=[_TILES[k] for k in (3, 2, 2)], layouts=("aligned", "packed"), props=dict(ntiles=7)),
    "tiles_8": dict(c=1, images=[_TILES[k] for k in (3, 2, 3)], layouts=("aligned", "packed"), props=dict(ntiles=8)),
    "tiles_9": dict(c=1, images=[_TILES[k] for k in (1, 3, 2, 3)], layouts=("aligned", "packed"), props=dict(ntiles=9)),
    "tiles_15": dict(c=1, images=[_TILES[k] for k in (3, 2, 3, 2, 3, 2)], layouts=("aligned", "packed"),
                     props=dict(ntiles=15)),
    # deep ratios: 100 : 1 (LDS up to 64 KiB), 250 : 1 (64 to 160 KiB), 649 : 1 (refused), and horizontally
    # 1500 : 1 (a 4-column strip's footprint leaves kLdsBudget one row) and 2400 : 1 (not even one)
    "deep_v_100": dict(c=1, deep=True, images=_both(16, 3700, 16, 37), layouts=("aligned",),
                       props=dict(smem=(0, 64 * _KIB))),
    "deep_v_250": dict(c=1, deep=True, images=_both(16, 9250, 16, 37), layouts=("aligned",),
                       props=dict(smem=(64 * _KIB, 160 * _KIB))),
    "deep_v_649": dict(c=1, deep=True, refused=True, images=_both(16, 24000, 16, 37), layouts=("aligned",), props={}),
    "deep_h_1500": dict(c=1, deep=True, images=_both(12000, 25, 8, 12), layouts=("aligned",),
                        props=dict(by_budget=1, group=1, strips=2, smem=(64 * _KIB, 160 * _KIB))),
    "deep_h_2400": dict(c=1, deep=True, images=_both(19200, 21, 8, 10), layouts=("aligned",),
                        props=dict(by_budget=0, group=1, strips=2, smem=(64 * _KIB, 160 * _KIB))),
    # the weighted form: two strips, every window, exactly transparent output pixels
    "rgba_weighted": dict(c=4, images=_windows(385, 75, 129, 37), weighted=[1] * 4, transparent=True,
                          layouts=("aligned", "packed", "base1"), props=dict(strips=2, vec=_ALIGNED_AND_NOT)),
    # the weighted form over Catmull-Rom tables: output pixels of negative filtered alpha (below kTinyAlpha and
    # not 0) keep their premultiplied colours
    "rgba_weighted_cubic": dict(c=4, filter="catmullrom", images=_windows(385, 75, 129, 37), weighted=[1] * 4,
                                plane="edges", negative_alpha=True, layouts=("aligned", "packed", "base1"),
                                props=dict(strips=2, vec=_ALIGNED_AND_NOT)),
    # weighted and unweighted images interleaved in one call: split_batch makes two launches
    "rgba_interleaved": dict(c=4, images=_both(385, 75, 129, 37) + _both(101, 41, 40, 20), weighted=[1, 0, 0, 1],
                             layouts=("aligned", "packed"), props=dict(vec=_ALIGNED_AND_NOT)),
    # cubic tables: negative weights, four channels; and past the 32 weights every entry is padded to
    "cubic_c4": dict(c=4, filter="catmullrom", images=_windows(101, 99, 40, 37), layouts=("aligned", "packed"),
                     props=dict(vec=_ALIGNED_AND_NOT)),
    "cubic_c1_37_taps": dict(c=1, filter="catmullrom", images=_windows(361, 333, 40, 37), layouts=("aligned", "packed"),
                             props=dict(xtaps_over=32, vec=_ALIGNED_AND_NOT)),
}

# (key or EXTRA name, index) -> seed, where the default seed's image does not pass the +-1 / 2e-3 gate
# between the two references (tests/test_general_shapes.py)
SEEDS = {
}


def main():
    for key in sorted({(v, c, a) for v, c, _, a in instantiations()}):
        print(f"    {key}: ({find(key, 0)}, {find(key, 1)}),", flush=True)


if __name__ == "__main__":
    main()
