"""The band kernels of mlx-data_amd/csrc/band.hip, one shape each.

``instantiations()`` reads the kernel list out of the source: the ``{taps, db,
s}`` classes of ``kBandClasses[]`` (csrc/band.h) times the window sizes ``NQ``
of ``pick_nq`` (csrc/band.hip); a key is ``(taps, nq)`` -- ``taps`` names the
class, and ``capi.describe_band_plan`` reports ``taps, db, s, nq``.  Each key
is built for u8 and for q/255 f32 output.  ``find(key, strips)`` searches, with
the host-only ``describe_band_plan`` under ``MXD_POLICY_PREFER_BAND``, for the
smallest whole-frame resize ``(src_w, src_h, out_w, out_h)`` whose plan is
exactly that key in u8 and in f32: once in one strip at about 20 output rows,
once in two strips at 68 rows and 64 columns or more.  ``SHAPES`` is the
committed result with the strip count of each frame (``python
tests/band_shapes.py [key ...]`` prints the entries again when a class is
added), ``UNREACHABLE`` the keys no frame plans with the condition of
``band_plan_image`` (csrc/band_plan.cpp) that rules them out, and ``EXTRA`` the
anisotropic cases of every key: the class follows the horizontal taps alone, so
an ``image_resize(w, h)`` with another vertical ratio keeps the key while an
output row's new source rows fill several groups (``deep``) or less than one
(``flat``).

Everything here is host only.  Sources are laid out as
tests/test_gpu_band_shapes.py lays them out: rows at the smallest pitch the
band kernel takes (``w * 3`` rounded up to 4).  Output height follows the
source's aspect (``wave_shapes.out_h``) except in ``EXTRA``; it is never a
multiple of 8 and always above 16.
"""
import os
import re

from mlx_data_amd import capi
from wave_shapes import dst_pad, out_h, whole

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlx-data_amd", "csrc")
BAND_H = os.path.join(CSRC, "band.h")
BAND_HIP = os.path.join(CSRC, "band.hip")

# ---- search bounds (find, and the bounded rerun of tests/test_band_shapes.py) --
ROWS_ONE = (20, 19, 21, 18, 22, 17, 23)  # output rows tried for the one-strip shape, in this order
ROWS_TWO = (68, 67, 69, 66, 70, 65, 71)  # ... and for the two-strip shape (the +-1 gate applies from 64)
MIN_RATIO = 0.5                          # source rows (columns) per output row (column): a 2x upscale ...
MAX_RATIO = 16                           # ... to the deepest class
MAX_COLS = 768                           # output columns: three strips of kBandThreads
EXTRA_ROWS = 68                          # output rows of the EXTRA frames
SHIFTS = (0, 1, 2, 3)                    # source base offsets (bytes past a 4-byte boundary)


def classes(path=BAND_H):
    """{taps: (db, s)} of kBandClasses[]."""
    text = open(path).read()
    m = re.search(r"kBandClasses\[\]\s*=\s*\{(.*?)\};", text, re.S)
    assert m, "band.h: no kBandClasses[] initialiser"
    triples = re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}", m.group(1))
    assert triples, "band.h: kBandClasses[] no longer reads as {taps, db, s} triples"
    out = {int(t): (int(db), int(s)) for t, db, s in triples}
    assert len(out) == len(triples), "band.h: two classes with the same taps"
    return out


def window_sizes(path=BAND_HIP):
    """The NQ cases of pick_nq."""
    text = open(path).read()
    m = re.search(r"BandKernel pick_nq\(.*?\n\}", text, re.S)
    assert m, "band.hip: no pick_nq"
    nqs = [int(a) for a, b in re.findall(r"case (\d+): return pick_class<C, F32, (\d+)>", m.group(0)) if a == b]
    assert nqs, "band.hip: pick_nq no longer reads as pick_class cases"
    return nqs


def instantiations(band_h=BAND_H, band_hip=BAND_HIP):
    """The (taps, nq) keys band.hip instantiates (each for u8 and f32)."""
    return {(t, q) for t in classes(band_h) for q in window_sizes(band_hip)}


def src_stride(w):
    """The smallest row pitch the band kernel takes."""
    return (w * 3 + 3) // 4 * 4


def entry(shape, g, shift=0, f32=False, filter=0):
    """The mxd_image fields of geometry g on an (h, w, 3) source, laid out as
    tests/test_gpu_band_shapes.py lays it out."""
    h, w, c = shape
    rw, rh, cx, cy, cw, ch, flip = g
    return dict(src=256 + shift, src_stride=src_stride(w), src_w=w, src_h=h, channels=c, resize_w=rw, resize_h=rh,
                crop_x=cx, crop_y=cy, crop_w=cw, crop_h=ch, flip=int(flip), dst=256,
                dst_stride=cw * c * (4 if f32 else 1) + dst_pad(f32), filter=capi.FILTERS.get(filter, filter))


def plan(shape, g, shift=0, f32=False, filter=0, policy=capi.MXD_POLICY_PREFER_BAND):
    prev = capi.set_kernel_policy(policy)
    try:
        return capi.describe_band_plan(entry(shape, g, shift, f32, filter), capi.MXD_F32_DIV255 if f32 else capi.MXD_U8)
    finally:
        capi.set_kernel_policy(prev)


def key_of(p):
    """The instantiation a describe_band_plan result names (None: no band kernel)."""
    return (p["taps"], p["nq"]) if p["band"] else None


def planned(key, shape, g, shifts=(0,)):
    """(every plan of g is `key` with the class's db and s, the strip count)
    over u8 / f32 and the shifts."""
    db, s = classes()[key[0]]
    ns = set()
    for shift in shifts:
        for f32 in (False, True):
            p = plan(shape, g, shift, f32)
            if key_of(p) != key or (p["db"], p["s"]) != (db, s):
                return False, None
            ns.add(p["nstrips"])
    return len(ns) == 1, ns.pop()


def tiny_windows(cw, ch):
    """Windows whose bands are shorter than the stream's la + 2 groups: one
    pixel, 3 x 2 mirrored, a full-width row and a full-height column."""
    return [(cw, ch, cw // 2, ch // 2, 1, 1, 0), (cw, ch, min(2, cw - 3), 3, 3, 2, 1), (cw, ch, 0, ch // 3, cw, 1, 0),
            (cw, ch, cw - 1, 0, 1, ch, 1)]


def new_rows(sh, ch):
    """(fewest, most) source rows new for one output row of an sh -> ch resize."""
    first, cnt, _ = capi.axis_taps(sh, ch)
    last = first + cnt - 1
    d = last[1:] - last[:-1]
    return int(d.min()), int(d.max())


def _ratios(taps):
    """Horizontal ratios (source per output column) worth planning for a class:
    a triangle's taps are about 2 r + 1, and the class takes the tap counts
    above the next smaller class's."""
    below = max([t for t in classes() if t < taps], default=0)
    return max(MIN_RATIO, (below - 3) / 2), min(MAX_RATIO, taps / 2 + 0.5)


def find(key, strips, rows=None, max_cols=MAX_COLS):
    """The first whole-frame (src_w, src_h, out_w, out_h), by output rows in
    the order of ROWS_ONE / ROWS_TWO, then source height, then output width,
    whose plan is `key` in u8 and f32 -- for strips == 2 from every base
    offset of SHIFTS, at 64 columns or more.  A frame in exactly `strips`
    strips ends the search; without one, the frame of the first row count that
    has any: in the fewest strips above `strips`, else (two asked for, and the
    planner only ever gives the key one) in one.  Frames keep the source's
    aspect.  Where no frame of 64 columns plans the key (the window of 64
    columns at the class's ratio is past nq KiB), the second shape is the
    68-row frame from 8 columns on.  None when nothing inside the bounds plans
    the key."""
    hit = _find(key, strips, rows, max_cols, 64 if strips == 2 else 8)
    if hit is None and strips == 2:
        hit = _find(key, strips, rows, 63, 8)
    return hit


def _find(key, strips, rows, max_cols, min_cols):
    lo, hi = _ratios(key[0])
    best = None
    for ch in rows or (ROWS_TWO if strips == 2 else ROWS_ONE):
        for sh in range(max(2, int(ch * lo)), int(ch * hi) + 2):
            for cw in range(min_cols, max_cols + 1):
                sw = round(sh * cw / ch)
                if sw < 1 or out_h(sw, sh, cw) != ch:
                    continue
                if key_of(plan((sh, sw, 3), whole(cw, ch))) != key:
                    continue
                ok, ns = planned(key, (sh, sw, 3), whole(cw, ch), SHIFTS if strips == 2 else (0,))
                if not ok:
                    continue
                if ns == strips:
                    return (sw, sh, cw, ch)
                rank = ns if ns > strips else 1 << 20  # more strips before fewer, the fewest of them first
                if best is None or rank < best[0]:
                    best = (rank, (sw, sh, cw, ch))
        if best is not None:
            return best[1]
    return None


def find_extra(key, kind):
    """(src w, src h), (out w, out h): the horizontal resize of the key's
    two-strip shape at EXTRA_ROWS output rows with the nearest source height
    that still plans the key and whose vertical table is `kind`:
    "deep" -- some output row brings more new source rows than the class's db
    (several groups per row); "flat" -- every output row brings fewer than db
    (db = 1: some row brings none, a vertical upscale)."""
    db, _ = classes()[key[0]]
    sw, _, cw, _, _ = SHAPES[key][1]
    ch = EXTRA_ROWS
    if kind == "deep":
        heights = range(ch * db, ch * (MAX_RATIO + 1))
    else:
        heights = [h for d in range(1, ch) for h in (ch + d, ch - d) if h >= ch * MIN_RATIO] + [ch]  # 1 : 1 last
    for sh in heights:
        lo, hi = new_rows(sh, ch)
        if (hi > db) if kind == "deep" else (hi < db or (db == 1 and lo == 0)):
            if planned(key, (sh, sw, 3), whole(cw, ch), SHIFTS)[0]:
                return (sw, sh), (cw, ch)
    return None


# key -> two whole frames (src w, src h, out w, out h, strips): about 20 rows in one strip, and 68 rows
# and 64 columns or more in two strips
SHAPES = {
    (2, 1): ((6, 12, 10, 20, 1), (166, 44, 257, 68, 2)),
    (4, 1): ((32, 21, 30, 20, 1), (261, 69, 257, 68, 2)),
    (4, 2): ((339, 27, 251, 20, 1), (670, 89, 512, 68, 2)),
    (6, 1): ((23, 41, 11, 20, 1), (518, 137, 257, 68, 2)),
    (6, 2): ((338, 41, 165, 20, 1), (669, 137, 332, 68, 2)),
    (6, 3): ((678, 53, 256, 20, 1), (1350, 180, 510, 68, 2)),
    (8, 1): ((92, 61, 30, 20, 1), (308, 205, 102, 68, 1)),
    (8, 2): ((336, 61, 110, 20, 1), (775, 205, 257, 68, 2)),
    (8, 3): ((677, 61, 222, 20, 1), (1348, 205, 447, 68, 2)),
    (8, 4): ((1020, 80, 255, 20, 1), (2029, 270, 511, 68, 2)),
    (10, 1): ((45, 81, 11, 20, 1), (257, 273, 64, 68, 1)),
    (10, 2): ((336, 81, 83, 20, 1), (1016, 273, 253, 68, 2)),
    (10, 3): ((676, 81, 167, 20, 1), (1341, 273, 334, 68, 2)),
    (12, 1): ((152, 101, 30, 20, 1), (322, 342, 64, 68, 1)),
    (12, 2): ((333, 101, 66, 20, 1), (672, 341, 134, 68, 2)),
    (17, 1): ((67, 121, 11, 20, 1), (211, 409, 35, 68, 1)),
    (17, 2): ((327, 121, 54, 20, 1), (1010, 409, 168, 68, 2)),
    (17, 3): ((672, 121, 111, 20, 1), (1323, 409, 220, 68, 2)),
    (25, 1): ((94, 170, 11, 20, 1), (94, 578, 11, 68, 1)),
    (25, 2): ((332, 170, 39, 20, 1), (672, 578, 79, 68, 2)),
    (32, 1): ((138, 250, 11, 20, 1), (138, 850, 11, 68, 1)),
    (32, 2): ((338, 250, 27, 20, 1), (838, 850, 67, 68, 2)),
}

# key -> the condition of band_plan_image (csrc/band_plan.cpp) that keeps every frame off it
_NO_DOWNSCALE = ("xw <= 2 holds up to a horizontal ratio of 257 : 256, so a strip of kBandThreads columns has "
                 "need <= 789 bytes and nq = ceil(need / kBandChunk) is 1")
_UP_TO_2 = "xw <= 4 holds up to 2 : 1, so a strip of kBandThreads columns has need <= 1560 bytes and nq <= 2"
_UP_TO_3 = "xw <= 6 holds up to 3 : 1, so a strip of kBandThreads columns has need <= 2337 bytes and nq <= 3"
_DB5 = "max_nq = kAreaCap / (max(db, 4) * kBandChunk) = 16 / 5 = 3 for db = 5: `nq <= max_nq` takes more strips instead"
_DB6 = "max_nq = kAreaCap / (max(db, 4) * kBandChunk) = 16 / 6 = 2 for db = 6: `nq <= max_nq` takes more strips instead"
_DB8 = "max_nq = kAreaCap / (max(db, 4) * kBandChunk) = 16 / 8 = 2 for db = 8: `nq <= max_nq` takes more strips instead"
UNREACHABLE = {
    (2, 2): _NO_DOWNSCALE,
    (2, 3): _NO_DOWNSCALE,
    (2, 4): _NO_DOWNSCALE,
    (4, 3): _UP_TO_2,
    (4, 4): _UP_TO_2,
    (6, 4): _UP_TO_3,
    (10, 4): _DB5,
    (12, 3): _DB6,
    (12, 4): _DB6,
    (17, 4): _DB5,
    (25, 3): _DB6,
    (25, 4): _DB6,
    (32, 3): _DB8,
    (32, 4): _DB8,
}

# name -> (key it must land on, (src w, src h), (out w, out h)): find_extra's frames
EXTRA = {
    "t2_q1_deep": ((2, 1), (166, 70), (257, 68)),
    "t2_q1_flat": ((2, 1), (166, 67), (257, 68)),
    "t4_q1_deep": ((4, 1), (261, 137), (257, 68)),
    "t4_q1_flat": ((4, 1), (261, 69), (257, 68)),
    "t4_q2_deep": ((4, 2), (670, 137), (512, 68)),
    "t4_q2_flat": ((4, 2), (670, 69), (512, 68)),
    "t6_q1_deep": ((6, 1), (518, 206), (257, 68)),
    "t6_q1_flat": ((6, 1), (518, 69), (257, 68)),
    "t6_q2_deep": ((6, 2), (669, 206), (332, 68)),
    "t6_q2_flat": ((6, 2), (669, 69), (332, 68)),
    "t6_q3_deep": ((6, 3), (1350, 206), (510, 68)),
    "t6_q3_flat": ((6, 3), (1350, 69), (510, 68)),
    "t8_q1_deep": ((8, 1), (308, 273), (102, 68)),
    "t8_q1_flat": ((8, 1), (308, 69), (102, 68)),
    "t8_q2_deep": ((8, 2), (775, 273), (257, 68)),
    "t8_q2_flat": ((8, 2), (775, 69), (257, 68)),
    "t8_q3_deep": ((8, 3), (1348, 273), (447, 68)),
    "t8_q3_flat": ((8, 3), (1348, 69), (447, 68)),
    "t8_q4_deep": ((8, 4), (2029, 273), (511, 68)),
    "t8_q4_flat": ((8, 4), (2029, 69), (511, 68)),
    "t10_q1_deep": ((10, 1), (257, 342), (64, 68)),
    "t10_q1_flat": ((10, 1), (257, 69), (64, 68)),
    "t10_q2_deep": ((10, 2), (1016, 342), (253, 68)),
    "t10_q2_flat": ((10, 2), (1016, 69), (253, 68)),
    "t10_q3_deep": ((10, 3), (1341, 342), (334, 68)),
    "t10_q3_flat": ((10, 3), (1341, 69), (334, 68)),
    "t12_q1_deep": ((12, 1), (322, 409), (64, 68)),
    "t12_q1_flat": ((12, 1), (322, 69), (64, 68)),
    "t12_q2_deep": ((12, 2), (672, 409), (134, 68)),
    "t12_q2_flat": ((12, 2), (672, 69), (134, 68)),
    "t17_q1_deep": ((17, 1), (211, 342), (35, 68)),
    "t17_q1_flat": ((17, 1), (211, 69), (35, 68)),
    "t17_q2_deep": ((17, 2), (1010, 342), (168, 68)),
    "t17_q2_flat": ((17, 2), (1010, 69), (168, 68)),
    "t17_q3_deep": ((17, 3), (1323, 342), (220, 68)),
    "t17_q3_flat": ((17, 3), (1323, 69), (220, 68)),
    "t25_q1_deep": ((25, 1), (94, 409), (11, 68)),
    "t25_q1_flat": ((25, 1), (94, 69), (11, 68)),
    "t25_q2_deep": ((25, 2), (672, 409), (79, 68)),
    "t25_q2_flat": ((25, 2), (672, 69), (79, 68)),
    "t32_q1_deep": ((32, 1), (138, 545), (11, 68)),
    "t32_q1_flat": ((32, 1), (138, 69), (11, 68)),
    "t32_q2_deep": ((32, 2), (838, 545), (67, 68)),
    "t32_q2_flat": ((32, 2), (838, 69), (67, 68)),
}

# name of an EXTRA case no frame gives -> why
NO_EXTRA = {
}

# (key, 0 / 1 for the key's first / second shape or an EXTRA name) -> seed, where the default seed's
# image does not pass the +-1 / 2e-3 gate between the two references (tests/test_band_shapes.py)
SEEDS = {
}


def seed_of(key, which):
    """The gpu_util.synth seed of a key's first (0) / second (1) shape or of an EXTRA case."""
    if (key, which) in SEEDS:
        return SEEDS[key, which]
    return 100 + sum(key) + (7 * which if isinstance(which, int) else 3 * len(which))


def main():
    """Prints the SHAPES / EXTRA entries of the keys given as arguments (all of band.hip's without any)."""
    import sys
    import time

    def strips(key, k, shape):
        if shape is None:
            return None
        sw, sh, cw, ch = shape
        return shape + (planned(key, (sh, sw, 3), whole(cw, ch), SHIFTS if k else (0,))[1],)

    only = [eval(a) for a in sys.argv[1:]]
    for key in sorted(only or instantiations()):
        t = time.time()
        one, two = strips(key, 0, find(key, 1)), strips(key, 1, find(key, 2))
        print(f"    {key}: ({one}, {two}),  # {time.time() - t:.0f} s", flush=True)
    for key in sorted(only or SHAPES):
        if key in SHAPES:
            for kind in ("deep", "flat"):
                hit = find_extra(key, kind)
                if hit is not None:
                    print(f'    "t{key[0]}_q{key[1]}_{kind}": ({key}, {hit[0]}, {hit[1]}),', flush=True)


if __name__ == "__main__":
    main()
