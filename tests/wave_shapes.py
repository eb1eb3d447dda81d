"""The triangle-filter wave kernels of mlx-data_amd/csrc/wave.hip, one shape each.

``instantiations()`` reads the kernel list out of wave.hip: a scatter key is
``(S, DMAX, taps, Q, P)`` (an ``MXD_SCATTER`` / ``MXD_SCATTER_B`` line; byte
lanes are P = 16), a gather key ``(C, taps, Q)`` (the ``select_q`` /
``select_taps`` cases for 1, 2 and 3 channels).  ``find(key, strips)`` searches,
with the host-only ``capi.describe_plan``, for the smallest whole-frame resize
``(src_w, src_h, out_w, out_h)`` whose plan is exactly that key: once in one
strip (or the fewest strips the key takes inside the search bounds) at about 20
output rows, once in two strips at 64 rows and columns or more.  ``SHAPES`` is the
committed result with the strip count of each frame (``python
tests/wave_shapes.py [key ...]`` prints the entries again when a kernel is
added), ``UNREACHABLE`` the keys no whole frame inside the bounds plans, and
``EXTRA`` named cases of the routes that run a shape on a deeper schedule or a
larger tap bucket than its own.

Everything here is host only.  Output height follows the source's aspect
(``out_h``), as in tests/test_gpu_filters.py, unless only a frame resized less
horizontally than vertically reaches the key; it is never a multiple of 8 and
always above 16, so the rows fall into several bands with a short last one.
"""
import os
import re

from mlx_data_amd import capi

WAVE_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlx-data_amd", "csrc",
                        "wave.hip")

# ---- search bounds (find, and the bounded rerun of tests/test_wave_shapes.py) --
ROWS_ONE = (20, 19, 21, 18, 22, 17, 23)  # output rows tried for the one-strip shape, in this order
ROWS_TWO = (68, 67, 69, 66, 70, 65, 71)  # ... and for the two-strip shape (the +-1 gate applies from 64)
MAX_RATIO = 16                           # source rows per output row: the deepest schedule
MAX_COLS = 768                           # output columns
ASPECTS = (None, 1.5)                    # horizontal ratio: the vertical one (None), then 1.5 : 1


def instantiations(path=WAVE_HIP):
    """The scatter keys (S, DMAX, taps, Q, P) and gather keys (C, taps, Q) wave.hip instantiates."""
    text = open(path).read()
    keys = set()
    for m in re.finditer(r"^\s*MXD_SCATTER\((\d+), *(\d+), *(\d+), *(\d+), *(\d+)\)", text, re.M):
        keys.add(tuple(int(v) for v in m.groups()))
    for m in re.finditer(r"^\s*MXD_SCATTER_B\((\d+), *(\d+), *(\d+), *(\d+)\)", text, re.M):
        keys.add(tuple(int(v) for v in m.groups()) + (16,))
    taps = [int(a) for a, b in re.findall(r"case (\d+): return select_gather<C, OUT, (\d+), Q>", text) if a == b]
    qs = [int(a) for a, b in re.findall(r"case (\d+): return select_taps<C, OUT, (\d+)>", text) if a == b]
    chans = [int(a) for a, b in re.findall(r"case (\d+): return select_q<(\d+), OUT>", text) if a == b]
    assert taps and qs and chans, "wave.hip: the gather selection no longer reads as select_q / select_taps cases"
    keys |= {(c, t, q) for c in chans for t in taps for q in qs}
    return keys


def is_gather(key):
    return len(key) == 3


def channels_of(key):
    return key[0] if is_gather(key) else 3


def policy_of(key):
    """The kernel policy under which the key's lane width is what the planner
    takes; each of them also keeps the band kernel off, so the wave plan is what
    launches."""
    if is_gather(key):
        return capi.MXD_POLICY_NO_SCATTER
    return {4: capi.MXD_POLICY_NARROW, 8: capi.MXD_POLICY_NO_BYTES, 16: capi.MXD_POLICY_BYTES}[key[4]]


def shifts_of(key):
    """Source base offsets (bytes past a 4-byte boundary) the key is run from:
    every one for byte lanes, which have no realigning form, else 0 and 1."""
    return (0, 1, 2, 3) if not is_gather(key) and key[4] == 16 else (0, 1)


SRC_PAD = 16  # bytes a shifted source's rows are longer than its pixels


def out_h(sw, sh, cw):
    return max(1, round(sh * cw / sw))


def whole(cw, ch, flip=0):
    return (cw, ch, 0, 0, cw, ch, flip)


def src_stride(w, c, shift):
    return (w * c + (SRC_PAD if shift else 0) + 15) // 16 * 16


def dst_pad(f32):
    """Bytes a destination row is longer than its pixels (the guard bytes): odd
    for u8, a whole element for f32."""
    return 8 if f32 else 5


def entry(shape, g, shift=0, f32=False):
    """The mxd_image fields of geometry g on an (h, w, c) source, laid out as
    tests/test_gpu_wave_shapes.py lays it out (a shifted source's rows SRC_PAD
    bytes longer, destination rows dst_pad bytes longer than the pixels)."""
    h, w, c = shape
    rw, rh, cx, cy, cw, ch, flip = g
    return dict(src=256 + shift, src_stride=src_stride(w, c, shift), src_w=w, src_h=h, channels=c, resize_w=rw,
                resize_h=rh, crop_x=cx, crop_y=cy, crop_w=cw, crop_h=ch, flip=int(flip), dst=256,
                dst_stride=cw * c * (4 if f32 else 1) + dst_pad(f32))


def plan(shape, g, policy, shift=0, f32=False):
    prev = capi.set_kernel_policy(policy)
    try:
        return capi.describe_plan(entry(shape, g, shift, f32), capi.MXD_F32_DIV255 if f32 else capi.MXD_U8)
    finally:
        capi.set_kernel_policy(prev)


def key_of(p, channels):
    """The instantiation a describe_plan result names (None: no wave kernel)."""
    if not p["wave"]:
        return None
    if p["kind"] == 0:
        return (channels, p["taps"], p["q"])
    return (p["s"], p["dmax"], p["taps"], p["q"], p["p"])


def windows(cw, ch):
    """The four entries every shape is run as: the whole frame, the whole frame
    mirrored, an inner window at odd offsets mirrored, and a window touching the
    far right and bottom edges."""
    return [whole(cw, ch), whole(cw, ch, 1), (cw, ch, 3, 2, cw - 5, ch - 3, 1),
            (cw, ch, cw // 3, ch // 4, cw - cw // 3, ch - ch // 4, 0)]


def planned(key, shape, g, shifts):
    """(every plan of g is `key`, the strip count) over u8 / f32 and the shifts."""
    ns = set()
    for shift in shifts:
        for f32 in (False, True):
            p = plan(shape, g, policy_of(key), shift, f32)
            if key_of(p, shape[2]) != key:
                return False, None
            ns.add(p["nstrips"])
    return len(ns) == 1, ns.pop()


_DEPTHS = (1, 2, 3, 4, 5, 6, 9, 12, 16)
_BUCKETS = (2, 3, 4, 6, 8, 10, 12, 17, 24, 32)


def _rows(key, ch, max_ratio):
    """Source heights worth planning for `ch` output rows: those whose vertical
    table has the key's schedule depth (above the next shallower depth
    instantiated, so the search starts at the shapes of the deeper-schedule
    route), or for gather keys a width in the key's tap bucket."""
    out = []
    for sh in range(max(2, ch // 3), ch * max_ratio + 1):
        first, cnt, w = capi.axis_taps(sh, ch)
        if is_gather(key):
            lo = max([b for b in _BUCKETS if b < key[1]], default=0)
            if not lo - 1 <= w.shape[1] <= key[1]:
                continue
        else:
            last = first + cnt - 1
            d = int((last[1:] - last[:-1]).max())
            lo = max([x for x in _DEPTHS if x < key[1]], default=0)
            if not lo < d <= key[1]:
                continue
        out.append(sh)
    return out


def find(key, strips, rows=None, max_ratio=MAX_RATIO, max_cols=MAX_COLS, aspects=ASPECTS):
    """The first whole-frame (src_w, src_h, out_w, out_h), by output rows in
    the order of ROWS_ONE / ROWS_TWO, then source height, then output width,
    whose plan is `key` in u8 and f32 -- for strips == 2 from every base offset
    of shifts_of(key), at 64 columns or more.  A frame in exactly `strips`
    strips ends the search; without one, the frame of the first row count that
    has any: in the fewest strips above `strips`, else (two asked for, and the
    planner only ever gives the key one) in one.  Frames keep the source's
    aspect (aspects[0] is None: out_h follows); only when no such frame plans
    the key, the horizontal ratios aspects[1:] are tried against the vertical
    one.  None when nothing inside the bounds plans the key."""
    for hr in aspects:
        hit = _find(key, strips, rows, max_ratio, max_cols, hr)
        if hit is not None:
            return hit
    return None


def _find(key, strips, rows, max_ratio, max_cols, hr):
    c = channels_of(key)
    q = key[2] if is_gather(key) else key[3]
    best = None
    for ch in rows or (ROWS_TWO if strips == 2 else ROWS_ONE):
        for sh in _rows(key, ch, max_ratio):
            for cw in range(64 if strips == 2 else 8, min(max_cols, 64 * q * max(strips, 2)) + 1):
                sw = round(sh * cw / ch) if hr is None else round(cw * hr)
                if sw < 1 or (hr is None and out_h(sw, sh, cw) != ch):
                    continue
                ok, ns = planned(key, (sh, sw, c), whole(cw, ch), shifts_of(key) if strips == 2 else (0,))
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


# key -> two whole frames (src w, src h, out w, out h, strips): about 20 rows in one strip (or the fewest),
# and 64 rows and columns or more in two strips (or the fewest above; one where the planner gives no more)
SHAPES = {
    (1, 2, 1): ((3, 6, 10, 20, 1), (29, 31, 64, 68, 1)),
    (1, 2, 2): ((20, 6, 65, 20, 1), (21, 22, 65, 68, 1)),
    (1, 2, 4): ((39, 6, 129, 20, 1), (83, 22, 257, 68, 2)),
    (1, 3, 1): ((32, 21, 30, 20, 1), (66, 70, 64, 68, 1)),
    (1, 3, 2): ((68, 21, 65, 20, 1), (104, 69, 102, 68, 1)),
    (1, 3, 4): ((135, 21, 129, 20, 1), (261, 69, 257, 68, 2)),
    (1, 4, 1): ((20, 30, 13, 20, 1), (97, 103, 64, 68, 1)),
    (1, 4, 2): ((98, 30, 65, 20, 1), (98, 102, 65, 68, 1)),
    (1, 4, 4): ((194, 30, 129, 20, 1), (386, 102, 257, 68, 2)),
    (1, 6, 1): ((16, 41, 8, 20, 1), (129, 137, 64, 68, 1)),
    (1, 6, 2): ((133, 41, 65, 20, 1), (131, 137, 65, 68, 1)),
    (1, 6, 4): ((264, 41, 129, 20, 1), (518, 137, 257, 68, 2)),
    (1, 8, 1): ((92, 61, 30, 20, 1), (194, 206, 64, 68, 1)),
    (1, 8, 2): ((198, 61, 65, 20, 1), (308, 205, 102, 68, 1)),
    (1, 8, 4): ((393, 61, 129, 20, 1), (775, 205, 257, 68, 2)),
    (1, 10, 1): ((32, 81, 8, 20, 1), (257, 273, 64, 68, 1)),
    (1, 10, 2): ((263, 81, 65, 20, 1), (1028, 273, 256, 68, 2)),
    (1, 10, 4): ((522, 81, 129, 20, 1), (1032, 273, 257, 68, 2)),
    (1, 12, 1): ((152, 101, 30, 20, 1), (322, 342, 64, 68, 1)),
    (1, 12, 2): ((328, 101, 65, 20, 1), (1028, 341, 205, 68, 2)),
    (1, 12, 4): ((651, 101, 129, 20, 1), (1289, 341, 257, 68, 2)),
    (1, 17, 1): ((48, 121, 8, 20, 1), (1026, 545, 128, 68, 2)),
    (1, 17, 2): ((393, 121, 65, 20, 1), (1029, 409, 171, 68, 2)),
    (1, 17, 4): ((780, 121, 129, 20, 1), (1546, 409, 257, 68, 2)),
    (2, 2, 1): ((3, 6, 10, 20, 1), (29, 31, 64, 68, 1)),
    (2, 2, 2): ((20, 6, 65, 20, 1), (21, 22, 65, 68, 1)),
    (2, 2, 4): ((39, 6, 129, 20, 1), (83, 22, 257, 68, 2)),
    (2, 3, 1): ((32, 21, 30, 20, 1), (66, 70, 64, 68, 1)),
    (2, 3, 2): ((68, 21, 65, 20, 1), (104, 69, 102, 68, 1)),
    (2, 3, 4): ((135, 21, 129, 20, 1), (261, 69, 257, 68, 2)),
    (2, 4, 1): ((20, 30, 13, 20, 1), (97, 103, 64, 68, 1)),
    (2, 4, 2): ((98, 30, 65, 20, 1), (98, 102, 65, 68, 1)),
    (2, 4, 4): ((194, 30, 129, 20, 1), (386, 102, 257, 68, 2)),
    (2, 6, 1): ((16, 41, 8, 20, 1), (129, 137, 64, 68, 1)),
    (2, 6, 2): ((133, 41, 65, 20, 1), (514, 137, 255, 68, 2)),
    (2, 6, 4): ((264, 41, 129, 20, 1), (518, 137, 257, 68, 2)),
    (2, 8, 1): ((92, 61, 30, 20, 1), (194, 206, 64, 68, 1)),
    (2, 8, 2): ((198, 61, 65, 20, 1), (516, 205, 171, 68, 2)),
    (2, 8, 4): ((393, 61, 129, 20, 1), (775, 205, 257, 68, 2)),
    (2, 10, 1): ((32, 81, 8, 20, 1), (514, 273, 128, 68, 2)),
    (2, 10, 2): ((263, 81, 65, 20, 1), (518, 273, 129, 68, 2)),
    (2, 10, 4): ((194, 81, 129, 20, 1), (386, 273, 257, 68, 2)),
    (2, 12, 1): ((152, 101, 30, 20, 1), (517, 341, 103, 68, 2)),
    (2, 12, 2): ((328, 101, 65, 20, 1), (647, 341, 129, 68, 2)),
    (2, 12, 4): ((194, 102, 129, 20, 1), (386, 342, 257, 68, 2)),
    (2, 17, 1): ((48, 121, 8, 20, 1), (517, 409, 86, 68, 2)),
    (2, 17, 2): ((393, 121, 65, 20, 1), (776, 409, 129, 68, 2)),
    (2, 17, 4): ((194, 121, 129, 20, 1), (386, 409, 257, 68, 2)),
    (3, 2, 1): ((3, 6, 10, 20, 1), (29, 31, 64, 68, 1)),
    (3, 2, 2): ((20, 6, 65, 20, 1), (21, 22, 65, 68, 1)),
    (3, 2, 4): ((39, 6, 129, 20, 1), (83, 22, 257, 68, 2)),
    (3, 3, 1): ((32, 21, 30, 20, 1), (66, 70, 64, 68, 1)),
    (3, 3, 2): ((68, 21, 65, 20, 1), (257, 69, 253, 68, 2)),
    (3, 3, 4): ((135, 21, 129, 20, 1), (261, 69, 257, 68, 2)),
    (3, 4, 1): ((20, 30, 13, 20, 1), (97, 103, 64, 68, 1)),
    (3, 4, 2): ((98, 30, 65, 20, 1), (260, 102, 173, 68, 2)),
    (3, 4, 4): ((194, 30, 129, 20, 1), (386, 102, 257, 68, 2)),
    (3, 6, 1): ((16, 41, 8, 20, 1), (258, 137, 128, 68, 2)),
    (3, 6, 2): ((133, 41, 65, 20, 1), (260, 137, 129, 68, 2)),
    (3, 6, 4): ((194, 41, 129, 20, 1), (386, 137, 257, 68, 2)),
    (3, 8, 1): ((92, 61, 30, 20, 1), (308, 205, 102, 68, 2)),
    (3, 8, 2): ((198, 61, 65, 20, 1), (389, 205, 129, 68, 2)),
    (3, 8, 4): ((194, 62, 129, 20, 1), (386, 206, 257, 68, 2)),
    (3, 10, 1): ((32, 81, 8, 20, 1), (257, 273, 64, 68, 2)),
    (3, 10, 2): ((98, 81, 65, 20, 1), (258, 273, 172, 68, 2)),
    (3, 10, 4): ((194, 81, 129, 20, 1), (386, 273, 257, 68, 2)),
    (3, 12, 1): ((152, 101, 30, 20, 1), (322, 342, 64, 68, 2)),
    (3, 12, 2): ((98, 102, 65, 20, 1), (258, 342, 172, 68, 2)),
    (3, 12, 4): ((194, 102, 129, 20, 1), (386, 342, 257, 68, 2)),
    (3, 17, 1): ((48, 121, 8, 20, 1), (385, 409, 64, 68, 2)),
    (3, 17, 2): ((98, 121, 65, 20, 1), (258, 409, 172, 68, 2)),
    (3, 17, 4): ((194, 121, 129, 20, 1), (386, 409, 257, 68, 2)),
    (2, 2, 3, 2, 4): ((72, 22, 65, 20, 1), (257, 70, 250, 68, 2)),
    (2, 2, 3, 2, 16): ((72, 22, 65, 20, 1), (343, 91, 256, 68, 2)),
    (2, 2, 3, 4, 8): ((509, 22, 463, 20, 2), (509, 70, 494, 68, 2)),
    (2, 2, 3, 4, 16): ((142, 22, 129, 20, 1), (265, 70, 257, 68, 2)),
    (2, 2, 4, 2, 4): ((98, 30, 65, 20, 1), (260, 102, 173, 68, 2)),
    (2, 2, 4, 2, 16): ((98, 30, 65, 20, 1), (344, 102, 229, 68, 2)),
    (2, 2, 4, 4, 8): ((510, 40, 255, 20, 1), (512, 102, 341, 68, 2)),
    (2, 2, 4, 4, 16): ((194, 30, 129, 20, 1), (386, 102, 257, 68, 2)),
    (2, 3, 6, 2, 4): ((133, 41, 65, 20, 1), (260, 137, 129, 68, 2)),
    (2, 3, 6, 2, 8): ((515, 41, 251, 20, 2), (514, 137, 255, 68, 2)),
    (2, 3, 6, 2, 16): ((133, 41, 65, 20, 1), (342, 137, 170, 68, 2)),
    (2, 4, 8, 1, 4): ((25, 62, 8, 20, 1), (258, 206, 85, 68, 2)),
    (2, 4, 8, 1, 16): ((25, 62, 8, 20, 1), (342, 206, 113, 68, 2)),
    (2, 4, 8, 2, 8): ((506, 79, 128, 20, 1), (515, 206, 170, 68, 2)),
    (2, 4, 8, 2, 16): ((202, 62, 65, 20, 1), (391, 206, 129, 68, 2)),
    (2, 5, 10, 1, 4): ((32, 81, 8, 20, 1), (257, 273, 64, 68, 2)),
    (2, 5, 10, 1, 16): ((32, 81, 8, 20, 1), (345, 273, 86, 68, 2)),
    (2, 5, 10, 2, 8): ((506, 81, 125, 20, 1), (518, 273, 129, 68, 2)),
    (2, 5, 10, 2, 16): ((263, 81, 65, 20, 1), (518, 273, 129, 68, 2)),
    (2, 6, 12, 1, 4): ((41, 102, 8, 20, 1), (322, 342, 64, 68, 2)),
    (2, 6, 12, 1, 16): ((41, 102, 8, 20, 1), (342, 342, 68, 68, 2)),
    (2, 6, 12, 2, 8): ((505, 102, 99, 20, 1), (649, 342, 129, 68, 2)),
    (2, 6, 12, 2, 16): ((332, 102, 65, 20, 1), (649, 342, 129, 68, 2)),
    (2, 9, 17, 1, 4): ((48, 121, 8, 20, 1), (385, 409, 64, 68, 2)),
    (2, 9, 17, 1, 8): ((502, 157, 64, 20, 1), (517, 409, 86, 68, 2)),
    (2, 9, 17, 1, 16): ((48, 121, 8, 20, 1), (385, 409, 64, 68, 2)),
    (2, 12, 24, 1, 4): ((73, 182, 8, 20, 1), (578, 614, 64, 68, 3)),
    (2, 12, 24, 1, 8): ((500, 182, 55, 20, 1), (578, 614, 64, 68, 2)),
    (2, 16, 32, 1, 4): ((96, 241, 8, 20, 1), (769, 817, 64, 68, 4)),
    (2, 16, 32, 1, 8): ((494, 241, 41, 20, 1), (769, 817, 64, 68, 2)),
    (3, 1, 2, 4, 4): ((77, 12, 129, 20, 1), (166, 44, 257, 68, 2)),
    (3, 1, 2, 4, 16): ((77, 12, 129, 20, 1), (166, 44, 257, 68, 2)),
}

# key -> why no whole frame inside the bounds above plans it.  (None today: the gather kernels with
# Q = 2 / 4 at 6 taps and more, whose strips of more than 64 (128) columns do not fit the window at
# the ratio those taps need, are reached by the 1.5 : 1 horizontal ratio of ASPECTS.)
UNREACHABLE = {
}

# name -> (key it must land on, (src w, src h), (out w, out h)): whole frames of an image_resize(w, h)
# that run on a kernel with a deeper schedule than their vertical ratio needs (bubble iterations
# fill it) or a larger tap bucket than their horizontal taps (zero weights fill it)
EXTRA = {
    "deeper_7_to_1": ((2, 9, 17, 1, 4), (504, 476), (72, 68)),
    "deeper_8_to_1": ((2, 9, 17, 1, 8), (576, 544), (72, 68)),
    "deeper_10_5_to_1": ((2, 12, 24, 1, 8), (756, 714), (72, 68)),
    "deeper_14_to_1": ((2, 16, 32, 1, 4), (1008, 952), (72, 68)),
    "larger_bucket_h1_5_v3_75": ((2, 4, 8, 2, 16), (144, 255), (96, 68)),  # 4 horizontal taps in the 8-tap kernel
    "deeper_h3_75_v1_9": ((2, 4, 8, 1, 4), (360, 133), (96, 70)),          # depth 2 rows on the depth-4 schedule
}

# (key, 0 / 1 for the key's first / second shape or an EXTRA name) -> seed, where the default seed's
# image does not pass the +-1 / 2e-3 gate between the two references (tests/test_wave_shapes.py)
SEEDS = {
}


def seed_of(key, which):
    """The gpu_util.synth seed of a key's first (0) / second (1) shape or of an EXTRA case."""
    if (key, which) in SEEDS:
        return SEEDS[key, which]
    return sum(key) + (7 * which if isinstance(which, int) else 3 * len(which))


def main():
    """Prints the SHAPES entries of the keys given as arguments (all of wave.hip's without any)."""
    import sys
    import time

    def strips(key, k, shape):
        if shape is None:
            return None
        sw, sh, cw, ch = shape
        return shape + (planned(key, (sh, sw, channels_of(key)), whole(cw, ch), shifts_of(key) if k else (0,))[1],)

    only = [eval(a) for a in sys.argv[1:]]
    for key in sorted(only or instantiations(), key=lambda k: (len(k), k)):
        t = time.time()
        one, two = strips(key, 0, find(key, 1)), strips(key, 1, find(key, 2))
        print(f"    {key}: ({one}, {two}),  # {time.time() - t:.0f} s", flush=True)


if __name__ == "__main__":
    main()
