"""GPU: every band kernel of mlx-data_amd/csrc/band.hip at its smallest shape
(tests/band_shapes.py), route asserted and bit exact.

One parametrized case per reachable (taps, nq) key.  The key's two whole-frame
shapes -- one strip at about 20 rows, two strips at 68 rows and 64 columns or
more -- are each submitted as the four windows of wave_shapes.windows (whole,
mirrored, an inner window at odd offsets mirrored, the far right and bottom
edges) and as the tiny windows of band_shapes.tiny_windows (1 x 1, 3 x 2
mirrored, one row, one column: bands shorter than la + 2 groups), under
MXD_POLICY_PREFER_BAND with MXD_TUNE_BAND_ROWS = 8, so that the test knows the
unit count of every image (strips x ceil(rows / 8); 20 rows are bands of 8, 8
and 4).  mxd_describe_band_plan must name the key (taps, db, s and nq) for
every whole frame before anything runs.  Launches per key, each in u8 and f32:

* every frame's windows, and its tiny windows;
* ragged: all of them in one launch -- the unit counts differ (asserted), so
  the kernel finds a unit's image in the unit_img table;
* uniform: three copies of the whole two-strip frame -- equal counts, the
  per_img division;
* the ragged launch again with MXD_TUNE_BAND_GRID = 2 and 3 (a workgroup
  streams several units across image boundaries), MXD_TUNE_BAND_LA = 1 and 8,
  and MXD_TUNE_BAND_ROWS = 3 (bands starting at arbitrary rows);
* the two-strip frame's windows from source base offsets 1, 2 and 3;
* the first frame's windows as ImageNet-normalised bfloat16 CHW
  (mxd_resize_crop_batch_fmt: band kernel into u8 scratch rows, then the
  format pass).

Expected: u8 bit-equal to the kernel-order restatement O.resize_crop_vfirst,
f32 exactly LUT[u8], bfloat16 the table of the oracle's bytes, frames of
64 x 64 and more within +-1 / 2e-3 of the stbir-order oracle.  Nothing expected
comes from the library's kernels.

Destinations are test_gpu_wave_shapes.Dsts (padded rows, a head and a tail,
0xA5 before the launch and outside the image afterwards).  Sources have rows at
the smallest pitch the kernel takes (w * 3 rounded up to 4), and every byte of
the allocation that is not a pixel -- row tails, a head, a tail longer than
the widest class's padded taps -- is 0xFF: the horizontal pass reads `taps`
columns past a strip's last tap with zero weights, and a weight there would
change bytes."""
import numpy as np
import pytest

import band_shapes as B
import filter_ref
import oracle as O
import test_gpu_wave_shapes as T
import wave_shapes as W
from gpu_util import synth
from mlx_data_amd import capi

pytestmark = pytest.mark.gpu

FILL = 0xFF
SRC_HEAD = 64                                   # 0xFF bytes before an image's first pixel (+ the base offset)
SRC_TAIL = max(B.classes()) * 3 + 16            # ... and after its last row, at least
ROWS = 8                                        # the forced band height of every launch but one

# every (key, output mode) whose whole frames the cases of this process launched
LAUNCHED = set()


def launch(imgs, geoms, mode, shift=0, filters=None):
    """One mxd_resize_crop_batch (/ _fmt) call; every distinct image is stored
    once, `shift` bytes past a 4-byte boundary.  Returns the guarded destinations."""
    pitch, off, total = {}, {}, 0
    for img in imgs:
        if id(img) not in off:
            h, w, _ = img.shape
            pitch[id(img)] = B.src_stride(w)
            off[id(img)] = total + SRC_HEAD + shift
            total += (SRC_HEAD + 4 + pitch[id(img)] * h + SRC_TAIL + 255) // 256 * 256
    host = np.full(total, FILL, np.uint8)
    for img in imgs:
        h, w, c = img.shape
        p, o = pitch[id(img)], off[id(img)]
        host[o:o + p * h].reshape(h, p)[:, :w * c] = img.reshape(h, w * c)
    src = capi.DeviceBuffer(total)
    src.upload(host)
    d = T.Dsts(geoms, [3] * len(imgs), mode)
    try:
        entries = []
        for k, (img, g) in enumerate(zip(imgs, geoms)):
            e = B.entry(img.shape, g, shift, mode == "f32", filters[k] if filters else 0)
            entries.append(dict(e, src=src.ptr + off[id(img)], dst=d.ptr(k), dst_stride=d.pitch[k]))
        arr, n = capi.make_images(entries)
        if d.elem is None:
            capi.resize_crop_batch(arr, n, capi.MXD_F32_DIV255 if mode == "f32" else capi.MXD_U8, 0, None)
        else:
            capi.resize_crop_batch_fmt(arr, n, d.fmt(3), 0, None)
        capi.check(capi.lib().mxd_device_synchronize(0))
    except BaseException:
        d.free()
        raise
    finally:
        src.free()
    return d


def with_knobs(f, rows=ROWS, la=0, grid=0):
    prev_p = capi.set_kernel_policy(capi.MXD_POLICY_PREFER_BAND)
    prev = [(k, capi.set_tuning(k, v)) for k, v in ((capi.MXD_TUNE_BAND_ROWS, rows), (capi.MXD_TUNE_BAND_LA, la),
                                                    (capi.MXD_TUNE_BAND_GRID, grid))]
    try:
        return f()
    finally:
        for k, v in prev:
            capi.set_tuning(k, v)
        capi.set_kernel_policy(prev_p)


class Case:
    """The frames of one key with the expected bytes of every window asked for."""

    def __init__(self, key, frames, tag, filter=0):
        self.key, self.frames, self.tag, self.filter = key, frames, tag, filter
        self.wants = {}

    def want(self, img, g):
        if (id(img), g) not in self.wants:
            w = filter_ref.vfirst(img, g, self.filter) if self.filter else O.resize_crop_vfirst(img, g)
            if not self.filter:
                T.gate(w, img, g)  # (the bytes the device must give, so this is its gate too)
            self.wants[id(img), g] = w
        return self.wants[id(img), g]

    def run(self, imgs, geoms, mode, what, shift=0, **knobs):
        filters = [self.filter] * len(imgs) if self.filter else None
        d = with_knobs(lambda: launch(imgs, geoms, mode, shift, filters), **knobs)
        try:
            d.check([self.want(i, g) for i, g in zip(imgs, geoms)], (self.tag, self.key, what, "shift", shift, knobs))
        finally:
            d.free()

    def units(self, imgs, geoms, f32, rows=ROWS):
        """strips x bands of every image the planner gives the key."""
        out = []
        for img, g in zip(imgs, geoms):
            p = B.plan(img.shape, g, 0, f32)
            if B.key_of(p) == self.key:
                out.append(p["nstrips"] * -(-g[5] // rows))
        return out


def assert_route(key, img, cw, ch, shifts, tag):
    assert ch % 8 != 0 and ch > 16
    ok, ns = B.planned(key, img.shape, W.whole(cw, ch), shifts)
    assert ok, (tag, key, img.shape, (cw, ch), [B.plan(img.shape, W.whole(cw, ch), s) for s in shifts])
    return ns


def run_key(key):
    frames = []
    for k, (sw, sh, cw, ch, ns) in enumerate(B.SHAPES[key]):
        img = synth(sh, sw, 3, B.seed_of(key, k))
        assert assert_route(key, img, cw, ch, B.SHIFTS if k else (0,), "shape") == ns
        frames.append((img, cw, ch))
    case = Case(key, frames, "band")
    per_frame = [[(img, g) for g in W.windows(cw, ch)] for img, cw, ch in frames]
    tiny = [[(img, g) for g in B.tiny_windows(cw, ch)] for img, cw, ch in frames]
    ragged = [x for a, b in zip(per_frame, tiny) for x in a + b]
    img2, cw2, ch2 = frames[1]
    uniform = [(img2, W.whole(cw2, ch2))] * 3
    for mode in ("u8", "f32"):
        f32 = mode == "f32"
        counts = case.units(*zip(*ragged), f32)
        assert len(set(counts)) > 1 and sum(counts) > 6, (key, counts)
        same = case.units(*zip(*uniform), f32)
        assert len(same) == 3 and len(set(same)) == 1 and same[0] == B.SHAPES[key][1][4] * -(-ch2 // ROWS), (key, same)
        for k in range(len(frames)):
            case.run(*zip(*per_frame[k]), mode, "windows %d" % k)
            case.run(*zip(*tiny[k]), mode, "tiny windows %d" % k)
        case.run(*zip(*ragged), mode, "ragged")
        case.run(*zip(*uniform), mode, "uniform")
        for grid in (2, 3):
            case.run(*zip(*ragged), mode, "persistent grid", grid=grid)
        for la in (1, 8):
            case.run(*zip(*ragged), mode, "lookahead", la=la)
        case.run(*zip(*ragged), mode, "band height", rows=3)
        for shift in (1, 2, 3):
            case.run(*zip(*per_frame[1]), mode, "base offset", shift=shift)
        LAUNCHED.add((key, mode))
    case.run(*zip(*per_frame[0]), "bf16_chw", "formatted")


@pytest.mark.parametrize("key", sorted(B.SHAPES), ids=lambda k: "t%d_q%d" % k)
def test_every_band_kernel(key):
    run_key(key)


@pytest.mark.parametrize("name", sorted(B.EXTRA))
def test_vertical_ratios_other_than_the_horizontal(name):
    """An output row whose new source rows fill several groups (deep), and
    groups that hold fewer rows than the class's db (flat; the taps-2 class: a
    vertical upscale, output rows that bring no new row)."""
    key, (sw, sh), (cw, ch) = B.EXTRA[name]
    img = synth(sh, sw, 3, B.seed_of(key, name))
    assert_route(key, img, cw, ch, B.SHIFTS, name)
    case = Case(key, [(img, cw, ch)], name)
    imgs, geoms = zip(*[(img, g) for g in W.windows(cw, ch) + B.tiny_windows(cw, ch)])
    for mode in ("u8", "f32"):
        for shift in (0, 3):
            case.run(imgs, geoms, mode, "ragged", shift=shift)
        case.run(imgs, geoms, mode, "persistent grid", grid=2)
        case.run(imgs, geoms, mode, "band height", rows=3)


@pytest.mark.parametrize("filter", ["catmullrom", "mitchell"])
def test_cubic_downscale_under_prefer_band(filter):
    """The route the band kernel declines (a cubic source row reaches four
    output rows, a schedule entry holds three weights): bit-equal to the
    kernel-order restatement of the filter.  The tiny windows are no higher
    than a class's accumulator slots, so the planner does give some of them to
    the band kernel, negative weights and all: the same bytes are expected."""
    img = synth(255, 270, 3, 31)
    cw, ch = 72, 68
    for g in W.windows(cw, ch):
        assert B.plan(img.shape, g, filter=filter)["band"] == 0, (filter, g)
    assert any(B.plan(img.shape, g, filter=filter)["band"] for g in B.tiny_windows(cw, ch))
    case = Case(None, [(img, cw, ch)], filter, filter)
    imgs, geoms = zip(*[(img, g) for g in W.windows(cw, ch) + B.tiny_windows(cw, ch)])
    for mode in ("u8", "f32"):
        case.run(imgs, geoms, mode, "cubic")
        case.run(imgs, geoms, mode, "cubic", shift=1)


def test_every_reachable_key_was_launched():
    missing = {(k, m) for k in B.SHAPES for m in ("u8", "f32")} - LAUNCHED
    assert not missing, sorted(missing)
