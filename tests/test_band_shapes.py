"""CPU: the shape table of the band kernels (tests/band_shapes.py).

* the table covers band.hip: every class of ``kBandClasses[]`` times every
  ``NQ`` of ``pick_nq`` has a shape or the condition of ``band_plan_image``
  that keeps every frame off it, so a class added without a shape fails here;
* every recorded shape (and every named anisotropic case) still plans its key
  under MXD_POLICY_PREFER_BAND -- taps, db, s and nq -- in u8 and f32, from
  source base offsets 0..3, in the recorded strip count;
* a bounded rerun of the finder reproduces the committed shapes of a few keys;
* a coarse sweep (horizontal ratios 0.7..16, widths up to the bound, both
  flips, base offsets 0..3, u8 and f32) plans no unreachable key;
* a cubic table never plans the band kernel for a crop of more rows than a
  class has accumulator slots (a cubic source row reaches four output rows, a
  schedule entry holds three weights);
* on every frame of 64 x 64 and more the reference alone passes the project's
  gate: the kernel-order restatement O.resize_crop_vfirst against the
  stbir-order oracle within +-1 and 2e-3 differing channels, on the seeds the
  GPU test uses."""
import pytest

import band_shapes as B
import oracle as O
import wave_shapes as W
from gpu_util import compare, oracle_out, synth

MAX_FRAC = 2e-3


def test_the_table_covers_every_instantiation():
    keys = B.instantiations()
    assert len(keys) >= 36 and len(B.classes()) >= 9 and len(B.window_sizes()) >= 4
    assert not set(B.SHAPES) & set(B.UNREACHABLE)
    assert set(B.SHAPES) | set(B.UNREACHABLE) == keys, (
        "without a shape", sorted(keys - set(B.SHAPES) - set(B.UNREACHABLE)),
        "not in band.hip", sorted((set(B.SHAPES) | set(B.UNREACHABLE)) - keys))
    assert all(isinstance(r, str) and r and "\n" not in r for r in B.UNREACHABLE.values())


def test_a_new_class_or_window_size_is_noticed(tmp_path):
    text = open(B.BAND_H).read()
    anchor = "{32, 8, 2}};"
    assert anchor in text
    h = tmp_path / "band.h"
    h.write_text(text.replace(anchor, "{32, 8, 2}, {48, 8, 2}};"))
    assert B.instantiations(band_h=str(h)) - B.instantiations() == {(48, q) for q in B.window_sizes()}
    text = open(B.BAND_HIP).read()
    anchor = "    case 4: return pick_class<C, F32, 4>(ci, seq);\n"
    assert anchor in text
    hip = tmp_path / "band.hip"
    hip.write_text(text.replace(anchor, anchor + "    case 5: return pick_class<C, F32, 5>(ci, seq);\n"))
    assert B.instantiations(band_hip=str(hip)) - B.instantiations() == {(t, 5) for t in B.classes()}


@pytest.mark.parametrize("key", sorted(B.SHAPES), ids=str)
def test_every_shape_plans_its_key(key):
    db, s = B.classes()[key[0]]
    for k, (sw, sh, cw, ch, ns) in enumerate(B.SHAPES[key]):
        assert ch % 8 != 0 and ch > 16 and (k == 0 or ch >= 64)
        if k == 1 and cw < 64:  # only where the same resize at 64 columns is past the key's window
            assert B.key_of(B.plan((sh, round(sw * 64 / cw), 3), W.whole(64, ch))) not in (key, None), (key, cw)
        for shift in B.SHIFTS:
            for f32 in (False, True):
                p = B.plan((sh, sw, 3), W.whole(cw, ch), shift, f32)
                assert p["band"] == 1 and (p["taps"], p["db"], p["s"], p["nq"], p["nstrips"]) == (key[0], db, s, key[1], ns), (
                    key, (sw, sh, cw, ch), shift, f32, p)


@pytest.mark.parametrize("name", sorted(B.EXTRA))
def test_every_extra_case_plans_its_key(name):
    """... and is what its name says: `deep`, an output row with more new
    source rows than a group holds; `flat`, never a full group (db = 1: output
    rows without a new source row)."""
    key, (sw, sh), (cw, ch) = B.EXTRA[name]
    db, _ = B.classes()[key[0]]
    assert key in B.SHAPES and ch % 8 != 0 and ch >= 64 and (sw, cw) == B.SHAPES[key][1][::2][:2]
    assert name.startswith("t%d_q%d_" % key)
    ok, _ = B.planned(key, (sh, sw, 3), W.whole(cw, ch), B.SHIFTS)
    assert ok, (name, B.plan((sh, sw, 3), W.whole(cw, ch)))
    lo, hi = B.new_rows(sh, ch)
    if name.endswith("deep"):
        assert hi > db, (name, hi)
    else:
        assert name.endswith("flat") and (hi < db or (db == 1 and lo == 0 and sh < ch)), (name, lo, hi)


def test_every_key_has_its_extra_cases():
    """Both kinds for every reachable key, but where the planner allows none."""
    for key in B.SHAPES:
        for kind in ("deep", "flat"):
            name = "t%d_q%d_%s" % (key + (kind,))
            assert name in B.EXTRA or (name in B.NO_EXTRA and B.NO_EXTRA[name]), name


# keys whose whole search (both shapes, every row count it needs) takes a second or two
RERUN = ((2, 1), (4, 1), (4, 2), (6, 1))


@pytest.mark.parametrize("key", RERUN, ids=str)
def test_the_finder_reproduces_the_table(key):
    for k, strips in enumerate((1, 2)):
        assert B.find(key, strips) == B.SHAPES[key][k][:4], (key, strips)


SWEEP_RATIOS = (0.7, 0.85, 1.0, 1.2, 1.5, 1.9, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 7.0, 8.5, 10.0, 12.0, 14.0, 16.0)
SWEEP_COLS = (8, 33, 64, 100, 129, 171, 200, 255, 256, 257, 320, 384, 400, 511, 512, 513, 640, 700, 767, 768)


def test_unreachable_keys_stay_unreachable():
    assert SWEEP_COLS[-1] == B.MAX_COLS and SWEEP_RATIOS[-1] == B.MAX_RATIO
    seen = set()
    for r in SWEEP_RATIOS:
        for cw in SWEEP_COLS:
            sw, ch = max(1, round(cw * r)), 20
            sh = max(2, round(ch * min(r, 4.0)))  # (the class and the window follow the horizontal taps alone)
            for flip in (0, 1):
                for shift in B.SHIFTS:
                    for f32 in (False, True):
                        seen.add(B.key_of(B.plan((sh, sw, 3), W.whole(cw, ch, flip), shift, f32)))
    assert not seen & set(B.UNREACHABLE), sorted(seen & set(B.UNREACHABLE))
    assert seen - {None} <= set(B.SHAPES)
    assert len(seen & set(B.SHAPES)) >= len(B.SHAPES) - 2, sorted(set(B.SHAPES) - seen)  # (the sweep does reach the kernels)


@pytest.mark.parametrize("filter", ["catmullrom", "mitchell", "cubicbspline"])
def test_a_cubic_table_never_plans_the_band_kernel(filter):
    for (sw, sh), (cw, ch) in (((270, 255), (72, 68)), ((300, 200), (200, 133)), ((640, 480), (96, 72)),
                               ((1280, 960), (100, 75)), ((1400, 300), (90, 68)), ((60, 50), (90, 75))):
        assert B.plan((sh, sw, 3), W.whole(cw, ch))["band"] == 1, "the triangle table of the same frame plans it"
        for g in W.windows(cw, ch) + B.tiny_windows(cw, ch):
            for shift in (0, 1):
                for f32 in (False, True):
                    p = B.plan((sh, sw, 3), g, shift, f32, filter)
                    # (a crop no higher than a class's s has no source row reaching more of its rows than
                    # s: the planner may take it, and tests/test_gpu_band_shapes.py checks its bytes)
                    assert p["band"] == 0 or g[5] <= p["s"], (filter, (sw, sh), g, shift, f32, p)


def _frames():
    for key in sorted(B.SHAPES):
        for k, shape in enumerate(B.SHAPES[key]):
            yield key, k, shape[:2], shape[2:4]
    for name, (key, src, out) in sorted(B.EXTRA.items()):
        yield key, name, src, out


def test_the_reference_alone_passes_the_gate():
    checked = 0
    for key, k, (sw, sh), (cw, ch) in _frames():
        if cw < 64 or ch < 64:
            continue
        img = synth(sh, sw, 3, B.seed_of(key, k))
        for g in W.windows(cw, ch):
            if g[4] >= 64 and g[5] >= 64:
                m, frac = compare(O.resize_crop_vfirst(img, g), oracle_out(img, g))
                assert m <= 1 and frac < MAX_FRAC, (key, k, g, m, frac)
                checked += 1
    assert checked >= len(B.SHAPES)
