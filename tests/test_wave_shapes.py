"""CPU: the shape table of the triangle wave kernels (tests/wave_shapes.py).

* the table covers wave.hip: every ``MXD_SCATTER`` / ``MXD_SCATTER_B`` line
  and every gather ``(C, taps, Q)`` has a shape or a stated reason why no
  whole frame reaches it, so a kernel line added without a shape fails here;
* every recorded shape (and every named extra case) still plans its key, in
  u8 and f32, from every source base offset it is run from, in the recorded
  strip count;
* a bounded rerun of the finder still finds nothing for an unreachable key.
  Bounds of the rerun: 20 and 68 output rows only (the first of
  wave_shapes.ROWS_ONE / ROWS_TWO), at most 320 output columns, both aspects
  of wave_shapes.ASPECTS -- the full bounds are those of wave_shapes.find;
* on every frame of 64 x 64 and more the reference alone passes the project's
  gate: the kernel-order restatement O.resize_crop_vfirst against the
  stbir-order oracle within +-1 and 2e-3 differing channels (the numbers of
  tests/test_gpu_parity.py), on the seeds the GPU test uses."""
import pytest

import oracle as O
import wave_shapes as W
from gpu_util import compare, oracle_out, synth

MAX_FRAC = 2e-3


def test_the_table_covers_every_instantiation():
    keys = W.instantiations()
    assert len([k for k in keys if not W.is_gather(k)]) >= 32 and len([k for k in keys if W.is_gather(k)]) >= 72
    assert not set(W.SHAPES) & set(W.UNREACHABLE)
    missing = keys - set(W.SHAPES) - set(W.UNREACHABLE)
    stale = (set(W.SHAPES) | set(W.UNREACHABLE)) - keys
    assert not missing and not stale, ("without a shape", sorted(missing), "not in wave.hip", sorted(stale))
    assert all(isinstance(r, str) and r for r in W.UNREACHABLE.values())


def test_a_new_kernel_line_is_noticed(tmp_path):
    text = open(W.WAVE_HIP).read()
    anchor = "  MXD_SCATTER(2, 4, 8, 1, 4)\n"
    assert anchor in text
    p = tmp_path / "wave.hip"
    p.write_text(text.replace(anchor, anchor + "  MXD_SCATTER(2, 7, 17, 1, 4)\n"))
    assert W.instantiations(str(p)) - W.instantiations() == {(2, 7, 17, 1, 4)}


@pytest.mark.parametrize("key", sorted(W.SHAPES, key=lambda k: (len(k), k)), ids=str)
def test_every_shape_plans_its_key(key):
    one, two = W.SHAPES[key]
    assert one is not None or two is not None
    for k, shape in enumerate((one, two)):
        if shape is None:
            continue
        sw, sh, cw, ch, ns = shape
        assert ch % 8 != 0 and ch > 16 and (k == 0 or (cw >= 64 and ch >= 64))
        ok, got = W.planned(key, (sh, sw, W.channels_of(key)), W.whole(cw, ch), W.shifts_of(key) if k else (0,))
        assert ok and got == ns, (key, shape, got, W.plan((sh, sw, W.channels_of(key)), W.whole(cw, ch),
                                                          W.policy_of(key)))


@pytest.mark.parametrize("name", sorted(W.EXTRA))
def test_every_extra_case_plans_its_key(name):
    key, (sw, sh), (cw, ch) = W.EXTRA[name]
    assert key in W.SHAPES and ch % 8 != 0 and cw >= 64 and ch >= 64
    ok, _ = W.planned(key, (sh, sw, 3), W.whole(cw, ch), W.shifts_of(key))
    assert ok, (name, W.plan((sh, sw, 3), W.whole(cw, ch), W.policy_of(key)))


def test_extra_cases_run_on_a_deeper_schedule_or_a_larger_bucket():
    """What each named case is there for, from the product's own tap tables:
    the vertical table's depth (largest step of the last tap row) is below the
    planned DMAX, or the horizontal taps are below the planned bucket."""
    from mlx_data_amd import capi

    def depth(n_in, n_out):
        first, cnt, _ = capi.axis_taps(n_in, n_out)
        last = first + cnt - 1
        return int((last[1:] - last[:-1]).max())

    for name, (key, (sw, sh), (cw, ch)) in W.EXTRA.items():
        d, xw = depth(sh, ch), capi.axis_taps(sw, cw)[2].shape[1]
        if name.startswith("deeper"):
            assert d < key[1], (name, d)
        else:
            assert min(b for b in W._BUCKETS if b >= xw) < key[2], (name, xw)
    for name, dmax in (("deeper_7_to_1", 9), ("deeper_8_to_1", 9), ("deeper_10_5_to_1", 12), ("deeper_14_to_1", 16)):
        key, (sw, sh), (cw, ch) = W.EXTRA[name]
        assert key[1] == dmax and abs(sh / ch - float(name[7:-5].replace("_", "."))) < 0.01, name
    key, (sw, sh), (cw, ch) = W.EXTRA["larger_bucket_h1_5_v3_75"]
    assert (sw / cw, sh / ch) == (1.5, 3.75) and capi.axis_taps(sw, cw)[2].shape[1] < key[2]
    key, (sw, sh), (cw, ch) = W.EXTRA["deeper_h3_75_v1_9"]
    assert sw / cw == 3.75 and abs(sh / ch - 1.9) < 0.01 and depth(sh, ch) < key[1]


def test_unreachable_keys_stay_unreachable():
    for key in sorted(W.UNREACHABLE, key=lambda k: (len(k), k)):
        for strips in (1, 2):
            rows = (W.ROWS_TWO if strips == 2 else W.ROWS_ONE)[:1]
            assert W.find(key, strips, rows=rows, max_cols=320) is None, (key, strips)


def _frames():
    for key in sorted(W.SHAPES, key=lambda k: (len(k), k)):
        for k, shape in enumerate(W.SHAPES[key]):
            if shape is not None:
                yield key, k, shape[:2], shape[2:4]
    for name, (key, src, out) in sorted(W.EXTRA.items()):
        yield key, name, src, out


def test_the_reference_alone_passes_the_gate():
    checked = 0
    for key, k, (sw, sh), (cw, ch) in _frames():
        if cw < 64 or ch < 64:
            continue
        img = synth(sh, sw, W.channels_of(key), W.seed_of(key, k))
        for g in W.windows(cw, ch):
            if g[4] >= 64 and g[5] >= 64:
                m, frac = compare(O.resize_crop_vfirst(img, g), oracle_out(img, g))
                assert m <= 1 and frac < MAX_FRAC, (key, k, g, m, frac)
                checked += 1
    assert checked >= 2 * len(W.SHAPES)
