"""GPU: image_random_erasing of the operator surface.  The expectation is the
batch of the same chain without the op, with the float64 noise of
tests/erase_ref.py (within its bound) or the CPU statement's bits put into the
boxes and seed that _plan reports."""
import numpy as np
import pytest

import erase_ref as R
from gpu_util import synth
from mlx_data_amd import capi
from mlx_data_amd import data as dx
from out_format_util import IMAGENET_MEAN, IMAGENET_STD
from test_gpu_tone_surface import bits, chain, one_device, plan, samples  # noqa: F401  (one_device: autouse)

pytestmark = pytest.mark.gpu
MODES = {"const": R.CONST, "rand": R.COLOR, "pixel": R.PIXEL}


def entries(b, n, seed):
    """The erase entries batch() will draw: it prepares its samples in order on this thread."""
    dx.set_state(seed)
    out = [plan(b, k)["erase"] for k in range(n)]
    dx.set_state(seed)
    return [None if e is None else (MODES[e[0]], e[1], e[2], 0.0) for e in out]


def check_f32(got, base, ents):
    for g, b, e in zip(got, base, ents):
        ref = R.apply(b, e)
        inside = np.zeros(b.shape, bool)
        for x0, y0, x1, y1 in (e[1] if e is not None else []):
            inside[y0:y1, x0:x1] = True
        assert np.array_equal(bits(g)[~inside], bits(b)[~inside])
        assert (np.abs(g - ref) <= R.BOUND * np.maximum(1.0, np.abs(ref))).all()


def test_device_and_host_batches_and_if_on_half_a_batch():
    n = 6
    b = chain(dx.buffer_from_vector(samples(n, 3))).image_to_float("image")
    base = b.batch(n)[0]["image"]
    for mode in ("pixel", "rand", "const"):
        t = b.image_random_erasing("image", prob=0.6, mode=mode, count=(1, 3))
        ents = entries(t, n, 31)
        assert any(e is None for e in ents) and any(e is not None for e in ents)
        host = t.batch(n)[0]["image"]
        check_f32(host, base, ents)
        dx.set_state(31)
        assert np.array_equal(bits(t.batch(n, device=0)[0]["image"].numpy()), bits(host))
    # float16 CHW, against the CPU statement's bits; the _if form on every other buffer
    f = chain(dx.buffer_from_vector(samples(n, 3))).image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD,
                                                                     dtype="float16", layout="chw")
    t = f.image_random_erasing("image", prob=1.0, mode="pixel")
    want = bits(f.batch(n)[0]["image"]).copy()
    for k, e in enumerate(entries(t, n, 32)):
        capi.erase_apply(want[k], e, capi.MXD_ERASE_F16, chw=True)
    assert np.array_equal(bits(t.batch(n)[0]["image"]), want)
    assert plan(f.image_random_erasing_if(False, "image", prob=1.0))["erase"] is None
    # a uint8 const erase, and a flip after it works on its bytes
    u = chain(dx.buffer_from_vector(samples(2, 9))).image_random_erasing("image", prob=1.0, value=9.0)
    (x0, y0, x1, y1), = entries(u, 1, 33)[0][1]
    got = u.batch(1)[0]["image"][0]
    assert (got[y0:y1, x0:x1] == 9).all()
    dx.set_state(33)
    assert np.array_equal(u.image_random_h_flip("image", 1.0).batch(1)[0]["image"][0], got[:, ::-1])


def test_batch_mix_composes_and_a_batch_split_over_two_slices():
    n = 8
    b = chain(dx.buffer_from_vector(samples(n, 40))).image_to_float("image")
    t = b.image_random_erasing("image", prob=1.0, mode="pixel")
    ents = entries(t, n, 41)
    # the same draws with the erased images under another key: the mixed batch without erases
    base = b.image_random_erasing("image", prob=1.0, mode="pixel", output_key="other").batch_mix(n, "image", mixup_alpha=1.0)[0]
    dx.set_state(41)
    got = t.batch_mix(n, "image", mixup_alpha=1.0)[0]
    assert np.array_equal(got["mix_lam"], base["mix_lam"])
    check_f32(got["image"], base["image"], ents)
    n = 128
    s = dx.buffer_from_vector([dict(image=synth(24, 28, 3, 500 + i)) for i in range(n)]).image_resize("image", 20, 16)
    s = s.image_to_float("image")
    base = s.batch(n)[0]["image"]
    t = s.image_random_erasing("image", prob=0.5, mode="pixel")
    ents = entries(t, n, 42)
    dx.set_devices([0, 0])
    check_f32(t.batch(n)[0]["image"], base, ents)
