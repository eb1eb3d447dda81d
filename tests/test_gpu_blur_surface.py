"""GPU: image_gaussian_blur and image_random_gaussian_blur of the operator
surface.  The expectation is always the float32 restatement (tests/blur_ref.py)
on the uint8 result of the same chain without the op, then the statements of
what composes after it; compared as integer bits."""
import numpy as np
import pytest

import blur_ref as B
import color_ref as C
import tone_ref as T
from mlx_data_amd import _pipeline
from mlx_data_amd import data as dx
from out_format_util import IMAGENET_MEAN, IMAGENET_STD
from test_gpu_tone_surface import EQ, bits, chain, formatted, one_device, plan, samples  # noqa: F401  (one_device: autouse)

pytestmark = pytest.mark.gpu


def blurred(batch, k, sigma):
    return np.stack([B.blur_f32(np.ascontiguousarray(x), k, sigma) for x in batch])


@pytest.mark.parametrize("k,sigma", [(3, 2.0), (23, 2.0), (33, 0.5)])
def test_host_and_device_batches_and_what_composes_after_the_op(k, sigma):
    b = chain(dx.buffer_from_vector(samples(6, 3)))
    u8 = b.batch(6)[0]["image"]
    t = b.image_gaussian_blur("image", k, sigma)
    want = blurred(u8, k, sigma)
    assert not np.array_equal(want, u8)
    host = t.batch(6)[0]["image"]
    assert host.dtype == np.uint8 and host.shape == (6, 29, 33, 3) and np.array_equal(host, want), plan(t)["enhance"]
    assert np.array_equal(t[2]["image"], want[2])  # a direct read: a launch of its own
    assert np.array_equal(t.batch(6, device=0)[0]["image"].numpy(), want)
    # equalize (of the blurred bytes), a colour twist and image_normalize after the op
    tw = t.image_equalize("image").image_color_twist("image", 1.15, 0.8, 1.6, 25.0)
    eq = C.apply_ref(np.stack([T.pillow_apply(q, EQ) for q in want]), np.float32(plan(tw)["color"]))
    n = tw.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="float16", layout="chw")
    ref = formatted(eq, "float16", IMAGENET_MEAN, IMAGENET_STD, "chw")
    assert np.array_equal(bits(n.batch(6)[0]["image"]), ref)
    assert np.array_equal(bits(n.batch(6, device=0)[0]["image"].numpy()), ref)


def test_a_flip_after_the_op_equals_the_op_after_a_flip_and_a_crop_runs_it_first():
    r = dx.buffer_from_vector(samples(4, 7)).image_resize("image", 70, 40)
    u8 = r.batch(4)[0]["image"]
    t = r.image_gaussian_blur("image", 23, 2.0)
    want = blurred(u8, 23, 2.0)
    f = t.image_random_h_flip("image", 1.0)
    assert plan(f)["enhance"] is not None and plan(f)["flip"] and plan(f)["src_shape"] != [40, 70, 3]
    got = f.batch(4)[0]["image"]
    assert np.array_equal(got, want[:, :, ::-1])
    assert np.array_equal(got, r.image_random_h_flip("image", 1.0).image_gaussian_blur("image", 23, 2.0).batch(4)[0]["image"])
    # a crop after the op: the reflected edges are the uncropped window's
    a = t.image_center_crop("image", 20, 16)
    assert plan(a)["enhance"] is None and plan(a)["src_shape"] == [40, 70, 3]
    assert np.array_equal(a.batch(4)[0]["image"], want[:, 12:28, 25:45])


def test_if_form_on_half_the_samples():
    bufs, wants = [], []
    for k in range(4):
        b = chain(dx.buffer_from_vector(samples(1, 20 + k)))
        u8 = b[0]["image"]
        bufs.append(b.image_gaussian_blur_if(k % 2 == 0, "image", 5 + 2 * k, 0.5 + k))  # each its own k and sigma
        assert (plan(bufs[-1])["enhance"] is not None) == (k % 2 == 0)
        wants.append(B.blur_f32(u8, 5 + 2 * k, 0.5 + k) if k % 2 == 0 else u8)
    for device in (None, 0):
        got = _pipeline._merge(bufs, 0, device)["image"]
        assert np.array_equal(got.numpy() if device is not None else got, np.stack(wants)), device


def test_the_random_form_equals_the_fixed_op_with_the_restated_draws():
    b = chain(dx.buffer_from_vector(samples(4, 40)))
    u8 = b.batch(4)[0]["image"]
    dx.set_state(9)  # batch() prepares its samples in order on this thread: image k takes draw k
    got = b.image_random_gaussian_blur("image", 23, sigma=(0.1, 2.0)).batch(4)[0]["image"]
    words = np.random.RandomState(9)
    for k in range(4):
        r0, r1 = (int(words.randint(0, 2 ** 32, dtype=np.uint64)) for _ in range(2))
        s = (float(r0) + float(r1) * 4294967296.0) / 18446744073709551616.0 * (2.0 - 0.1) + 0.1
        assert np.array_equal(got[k], B.blur_f32(u8[k], 23, float(np.float32(s)))), k
