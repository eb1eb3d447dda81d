"""GPU: image_pil_gaussian_blur, image_random_pil_gaussian_blur and
image_pil_box_blur of the operator surface.  The expectation is always Pillow's
own ImageFilter on the uint8 result of the same chain without the op."""
import numpy as np
import pytest
from PIL import Image, ImageFilter

from mlx_data_amd import _pipeline
from mlx_data_amd import data as dx
from test_gpu_tone_surface import chain, one_device, plan, samples  # noqa: F401  (one_device: autouse)

pytestmark = pytest.mark.gpu


def pillow(batch, flt):
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(x)).filter(flt)) for x in batch])


@pytest.mark.parametrize("op,flt", [("image_pil_gaussian_blur", ImageFilter.GaussianBlur), ("image_pil_box_blur", ImageFilter.BoxBlur)])
@pytest.mark.parametrize("r", [0.3, 2.0])
def test_host_and_device_batches_equal_pillow(op, flt, r):
    b = chain(dx.buffer_from_vector(samples(6, 3)))
    u8 = b.batch(6)[0]["image"]
    t = getattr(b, op)("image", r)
    want = pillow(u8, flt(r))
    assert not np.array_equal(want, u8)
    host = t.batch(6)[0]["image"]
    assert host.dtype == np.uint8 and host.shape == (6, 29, 33, 3) and np.array_equal(host, want), plan(t)["enhance"]
    assert np.array_equal(t.batch(6, device=0)[0]["image"].numpy(), want)


def test_a_crop_after_the_op_is_the_crop_of_the_blur_and_a_flip_composes():
    r = dx.buffer_from_vector(samples(4, 7)).image_resize("image", 70, 40)
    t = r.image_pil_gaussian_blur("image", 2.0)
    want = pillow(r.batch(4)[0]["image"], ImageFilter.GaussianBlur(2.0))
    a = t.image_center_crop("image", 20, 16)  # the clamped edges are the uncropped window's
    assert plan(a)["enhance"] is None and plan(a)["src_shape"] == [40, 70, 3]
    assert np.array_equal(a.batch(4)[0]["image"], want[:, 12:28, 25:45])
    f = t.image_random_h_flip("image", 1.0)
    assert plan(f)["enhance"] is not None and plan(f)["flip"]
    assert np.array_equal(f.batch(4)[0]["image"], want[:, :, ::-1])


def test_if_form_on_half_the_samples():
    bufs, wants = [], []
    for k in range(4):
        b = chain(dx.buffer_from_vector(samples(1, 20 + k)))
        bufs.append(b.image_pil_gaussian_blur_if(k % 2 == 0, "image", 0.5 + k))  # each its own radius
        assert (plan(bufs[-1])["enhance"] is not None) == (k % 2 == 0)
        wants.append(pillow(b[0]["image"][None], ImageFilter.GaussianBlur(0.5 + k))[0] if k % 2 == 0 else b[0]["image"])
    for device in (None, 0):
        got = _pipeline._merge(bufs, 0, device)["image"]
        assert np.array_equal(got.numpy() if device is not None else got, np.stack(wants)), device


def test_the_random_form_equals_pillow_with_the_restated_draws():
    b = chain(dx.buffer_from_vector(samples(4, 40)))
    u8 = b.batch(4)[0]["image"]
    dx.set_state(9)  # batch() prepares its samples in order on this thread: image k takes draw k
    got = b.image_random_pil_gaussian_blur("image", radius=(0.1, 2.0)).batch(4)[0]["image"]
    words = np.random.RandomState(9)  # std::mt19937(seed); generate_canonical<double, 53>: two words a draw, low first
    for k in range(4):
        r0, r1 = (int(words.randint(0, 2 ** 32, dtype=np.uint64)) for _ in range(2))
        s = (float(r0) + float(r1) * 4294967296.0) / 18446744073709551616.0 * (2.0 - 0.1) + 0.1
        assert np.array_equal(got[k], pillow(u8[k][None], ImageFilter.GaussianBlur(float(np.float32(s))))[0]), k
