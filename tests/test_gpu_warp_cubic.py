"""GPU: bicubic images (warp_cubic.hip) through mxd_resize_crop_batch_warp on crop-only plans and the surface,
against Pillow's transform(AFFINE, BICUBIC) and the CPU statement; bits compared, padding must keep its 0xff."""
import numpy as np
import pytest

import tone_ref as T
import warp_ref as W
from mlx_data_amd import _pipeline
from mlx_data_amd import data as dx
from test_gpu_color import U8, Sources
from test_gpu_tone_surface import chain, one_device, samples  # noqa: F401 (one_device: autouse)
from test_gpu_warp import BF16_CHW, _check  # (the CPU statement must equal Pillow, the call must equal both)
from test_warp_cubic import CUBIC, FILL, image  # (and its Image.BICUBIC entry of warp_ref's mapping)

pytestmark = pytest.mark.gpu

KINDS = ["noise", "binary"]
# 1x1, 3x2: smaller than a neighbourhood; 61x33: row tails of 1 to 3 pixels, partial tiles; 130x35: 3 x 3 tiles
SIZES = [(1, 1), (3, 2), (61, 33), (130, 35)]
MATRICES = {"shear": lambda w, h: W.shear(0.3, -0.1), "translate": lambda w, h: W.translate(2.5, -1.25),
            "rotate-30": lambda w, h: W.rotate_matrix(w, h, 30.0), "rotate-45": lambda w, h: W.rotate_matrix(w, h, 45.0),
            "tiles-outside": lambda w, h: W.translate(70.5, 3.25),  # 130x35: one tile partly, two wholly outside
            "outside": lambda w, h: W.OUTSIDE}


def crop_only(imgs, windows):  # sources whose plans only crop: (x, y, w, h) windows of the images
    return Sources(imgs, [(i.shape[1], i.shape[0], x, y, w, h, 0) for i, (x, y, w, h) in zip(imgs, windows)])


def one_call(imgs, windows, warps, tag):
    src = crop_only(imgs, windows)
    try:
        _check(src, src.plain_u8(), warps, U8, tag)
    finally:
        src.free()


@pytest.fixture(scope="module", params=KINDS)
def windows(request):
    imgs = [image(request.param, 140, 40, 900 + k) for k in range(4)]
    src = crop_only(imgs, [(3 + k, 2 + k, w, h) for k, (w, h) in enumerate(SIZES)])
    yield src, src.plain_u8()
    src.free()


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one-byte-past"])
@pytest.mark.parametrize("name", list(MATRICES))
def test_small_windows_equal_pillow(windows, name, shift):
    src, plain = windows
    warps = [(CUBIC, FILL, MATRICES[name](g[4], g[5])) for g in src.geoms]
    _check(src, plain, warps, U8, name, dst_pad=2 * shift, dst_shift=shift)


@pytest.mark.parametrize("kind", KINDS)
def test_a_box_no_lds_holds_takes_the_gather_route(kind):
    """600x80 under (9.3, 0, 0, 0, 5, 0): the first tile's box is 48,000 pixels; beside it a shear, which is staged."""
    warps = [(CUBIC, FILL, (9.3, 0, 0, 0, 5, 0)), (CUBIC, FILL, W.shear(0.3, -0.1))]
    one_call([image(kind, 600, 80, 77)] * 2, [(0, 0, 600, 80)] * 2, warps, "gather")


def test_a_mixed_call_keeps_each_image_with_its_kernel():
    sizes = [(33, 20), (61, 33), (70, 18), (20, 40), (130, 35), (65, 17)]
    warps = [(W.NONE, 0, None), (CUBIC, FILL, W.rotate_matrix(61, 33, 30.0)), (W.NEAREST, 5, W.translate(2.5, -1.25)),
             (W.BILINEAR, (1, 2, 3), W.rotate_matrix(20, 40, 45.0)), (CUBIC, 77, W.shear(-0.2, 0.15)),
             (W.NEAREST, FILL, W.shear(0.3, -0.1))]
    one_call([image("noise", w + 4, h + 4, 40 + k) for k, (w, h) in enumerate(sizes)], [(2, 1, w, h) for w, h in sizes], warps,
             "mixed")


def test_cubic_then_equalize_then_bf16_chw(windows):
    src, plain = windows
    warps = [(CUBIC, (255, 0, 30), W.rotate_matrix(g[4], g[5], 30.0)) for g in src.geoms]
    _check(src, plain, warps, BF16_CHW, "chain", [(T.EQUALIZE, 0, 0.0)] * 4)


def test_the_surface_random_rotate_and_an_if_on_half_the_batch():
    b = chain(dx.buffer_from_vector(samples(4, 3)))
    u8 = b.batch(4)[0]["image"]
    t = b.image_random_affine_rotate("image", (-45, 45), resample="cubic", fill=FILL)
    dx.set_state(9)
    ms = [_pipeline._plan(t, k, "image")["warp"][2] for k in range(4)]  # the four draws, in order
    want = np.stack([W.pillow_apply(u8[k], (CUBIC, FILL, ms[k])) for k in range(4)])
    assert len(set(ms)) == 4 and not np.array_equal(want, u8)
    dx.set_state(9)
    assert np.array_equal(t.batch(4)[0]["image"], want)
    dx.set_state(9)
    assert np.array_equal(t.batch(4, device=0)[0]["image"].numpy(), want)
    bufs = [chain(dx.buffer_from_vector(samples(1, 20 + k))) for k in range(4)]
    want = np.stack([W.pillow_rotate(q[0]["image"], 30.0, CUBIC, FILL) if k % 2 == 0 else q[0]["image"]
                     for k, q in enumerate(bufs)])
    bufs = [q.image_affine_rotate_if(k % 2 == 0, "image", 30.0, resample="cubic", fill=FILL) for k, q in enumerate(bufs)]
    assert np.array_equal(_pipeline._merge(bufs, 0, None)["image"], want)
    assert np.array_equal(_pipeline._merge(bufs, 0, 0)["image"].numpy(), want)
