"""CPU: Random Erasing's statement (mxd_erase_apply, mxd_erase_normals) against
the plain NumPy of tests/erase_ref.py, the overlap rule, the casts, the
validation messages of mxd_erase_validate, and the operator surface's draws
and marked plan."""
import numpy as np
import pytest

import erase_ref as R
from mlx_data_amd import capi

H, W, BOX = 72, 80, (9, 5, 73, 69)  # a 64 x 64 box that begins and ends inside quads


@pytest.mark.parametrize("counter,key,words", R.KNOWN)
def test_philox_known_answers(counter, key, words):
    assert tuple(int(v) for v in capi.erase_normals(counter, key)[1]) == words
    assert tuple(int(v) for v in R.philox(counter, key)) == words


@pytest.mark.parametrize("seed", [(1, 2), (0xdeadbeef, 0x9e3779b9)])
@pytest.mark.parametrize("mode", [R.PIXEL, R.COLOR])
def test_noise_within_the_bound_and_equal_in_both_layouts(mode, seed):
    erase = (mode, [BOX], seed)
    hwc = capi.erase_apply(np.zeros((H, W, 3), np.float32), erase, capi.MXD_ERASE_F32)
    chw = capi.erase_apply(np.zeros((3, H, W), np.float32), erase, capi.MXD_ERASE_F32, chw=True)
    assert np.array_equal(hwc.view(np.uint32), chw.transpose(1, 2, 0).view(np.uint32))
    ref = R.apply(np.zeros((H, W, 3)), erase)
    err = np.abs(hwc - ref) / np.maximum(1.0, np.abs(ref))
    print("max error in units of the bound:", err.max() / R.BOUND)
    assert err.max() <= R.BOUND
    x0, y0, x1, y1 = BOX
    inside = np.zeros((H, W), bool)
    inside[y0:y1, x0:x1] = True
    assert not hwc[~inside].any() and np.count_nonzero(hwc[inside]) == 64 * 64 * 3
    if mode == R.PIXEL:
        assert abs(hwc[inside].mean()) < 0.05 and abs(hwc[inside].std() - 1) < 0.05
        assert len(np.unique(hwc[inside])) > 12000
    else:
        assert len(np.unique(hwc[inside])) == 3


def test_sixteen_bit_elements_round_to_nearest_even():
    erase = (R.PIXEL, [(0, 0, W, H)], (5, 6))
    f32 = capi.erase_apply(np.zeros((H, W, 3), np.float32), erase, capi.MXD_ERASE_F32)
    f16 = capi.erase_apply(np.zeros((H, W, 3), np.uint16), erase, capi.MXD_ERASE_F16)
    bf16 = capi.erase_apply(np.zeros((H, W, 3), np.uint16), erase, capi.MXD_ERASE_BF16)
    assert np.array_equal(f16, f32.astype(np.float16).view(np.uint16))
    u = f32.view(np.uint32).astype(np.uint64)
    assert np.array_equal(bf16, ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16))
    const = (R.CONST, [(1, 1, 3, 2)], None, (0.1, -2.5, 1e-6))
    got = capi.erase_apply(np.full((4, 4, 3), 7, np.uint16), const, capi.MXD_ERASE_F16)
    assert np.array_equal(got[1, 1:3], np.tile(np.array(const[3], np.float16).view(np.uint16), (2, 1)))
    assert (got[0] == 7).all() and (got[2:] == 7).all() and (got[1, 0] == 7).all() and (got[1, 3] == 7).all()


@pytest.mark.parametrize("mode", [R.CONST, R.COLOR, R.PIXEL])
def test_the_highest_numbered_box_wins(mode):
    boxes = [(2, 2, 30, 20), (10, 0, 40, 12), (0, 8, 18, 30), (12, 10, 14, 11)]
    erase = (mode, boxes, (3, 4), 1.0)
    got = capi.erase_apply(np.zeros((32, 44, 3), np.float32), erase, capi.MXD_ERASE_F32)
    owner = np.full((32, 44), -1)
    for b, (x0, y0, x1, y1) in enumerate(boxes):
        owner[y0:y1, x0:x1] = b
    for b, box in enumerate(boxes):
        alone = R.apply(np.zeros((32, 44, 3)), (mode, [(0, 0, 0, 0)] * b + [box], (3, 4), 1.0))
        assert np.allclose(got[owner == b], alone[owner == b], rtol=0, atol=R.BOUND * 6), b
    assert not got[owner < 0].any() and all((owner == b).any() for b in range(4))


def _refuses(erase, elem, needle, images=None):
    with pytest.raises(capi.MxdError) as info:
        capi.erase_validate(images, [erase], elem)
    assert needle in str(info.value) and "(image 0)" in str(info.value), str(info.value)


def test_validation_names_the_image_and_the_field():
    arr, _ = capi.make_images([dict(src=0, src_stride=30, src_w=10, src_h=8, channels=3, resize_w=10, resize_h=8,
                                    crop_x=0, crop_y=0, crop_w=10, crop_h=8, flip=0, dst=0, dst_stride=30)])
    ok = (R.CONST, [(0, 0, 10, 8)], None, 3.0)
    capi.erase_validate(arr, [ok], capi.MXD_ERASE_U8)
    _refuses((R.CONST, [(0, 0, 1, 1)] * 5), capi.MXD_ERASE_F32, "count 5 outside 0..4")
    _refuses((7, [(0, 0, 1, 1)]), capi.MXD_ERASE_F32, "unknown mode 7")
    _refuses((R.CONST, [(0, 0, 11, 8)]), capi.MXD_ERASE_F32, "box[0] needs 0 <= x0 <= x1 <= crop_w", arr)
    _refuses((R.CONST, [(0, 0, 1, 1), (0, 5, 4, 3)]), capi.MXD_ERASE_F32, "box[1] needs 0 <= y0 <= y1 <= crop_h", arr)
    _refuses((R.CONST, [(0, 0, 1, 1)], None, float("nan")), capi.MXD_ERASE_F32, "value[0] is not finite")
    _refuses((R.CONST, [(0, 0, 1, 1)], None, 2.5), capi.MXD_ERASE_U8, "value[0] must be an integer in 0..255")
    _refuses((R.PIXEL, [(0, 0, 1, 1)], (1, 2)), capi.MXD_ERASE_U8, "needs a float element type")
    bad = capi.make_erases([ok])[0]
    bad.reserved[3] = 1
    _refuses(bad, capi.MXD_ERASE_F32, "reserved must be 0")


# ---- the operator surface: draws and the marked plan ---------------------------------------

def _restated(words, h, w, prob, area, aspect, mode, count):
    """image_random_erasing's entry for one h x w image, restated from mt19937 words."""
    if not words.uniform() <= prob:
        return None
    n = count[0] if count[0] == count[1] else count[0] + words.below(count[1] - count[0] + 1)
    boxes = []
    for _ in range(n):
        for _ in range(10):
            target = (area[0] + (area[1] - area[0]) * words.uniform()) * (h * w) / n
            la, lb = np.log(aspect[0]), np.log(aspect[1])
            ratio = np.exp(la + (lb - la) * words.uniform())
            bh, bw = int(np.floor(np.sqrt(target * ratio) + 0.5)), int(np.floor(np.sqrt(target / ratio) + 0.5))
            if bw < w and bh < h:
                top = words.below(h - bh + 1)
                left = words.below(w - bw + 1)
                boxes.append((left, top, left + bw, top + bh))
                break
    if not boxes:
        return None
    seed = (words.word(), words.word()) if mode != "const" else (0, 0)
    return (mode, boxes, seed)


@pytest.mark.parametrize("mode,count", [("const", (1, 1)), ("pixel", (1, 1)), ("rand", (2, 4))])
def test_the_draw_stream_restated_from_mt19937_words(mode, count):
    from mlx_data_amd import _pipeline
    from mlx_data_amd import data as dx
    from test_mix import Words

    area, aspect = (0.02, 1 / 3), (0.3, 1 / 0.3)
    for seed, prob in ((21, 1.0), (22, 0.5), (23, 0.5), (24, 0.0)):
        dx.set_state(seed)
        got = [_pipeline._random_erasing_draws(29, 33, prob, area, aspect, mode, count if count[0] != count[1] else count[0])
               for _ in range(6)]
        words = Words(seed)
        want = [_restated(words, 29, 33, prob, area, aspect, mode, count) for _ in range(6)]
        assert got == want, (seed, got, want)
        for e in got:
            assert e is None or all(0 <= x0 < x1 <= 33 and 0 <= y0 < y1 <= 29 for x0, y0, x1, y1 in e[1])
    assert any(e is None for e in got) and prob == 0.0


def test_the_marked_plan_and_what_composes_or_materialises():
    from mlx_data_amd import _pipeline
    from mlx_data_amd import data as dx

    img = np.arange(40 * 50 * 3, dtype=np.uint8).reshape(40, 50, 3)
    base = dx.buffer_from_vector([dict(image=img)]).image_center_crop("image", 32, 24)
    dx.set_state(5)
    marked = base.image_normalize("image", dtype="bfloat16", layout="chw").image_random_erasing("image", prob=1.0, mode="pixel")
    plan = _pipeline._plan(marked, 0, "image")
    dx.set_state(5)
    assert plan["erase"] == _pipeline._random_erasing_draws(24, 32, prob=1.0, mode="pixel") and plan["erase"][0] == "pixel"
    assert _pipeline._plan(base.image_random_erasing("image", prob=0.0), 0, "image")["erase"] is None
    assert _pipeline._plan(base.image_random_erasing_if(False, "image", prob=1.0), 0, "image")["erase"] is None
    const = base.image_random_erasing("image", prob=1.0, value=7.0)
    assert _pipeline._plan(const, 0, "image")["erase"][0] == "const"
    for mode in ("rand", "pixel"):
        with pytest.raises(RuntimeError, match="image_to_float or image_normalize"):
            base.image_random_erasing("image", prob=1.0, mode=mode)[0]
    for kw in (dict(mode="noise"), dict(count=5), dict(count=(2, 1)), dict(area=(0.5, 0.1)), dict(aspect=(0.0, 1.0)),
               dict(prob=1.5)):
        with pytest.raises(ValueError, match="image_random_erasing"):
            base.image_random_erasing("image", **kw)
