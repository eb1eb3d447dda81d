"""CPU: MXD_ENHANCE_GAUSSIAN_BLUR -- the weights, the CPU statement against the
float32 restatement and the float64 convolution (tests/blur_ref.py), the
refusals, and the operator surface's marked plan."""
import numpy as np
import pytest

import blur_ref as B
from mlx_data_amd import capi
from mlx_data_amd import data as dx
from test_enhance import _buf, _calls, _entry, _materialised, _plan

BLUR = capi.MXD_ENHANCE_GAUSSIAN_BLUR
KERNELS = [(3, 0.1), (3, 2.0), (23, 2.0), (33, 0.5), (33, 5.0)]


@pytest.mark.parametrize("k,sigma", KERNELS + [(5, 1e6), (33, 1e-3)])
def test_weights(k, sigma):
    w = capi.gaussian_weights(sigma, k)
    assert w.dtype == np.float32 and w.shape == (k,) and np.array_equal(w, w[::-1])
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= k * 2.0 ** -24
    x = np.arange(k, dtype=np.float64) - (k - 1) // 2
    p = np.exp(-0.5 * (x / np.float64(np.float32(sigma))) ** 2)
    ref = p / p.sum()
    flushed = ref.astype(np.float32) < 2.0 ** -126  # stored as 0: no float32 denormal reaches the device
    ulp = np.spacing(np.maximum(ref, 2.0 ** -126).astype(np.float32)).astype(np.float64)
    assert (w[flushed] == 0).all() and (np.abs(w.astype(np.float64) - ref) <= ulp)[~flushed].all()
    assert (k, sigma) != (33, 0.5) or flushed[:8].all()


@pytest.mark.parametrize("k,sigma", KERNELS)
@pytest.mark.parametrize("h,w", [(1, 1), (5, 2), (3, 17), (40, 37)])
def test_cpu_statement_equals_the_restatement_and_stays_by_the_float64_convolution(h, w, k, sigma):
    """The margin 2e-3 is derived: each pass has at most R + 3 rounded
    operations on magnitudes <= 255 at 2^-24 relative error, about 3e-4 per
    pass at R = 16, and the H error passes through V with weights summing to 1."""
    img = B.rand_image(h, w, 31 * h + w + k)
    got = capi.enhance_apply_u8(img, (BLUR, sigma, k))
    assert np.array_equal(got, B.blur_f32(img, k, sigma))
    f64 = B.blur_f64(img, k, sigma)
    assert np.abs(got - np.rint(f64)).max() <= 1
    far = np.abs(f64 - np.floor(f64) - 0.5) > 2e-3
    assert np.array_equal(got[far], np.rint(f64)[far].astype(np.uint8))
    # the mirrored image gives the mirrored result, bit for bit
    assert np.array_equal(capi.enhance_apply_u8(img[:, ::-1].copy(), (BLUR, sigma, k)), got[:, ::-1])


def _blur(sigma, k, r1=0):
    e = capi.MxdEnhance()
    e.op, e.factor = BLUR, sigma
    e.reserved[0], e.reserved[1] = k, r1
    return e


SIZE = "reserved[0] (the kernel size) must be odd and in 3..33"
SIGMA = "factor (sigma) must be finite, > 0 and at most 1e6"


@pytest.mark.parametrize("e,what", [
    (_blur(1.0, 4), SIZE), (_blur(1.0, 1), SIZE), (_blur(1.0, 35), SIZE), (_blur(0.0, 5), SIGMA), (_blur(-1.0, 5), SIGMA),
    (_blur(float("nan"), 5), SIGMA), (_blur(1.0, 5, 1), "reserved[1] must be 0"),
    ((capi.MXD_ENHANCE_COLOR, 1.0, 5), "reserved must be 0"), ((4, 1.0), "unknown op 4")])
def test_refusals_name_the_image_and_the_field(e, what):
    arr, n = capi.make_images([_entry(), _entry()])
    rcs, msg = _calls(arr, None, capi.make_enhances([(BLUR, 1.0, 3), e]), None, None, n, capi.MXD_U8, None)
    assert rcs == (capi.MXD_ERR_INVALID,) * 2 and msg == f"mxd_enhance: {what} (image 1)", (rcs, msg)
    with pytest.raises(RuntimeError):
        capi.enhance_apply_u8(B.rand_image(4, 4, 0), e)


@pytest.mark.parametrize("make,word", [
    (lambda b: b.image_gaussian_blur("image", 4, 1.0), "image_gaussian_blur: kernel_size must be odd and in 3..33"),
    (lambda b: b.image_gaussian_blur("image", 35, 1.0), "image_gaussian_blur: kernel_size must be odd and in 3..33"),
    (lambda b: b.image_gaussian_blur("image", 5, 0.0), "image_gaussian_blur: sigma must be finite, > 0 and at most 1e6"),
    (lambda b: b.to_stream().image_gaussian_blur("image", 5, float("nan")), "image_gaussian_blur: sigma must be finite, > 0"),
    (lambda b: b.image_random_gaussian_blur("image", 5, sigma=(2.0, 0.1)), "image_random_gaussian_blur: sigma range has lo > hi"),
    (lambda b: b.image_random_gaussian_blur("image", 5, sigma=1.0), "image_random_gaussian_blur: sigma must be a (lo, hi) pair"),
])
def test_surface_refuses_bad_arguments_when_the_op_is_made(make, word):
    with pytest.raises(ValueError) as err:
        make(_buf())
    assert word in str(err.value), str(err.value)


def test_the_op_marks_the_plan_and_composes_as_sharpness_does():
    with pytest.raises(RuntimeError) as err:
        _buf(c=4).image_random_gaussian_blur("image", 5)[0]
    assert str(err.value) == "image_random_gaussian_blur: image must have 3 channels, not 4"
    b = _buf().image_resize("image", 30, 20)
    q = _plan(b)
    t = b.image_gaussian_blur("image", 23, 0.1)
    p = _plan(t)
    assert p["enhance"] == ("gaussian_blur", float(np.float32(0.1)), 23)
    assert {k: p[k] for k in p if k != "enhance"} == {k: q[k] for k in q if k != "enhance"}
    e = _plan(t.image_equalize("image").image_color_twist("image", 1.2, 0.5).image_random_h_flip("image", 1.0)
              .image_normalize("image", mean=0.5, std=0.5, dtype="bfloat16", layout="chw"))
    assert e["enhance"] == p["enhance"] and e["tone"] == ("equalize", None) and e["flip"] and e["shape"] == [3, 20, 30]
    assert e["src_shape"] == [40, 60, 3] and e["format"]["dtype"] == "bfloat16"
    wp = _plan(b.image_shear("image", 0.3).image_random_gaussian_blur("image", 5, sigma=(2, 2)))
    assert wp["enhance"] == ("gaussian_blur", 2.0, 5) and wp["warp"] is not None
    assert _plan(b.image_gaussian_blur_if(False, "image", 5, 1.0))["enhance"] is None
    assert _plan(b.image_random_gaussian_blur_if(True, "image", 5, sigma=(1, 1)))["enhance"] == ("gaussian_blur", 1.0, 5)
    o = b.image_gaussian_blur("image", 3, 1.0, output_key="o")
    assert _plan(o, 0, "o")["enhance"] == ("gaussian_blur", 1.0, 3) and _plan(o, 0, "image")["enhance"] is None
    assert b.to_stream().image_gaussian_blur("image", 3, 1.0).image_random_gaussian_blur_if(False, "image", 3) is not None
    # a crop, a resize, a warp or a second enhance op after it, and the op after a tone or colour op, materialise
    for chain, check in (
            (lambda: t.image_center_crop("image", 10, 8), lambda m: m["enhance"] is None and m["crop"] == (10, 6, 10, 8)),
            (lambda: t.image_resize("image", 15, 10), lambda m: m["enhance"] is None and m["resize"] == (15, 10)),
            (lambda: t.image_shear("image", 0.3), lambda m: m["enhance"] is None and m["warp"] is not None),
            (lambda: t.image_sharpness("image", 0.5), lambda m: m["enhance"] == ("sharpness", 0.5)),
            (lambda: b.image_posterize("image", 4).image_gaussian_blur("image", 3, 1.0),
             lambda m: m["enhance"] == ("gaussian_blur", 1.0, 3) and m["tone"] is None),
            (lambda: b.image_color_twist("image", 1.2).image_gaussian_blur("image", 3, 1.0),
             lambda m: m["enhance"] == ("gaussian_blur", 1.0, 3) and m["color"] is None)):
        m = _materialised(chain)
        assert m is None or check(m), m


def test_the_random_form_draws_one_uniform_sigma_per_image():
    op = _buf(4).image_random_gaussian_blur("image", 23)  # sigma = (0.1, 2.0)
    dx.set_state(21)
    got = [_plan(op, i)["enhance"] for i in range(4)]
    words = np.random.RandomState(21)  # std::mt19937(seed); generate_canonical<double, 53>: two words a draw, low first
    for g in got:
        r0, r1 = (int(words.randint(0, 2 ** 32, dtype=np.uint64)) for _ in range(2))
        u = (float(r0) + float(r1) * 4294967296.0) / 18446744073709551616.0
        assert g == ("gaussian_blur", float(np.float32(u * (2.0 - 0.1) + 0.1)), 23)
    assert len({g[1] for g in got}) == 4
