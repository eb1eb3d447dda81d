"""The arithmetic-domain sweeps of tests/stage_domains.py without a device: every
builder precondition the device file (tests/test_gpu_stage_domains.py) relies on,
and every input through the CPU statements of the C ABI, against Pillow for the
tone, warp and enhance stages and against the NumPy statements for colour,
Gaussian blur and mix.  Every comparison is equality of bytes.

The contraction cases assert the witness property itself: at every witness the
exact unfused evaluator gives the reference's byte and the fused variant another,
so a reference (or CPU statement) that began to contract fails here."""
import time

import numpy as np
import pytest

import blur_ref as B
import color_ref as C
import enhance_ref as E
import mix_ref as M
import stage_domains as S
import tone_ref as T
import warp_ref as W
from mlx_data_amd import capi

AC, EQ = (T.AUTOCONTRAST, 0, 0.0), (T.EQUALIZE, 0, 0.0)


def _tone_three_ways(img, tone):
    """Pillow's bytes, which the NumPy restatement and the CPU statement must give too."""
    want = T.pillow_apply(img, tone)
    assert np.array_equal(T.apply(img, tone), want), tone
    assert np.array_equal(capi.tone_apply_u8(img, tone), want), tone
    return want


# ---- 1. tone ----------------------------------------------------------------------------------

def test_autocontrast_pairs_are_all_32640():
    pairs = S.autocontrast_pairs().reshape(-1, 2)
    assert len({(int(a), int(b)) for a, b in pairs}) == 32640 and (pairs[:, 0] < pairs[:, 1]).all()
    assert pairs.min() == 0 and pairs.max() == 255
    chunks = S.autocontrast_chunks()
    assert chunks[0][0] == 0 and chunks[-1][1] == 10883 and all(b - a <= 1024 for a, b in chunks)
    assert all(chunks[k][1] == chunks[k + 1][0] for k in range(len(chunks) - 1))


@pytest.mark.parametrize("chunk", S.autocontrast_chunks(), ids=lambda c: f"{c[0]}-{c[1]}")
def test_autocontrast_every_lo_hi(chunk):
    """Each channel holds every value of lo..hi and nothing outside; Pillow, the restatement
    and the CPU statement agree on every image of the chunk."""
    imgs, pairs = S.autocontrast_images()
    spent = 0.0
    for n in range(*chunk):
        for c in range(3):
            lo, hi = pairs[n, c]
            assert np.array_equal(np.unique(imgs[n, :, :, c]), np.arange(lo, hi + 1)), (n, c, lo, hi)
        t0 = time.perf_counter()
        want = T.pillow_apply(imgs[n], AC)
        spent += time.perf_counter() - t0
        got = capi.tone_apply_u8(imgs[n], AC)
        assert np.array_equal(got, want) and np.array_equal(T.apply(imgs[n], AC), want), (n, pairs[n].tolist())
        for c in range(3):
            if pairs[n, c, 0] == pairs[n, c, 1]:
                assert np.array_equal(want[..., c], imgs[n, :, :, c])  # one bin: the identity
    print(f"autocontrast chunk {chunk}: Pillow took {spent:.3f} s")
    assert spent < 2.0  # (a chunk's expectation must stay cheap for the device file)


def test_contrast_every_rounded_mean_under_every_factor():
    means = S.contrast_mean_images()
    assert sorted(means) == list(range(256))
    full = [m for m, (_, lo, hi) in means.items() if (lo, hi) == (0, 255)]
    assert sorted(full) == list(S.FULL_RAMP_MEANS)
    for m, (img, lo, hi) in means.items():
        assert T.mean_luma(img) == m
        assert np.array_equal(np.unique(img[..., 2]), np.arange(lo, hi + 1)), m
        for f in S.contrast_factors():
            _tone_three_ways(img, (T.CONTRAST, 0, f))


def test_contrast_means_on_the_rounding_boundary():
    ties = S.contrast_tie_images()
    assert len({k for k, _, _ in ties[:16]}) == 16 and ties[0][0] == 0 and ties[15][0] == 254
    for k, on, below in ties:
        n = on.shape[0] * on.shape[1]
        assert 2 * int(T.luma(on).sum()) == (2 * k + 1) * n and T.mean_luma(on) == k + 1  # exactly k + 0.5
        assert int(T.luma(below).sum()) == k * n + n // 2 - 1 and T.mean_luma(below) == k  # one luma step below
        assert set(np.unique(on)) == {k, k + 1} == set(np.unique(below))
        for f in S.contrast_factors():
            for img in (on, below):
                _tone_three_ways(img, (T.CONTRAST, 0, f))


def test_contrast_factors_reach_the_truncation_edge():
    """For each edge factor some image's ramp holds a v with m + f (v - m) exactly an integer."""
    means = S.contrast_mean_images()
    assert sum(0 < f < 1 for f in S.EDGE_FACTORS) >= 2 and sum(f > 1 for f in S.EDGE_FACTORS) >= 2
    for f in S.EDGE_FACTORS:
        hits = {m: S.contrast_integer_hits(f, m, range(lo, hi + 1)) for m, (_, lo, hi) in means.items()}
        assert sum(len(v) for v in hits.values()) > 1000, f
        m = 100
        v = hits[m][0]
        x = np.float32(m) + np.float32(f) * np.float32(v - m)
        assert x == np.trunc(x) and T.table(means[m][0], (T.CONTRAST, 0, f))[0, v] == int(np.clip(x, 0, 255))


@pytest.mark.parametrize("name", list(S.EQUALIZE_STEPS))
def test_equalize_histograms(name):
    img, steps = S.equalize_cases()[name]
    assert steps == S.EQUALIZE_STEPS[name]
    want = _tone_three_ways(img, EQ)
    for c, (step, bins) in enumerate(steps):
        if step == 0 or bins <= 1:
            assert np.array_equal(want[..., c], img[..., c])  # the gate: the identity
    if name == "zeros-five":
        assert want.max() == 255  # (0 + 395) / 1 without the min


def test_equalize_cases_cover_the_steps_named():
    steps = {s for v in S.EQUALIZE_STEPS.values() for s, _ in v}
    assert {0, 1, 16, 24} <= steps and set(S.EQUALIZE_STEPS) == set(S.equalize_cases())
    assert S.equalize_cases()["steps-64x64"][0].shape == (64, 64, 3)
    assert (64 * 64 - 1) // 255 == 16  # the largest step of a 64 x 64 image


def test_every_posterize_and_solarize_argument():
    img = S.all_bytes_image()
    assert all(np.array_equal(np.unique(img[..., c]), np.arange(256)) for c in range(3))
    tones = S.poster_solar_tones()
    assert len(tones) == 8 + 257
    for tone in tones:
        _tone_three_ways(img, tone)


# ---- 2. encode ties ---------------------------------------------------------------------------

def test_encode_ties_and_saturation():
    img = S.all_bytes_image()
    mats = S.tie_matrices()
    assert len(mats) == 31
    vals = np.concatenate([S.pre_encode(img, m).reshape(-1) for m in mats[:30]])
    exact = np.concatenate([(np.asarray(m, np.float64)[:, :3] @ img.reshape(-1, 3).T.astype(np.float64)
                             + np.asarray(m, np.float64)[:, 3:]).reshape(-1) for m in mats[:30]])
    assert np.array_equal(np.sort(vals.astype(np.float64)), np.sort(exact))  # every a q + t is exact in float32
    halves = vals[(vals > 0) & (vals < 255) & (vals * 2 == np.trunc(vals * 2)) & (vals != np.trunc(vals))]
    assert len(np.unique(halves)) >= 255  # every k + 0.5 of (0, 255)
    assert ((vals > -1) & (vals <= -0.5)).any() and (vals == -0.5).any()
    assert ((vals >= 254.5) & (vals <= 255.5)).any() and (vals == 254.5).any() and (vals == 255.5).any()
    near = S.pre_encode(img, mats[30]).reshape(-1)
    ties = np.trunc(near) + np.float32(0.5)
    below = np.unique(near[near == np.nextafter(ties, np.float32(-np.inf))])
    assert len(below) >= 3, below
    assert (np.asarray(S.NEIGHBOUR_ROWS)[:, :3] != 0).all()  # three-term rows
    for m in mats:
        want = C.apply_ref(img, m)
        assert np.array_equal(capi.color_apply_u8(img, m), want)
    # an exact tie rounds up, its neighbour below rounds down
    k = int(np.flatnonzero(near == below[0])[0])
    assert C.apply_ref(img, mats[30]).reshape(-1)[k] == int(below[0])


# ---- 3. contraction witnesses -------------------------------------------------------------------

def test_colour_witnesses():
    found = S.color_witnesses()
    mats = S.color_matrices()
    print({k: v[0] for k, v in found.items() if v[0]})
    for name in mats:
        assert sum(len(found[(name, c, "FULL")][1]) for c in range(3)) > 0, name
    for (name, c, variant), (_, tri) in found.items():
        for t in tri:
            unfused = S.color_byte(mats[name][c], t)
            assert unfused != S.color_byte(mats[name][c], t, S.COLOR_VARIANTS[variant]), (name, c, variant, t)
            assert C.apply_ref(t[None, :], mats[name])[0, c] == unfused, (name, c, t)
    for name, imgs in S.color_witness_images().items():
        for img in imgs:
            assert np.array_equal(capi.color_apply_u8(img, mats[name]), C.apply_ref(img, mats[name])), name


def test_mixup_witnesses():
    found = S.mix_witnesses()
    print({k: v[0] for k, v in found.items()})
    assert any(len(found[(lam, "FULL")][1]) for lam in S.MIX_LAMS)  # a lam of test_every_byte_pair_on_the_device
    q, r = M.byte_pair_grid()
    for (lam, variant), (n, pairs) in found.items():
        grid = M.mixup(q, r, lam)[..., 0]
        for a, b in pairs:
            unfused = S.mix_byte(a, b, lam)
            assert unfused != S.mix_byte(a, b, lam, S.MIX_VARIANTS[variant]) and grid[a, b] == unfused, (lam, a, b)
    for lam in S.MIX_LAMS:
        if not len(found[(lam, "FULL")][1]):
            continue
        own, partner = S.mix_witness_images(lam)
        want = M.mixup(own, partner, lam)
        assert np.array_equal(capi.mix_apply_u8(own, partner, M.entry_mixup(1, lam)), want)


def test_blend_witnesses():
    pairs, found = S.blend_pairs(), S.blend_witnesses()
    print({f: len(p) for f, p in pairs.items()}, {k: len(v[1]) for k, v in found.items()})
    assert set(pairs) == set(T.BLEND_FACTORS)
    assert {op for op, _ in found} == {E.COLOR, E.SHARPNESS}
    for f, p in pairs.items():
        assert (p[:, 0] != 0).all()  # D = 0, all BRIGHTNESS has, is never a witness
        assert bool(len(p)) == (((E.COLOR, f) in found) or ((E.SHARPNESS, f) in found))
    for (op, f), (img, at) in found.items():
        want = E.pillow_apply(img, (op, f))
        assert np.array_equal(E.apply(img, (op, f)), want) and np.array_equal(capi.enhance_apply_u8(img, (op, f)), want)
        deg = E.degenerate(img, op)
        for y, x, c, d, q in at:
            assert (deg[y, x, c], img[y, x, c]) == (d, q)
            assert want[y, x, c] == S.blend_byte(d, q, f) != S.blend_byte(d, q, f, True), (op, f, d, q)


@pytest.mark.parametrize("mode", [W.BILINEAR, S.CUBIC], ids=["bilinear", "bicubic"])
def test_warp_witnesses(mode):
    found = S.bilinear_witnesses() if mode == W.BILINEAR else S.bicubic_witnesses()
    mats = S.warp_matrices()
    print({k: len(v) for k, v in found.items()})
    assert sum(len(v) for k, v in found.items() if k.startswith("shear")) > 0
    for name, cases in found.items():
        inside, X, Y, dx, dy = S.warp_coords(mats[name])
        for img, x, y, names in cases:
            assert "FULL" in names and inside[y, x]
            want = S._pillow_warp(img, mode, mats[name])
            assert np.array_equal(capi.warp_apply_u8(img, (mode, S.FILL, mats[name])), want), (name, x, y)
            if mode == W.BILINEAR:
                p0, p1, q0, q1 = (int(img[Y[y, x] + j, X[y, x] + i, 0]) for j in (0, 1) for i in (0, 1))
                byte = lambda s: S.bilinear_byte(p0, p1, q0, q1, dx[y, x], dy[y, x], s)  # noqa: E731
                variants = S.BILINEAR_VARIANTS
            else:
                rows = img[Y[y, x] - 1: Y[y, x] + 3, X[y, x] - 1: X[y, x] + 3, 0].astype(int)
                across = (rows == rows[0]).all()  # equal rows: the row pass decides; else equal columns
                quad, d = (rows[0], dx[y, x]) if across else (rows[:, 0], dy[y, x])
                assert across or (rows == rows[:, :1]).all()
                byte = lambda s: S.bicubic_byte(quad, d, s)  # noqa: E731
                variants = S.CUBIC_VARIANTS
            assert want[y, x, 0] == byte(())
            for v in names:
                assert byte(variants[v]) != byte(()), (name, x, y, v)


@pytest.mark.parametrize("k,sigma", S.BLUR_KERNELS)
def test_blur_witnesses(k, sigma):
    w = capi.gaussian_weights(sigma, k)
    cases, counts = S.blur_witnesses(w, 5)
    print(counts)
    assert any("FULL" in names for *_, names in cases)
    variants = {"FULL": tuple(S.blur_sites(k)), **{f"{p}{d}": ((p, d),) for p, d in S.blur_sites(k)}}
    for img, y, x, c, names in cases:
        want = B.blur_f32(img, k, sigma)
        assert np.array_equal(S.blur_bytes(img[None], w)[0], want)  # the restatement is blur_ref's
        assert np.array_equal(capi.enhance_apply_u8(img, (capi.MXD_ENHANCE_GAUSSIAN_BLUR, sigma, k)), want)
        assert want[y, x, c] == S.blur_byte(img, w, y, x, c)
        for v in names:
            assert S.blur_byte(img, w, y, x, c, variants[v]) != want[y, x, c], (k, y, x, c, v)
