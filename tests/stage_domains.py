"""Inputs that sweep the arithmetic domains of the stages behind the resize, and
their properties: pure NumPy / Pillow / fractions, nothing from the library, no
device.  tests/test_stage_domains.py asserts every property stated here and runs
the inputs through the CPU statements; tests/test_gpu_stage_domains.py runs the
same inputs through the device calls.

1. Tone tables over their whole domain: every AUTOCONTRAST (lo, hi), every
   rounded CONTRAST mean with its rounding boundary, adversarial EQUALIZE
   histograms, every POSTERIZE / SOLARIZE argument.
2. The colour map's encode on exact ties, their float32 neighbours and both
   saturation ends.
3. Contraction witnesses: inputs at which evaluating a statement with a fused
   multiply-add (one rounding for x*y + z) changes a result byte.  Each
   statement has an exact evaluator over fractions.Fraction whose `fused`
   argument names the contracted sites; the vectorised float64 scans are sieves
   only, and every witness kept is confirmed by the exact evaluator.

Sites and variants (FULL is every x*y + z of the expression, read left to right):
  colour   ((m0 q0 + m1 q1) + m2 q2) + m3: "0L" fma(m0, q0, m1 q1), "0R"
           fma(m1, q1, m0 q0), "1" fma(m2, q2, .); FULL = 0L + 1, ALT = 0R + 1.
  mixup    a l + b m: "L" fma(a, l, b m) = FULL, "R" fma(b, m, a l).
  blend    D + f (q - D): one site.
  bilinear a + (b - a) d: "h1", "h2" (the two rows), "v"; FULL = all three.
  bicubic  cub's three d * t + p: "t1", "t3", "r"; FULL = all three.
  blur     a + w[r + d] * pair in both passes: ("h", d), ("v", d); FULL = all.

What the searches find here (seeded; test_stage_domains.py prints the counts):
  colour   three twists and NEGATIVE, all (q0, q1) x 64 seeded q2 per row.
           FULL per row: twist-0 6 / 7 / 20, twist-1 11 / 11 / 11, twist-2
           72 / 85 / 261, NEGATIVE 0 / 0 / 9,414 (-q + 255 is exact; in
           0.5 q0 - 0.75 q1 + 0.3 q2 + 120 the ties of 0.3 q2 land on the same
           side either way); every single site has witnesses too; at most 64
           of a list are kept.
  mixup    lam 0.3: L 153 and R 128 of the 65,536 byte pairs; lam 0.5: none
           (both products are exact).
  blend    every (D, q) of every BLEND_FACTORS entry: 185 pairs at 3.7, none
           at any other factor; COLOR and SHARPNESS realise 12 each,
           BRIGHTNESS cannot (D = 0: 0 + f q has one rounding either way).
  bilinear every (a, b) at every fraction of four shear matrices: 12 kept a
           matrix; W.rotate_matrix(16, 16, 30): none (its fractions are
           generic doubles: no (b - a) d comes within an ulp of an integer).
  bicubic  the same matrices, on the quadruples (a, a, b, b) and 40,000
           seeded ones per fraction: 12 kept a shear matrix, 2 under the rotation.
  blur     sigma 2: k = 3 over 6,000 seeded 16 x 16 images FULL 19, h1 9, v1 14;
           k = 23 over 400 images FULL 2, h2 1, h4 1, v2 1, no other single site.
"""
import functools
from fractions import Fraction

import numpy as np
from PIL import Image

import color_ref as C
import enhance_ref as E
import tone_ref as T
import warp_ref as W

F32, F64 = 24, 53
CUBIC = 8  # MXD_WARP_BICUBIC
FILL = (10, 200, 90)


def geoms(images):
    """The crop-only plan of each image: resize to the source size, crop all of it."""
    return [(i.shape[1], i.shape[0], 0, 0, i.shape[1], i.shape[0], 0) for i in images]


# ---- exact arithmetic ---------------------------------------------------------------------

def rnd(x, bits):
    """x (a Fraction) rounded to the nearest value of `bits` significant bits, ties to
    even: one IEEE rounding (no value here is near the subnormal or overflow range)."""
    x = Fraction(x)
    if x == 0:
        return x
    a = abs(x)
    sh = a.numerator.bit_length() - a.denominator.bit_length() - bits
    s = a / Fraction(2) ** sh
    while s >= 2 ** bits:
        sh, s = sh + 1, s / 2
    while s < 2 ** (bits - 1):
        sh, s = sh - 1, s * 2
    assert sh > -140
    n = round(s) * Fraction(2) ** sh  # round(Fraction) is half to even
    return n if x > 0 else -n


def fr(v):
    return Fraction(float(v))


def trunc(x):
    return int(x) if x >= 0 else -int(-x)


# ---- 1. tone --------------------------------------------------------------------------------

def all_bytes_image():
    """16 x 16, every byte 0..255 in each channel: a ramp in R, its reverse in G, 167 p + 13 mod 256 in B."""
    p = np.arange(256)
    return np.stack([p, 255 - p, (167 * p + 13) % 256], axis=1).astype(np.uint8).reshape(16, 16, 3)


def autocontrast_pairs():
    """Every (lo, hi) with 0 <= lo < hi <= 255, as (10880, 3, 2): image n carries pairs [n] in its channels."""
    lo, hi = np.triu_indices(256, 1)
    pairs = np.stack([lo, hi], axis=1)
    assert pairs.shape == (32640, 2)
    return pairs.reshape(10880, 3, 2)


SINGLE_BIN = [((7, 7), (0, 255), (255, 255)), ((0, 0), (100, 100), (3, 200)), ((128, 129), (254, 254), (1, 1))]


@functools.lru_cache(None)
def autocontrast_images():
    """(10883, 16, 16, 3) uint8 and (10883, 3, 2) (lo, hi): channel c of image n is the
    ramp 0..255 clipped to lo..hi, so it holds every value of the range and nothing
    outside.  The last three images have single-bin channels (hi == lo: the identity)."""
    pairs = np.concatenate([autocontrast_pairs(), np.array(SINGLE_BIN)])
    ramp = np.arange(256)[None, :, None]
    imgs = np.clip(ramp, pairs[:, None, :, 0], pairs[:, None, :, 1]).astype(np.uint8)
    return imgs.reshape(-1, 16, 16, 3), pairs


AUTOCONTRAST_CHUNK = 1024


def autocontrast_chunks():
    n = len(autocontrast_images()[0])
    return [(a, min(a + AUTOCONTRAST_CHUNK, n)) for a in range(0, n, AUTOCONTRAST_CHUNK)]


def _mean_image(rg, b):
    img = np.empty((256, 3), np.uint8)
    img[:, 0], img[:, 1], img[:, 2] = rg, rg, b
    return img.reshape(16, 16, 3)


@functools.lru_cache(None)
def contrast_mean_images():
    """m -> (image, lowest, highest value of its ramp channel) for every m of 0..255 with
    int(mean_luma + 0.5) == m.  B carries the ramp (its luma weight is the smallest).
    A full 0..255 ramp with R = G = g constant reaches the means FULL_RAMP_MEANS; below
    them R = G = 0 and B holds 0..top once each and zeros (the largest top of that
    mean), above them R = G = 255 and B holds bottom..255 once each and 255s."""
    ramp = np.arange(256)
    out = {}
    for g in range(256):
        img = _mean_image(g, ramp)
        out.setdefault(T.mean_luma(img), (img, 0, 255))
    for top in range(255):
        img = _mean_image(0, np.where(ramp <= top, ramp, 0))
        m = T.mean_luma(img)
        if m not in out or (out[m][1] == 0 and out[m][2] < top):
            out[m] = (img, 0, top)
    for bottom in range(255, 0, -1):
        img = _mean_image(255, np.where(ramp >= bottom, ramp, 255))
        m = T.mean_luma(img)
        if m not in out or (out[m][2] == 255 and out[m][1] > bottom):
            out[m] = (img, bottom, 255)
    return out


FULL_RAMP_MEANS = range(15, 241)  # asserted by test_stage_domains.py
TIE_KS = tuple(int(k) for k in np.linspace(0, 254, 16))  # 0, 16, 33, ..., 254


def gray_pair_image(k, n_low, h=16, w=16):
    """n_low gray pixels of k, the others k + 1: luma of gray v is v, so the mean is k + (h w - n_low) / (h w)."""
    v = np.where(np.arange(h * w) < n_low, k, k + 1).astype(np.uint8)
    return np.repeat(v[:, None], 3, axis=1).reshape(h, w, 3)


def contrast_tie_images():
    """(k, image exactly on k + 0.5, image on the closest mean below it) for TIE_KS on
    16 x 16, then the same on 12 x 10 (120 pixels: S / N is no power-of-two division)."""
    out = [(k, gray_pair_image(k, 128), gray_pair_image(k, 129)) for k in TIE_KS]
    return out + [(k, gray_pair_image(k, 60, 10, 12), gray_pair_image(k, 61, 10, 12)) for k in (0, 101, 254)]


EDGE_FACTORS = (0.25, 0.75, 1.5, 2.5)  # two inside (0, 1), two outside


def contrast_factors():
    return tuple(T.CONTRAST_FACTORS) + EDGE_FACTORS


def contrast_integer_hits(f, m, values):
    """The v of `values` (v != m) at which m + f (v - m), evaluated in float32 as the
    statement does, is exactly an integer: the truncation edge."""
    f32 = np.float32(f)
    v = np.asarray(sorted(values), np.int64)
    x = np.float32(m) + f32 * (v - m).astype(np.float32)
    return [int(k) for k in v[(x == np.trunc(x)) & (v != m)]]


def channel_of(hist, seed=0):
    """The pixels of a 256-bin histogram, shuffled."""
    v = np.repeat(np.arange(256), np.asarray(hist, np.int64)).astype(np.uint8)
    np.random.default_rng(seed).shuffle(v)
    return v


def _hist(**bins):
    h = np.zeros(256, np.int64)
    for k, n in bins.items():
        h[int(k[1:])] = n
    return h


def _spread(total, last, seed):
    """`total` pixels: `last` in bin 255, the others over bins 0..254 (seeded, every bin non-empty)."""
    rng = np.random.default_rng(seed)
    h = np.ones(256, np.int64)
    h[:255] += np.bincount(rng.integers(0, 255, total - last - 255), minlength=255)
    h[255] = last
    return h


def equalize_step(channel):
    h = np.bincount(channel.reshape(-1), minlength=256)
    return int((channel.size - h[np.flatnonzero(h)[-1]]) // 255), int((h > 0).sum())


@functools.lru_cache(None)
def equalize_cases():
    """name -> (image, ((step, bins) per channel)): the histograms of the issue, one per channel."""
    def image(h, w, hists):
        return np.stack([channel_of(x, 7 + c) for c, x in enumerate(hists)], axis=1).reshape(h, w, 3)

    ones = np.ones(256, np.int64)

    def dominant(at):
        d = ones.copy()
        d[at] = 257
        return d

    cases = {
        # 17 x 16 = 272 pixels: npix - last = 254, 255, 256 -> step 0, 1, 1
        "two-bins-254-255-256": image(17, 16, [_hist(b30=254, b200=18), _hist(b30=255, b200=17), _hist(b30=256, b200=16)]),
        "all-bins-equal": image(16, 16, [ones, ones, ones]),
        # 32 x 16 = 512 pixels: 255 singletons and one bin of 257, first, in the middle and last
        "dominant-and-singletons": image(32, 16, [dominant(0), dominant(128), dominant(255)]),
        "last-bin-all-but-one": image(16, 16, [_hist(b0=1, b255=255), _hist(b77=1, b78=255), _hist(b254=1, b255=255)]),
        "zeros-five": T.zeros_five(),
        # 16 x 16: step is 0 or 1 only; largest 255 // 255, smallest non-zero the same, and 254 // 255 = 0
        "steps-16x16": image(16, 16, [_spread(256, 1, 1), _hist(b9=200, b10=55, b250=1), _hist(b9=254, b250=2)]),
        # 64 x 64: largest 4095 // 255 = 16, smallest non-zero 255 // 255 = 1, 254 // 255 = 0
        "steps-64x64": image(64, 64, [_spread(4096, 1, 2), _spread(4096, 4096 - 255, 3), _hist(b3=200, b40=54, b99=3842)]),
        # 96 x 64: 6143 // 255 = 24 (a 64 x 64 image cannot exceed 16)
        "step-24-96x64": image(96, 64, [_spread(6144, 1, 4), _spread(6144, 24, 5), _spread(6144, 3000, 6)]),
        "three-histograms": image(16, 16, [ones, _hist(b0=128, b255=128), _hist(b5=1, b6=100, b7=100, b200=55)]),
    }
    return {k: (v, tuple(equalize_step(v[..., c]) for c in range(3))) for k, v in cases.items()}


EQUALIZE_STEPS = {
    "two-bins-254-255-256": ((0, 2), (1, 2), (1, 2)), "all-bins-equal": ((1, 256),) * 3,
    "dominant-and-singletons": ((2, 256), (2, 256), (1, 256)), "last-bin-all-but-one": ((0, 2),) * 3,
    "zeros-five": ((1, 2),) * 3, "steps-16x16": ((1, 256), (1, 3), (0, 2)),
    "steps-64x64": ((16, 256), (1, 256), (0, 3)), "step-24-96x64": ((24, 256), (24, 256), (12, 256)),
    "three-histograms": ((1, 256), (0, 2), (0, 4)),
}


def poster_solar_tones():
    return [(T.POSTERIZE, b, 0.0) for b in range(1, 9)] + [(T.SOLARIZE, t, 0.0) for t in range(257)]


# ---- 2. encode ties ----------------------------------------------------------------------

TIE_A = (0.5, 1.5, 0.25, -0.5, -1.0)
TIE_T = (0.0, 0.5, -0.5, 254.5, 255.5, 127.5)
# three-term rows: 0.5 q0 + 0.5 on a tie, pulled below it by less than an ulp and rounded to the neighbour
NEIGHBOUR_ROWS = ((0.5, -3e-8, 1e-8, 0.5), (0.5, -6e-8, 2e-8, 0.5), (0.5, -1.5e-8, 0.5e-8, 0.5))


def tie_matrices():
    """30 diagonal matrices (a, t) and one of the three-term rows."""
    out = []
    for a in TIE_A:
        for t in TIE_T:
            m = np.zeros((3, 4), np.float32)
            m[0, 0] = m[1, 1] = m[2, 2] = a
            m[:, 3] = t
            out.append(m)
    return out + [np.array(NEIGHBOUR_ROWS, np.float32)]


def pre_encode(rgb, m):
    """The float32 value of the statement in front of the encode, (..., 3) float32."""
    m = np.asarray(m, np.float32).reshape(3, 4)
    q = [rgb[..., k].astype(np.float32) for k in range(3)]
    return np.stack([((m[c, 0] * q[0] + m[c, 1] * q[1]) + m[c, 2] * q[2]) + m[c, 3] for c in range(3)], axis=-1)


# ---- 3. contraction witnesses ---------------------------------------------------------------

KEEP = 64  # witnesses kept per list

# -- colour --

def color_matrices():
    """name -> matrix: the three twists of eight_matrices() and NEGATIVE."""
    e = C.eight_matrices()
    return {"twist-0": e[5], "twist-1": e[6], "twist-2": e[7], "negative": C.NEGATIVE}


COLOR_VARIANTS = {"FULL": ("0L", "1"), "ALT": ("0R", "1"), "0L": ("0L",), "0R": ("0R",), "1": ("1",)}


def _flushed(row):
    row = np.asarray(row, np.float32).copy()
    row[np.abs(row) < np.float32(2.0 ** -100)] = 0
    return row


def color_value(row, q, fused=()):
    """Exact: the float32 value of one matrix row at the bytes q, the sites of `fused` contracted."""
    m = [fr(v) for v in _flushed(row)]
    p = [m[k] * int(q[k]) for k in range(3)]
    if "0L" in fused:
        s = rnd(p[0] + rnd(p[1], F32), F32)
    elif "0R" in fused:
        s = rnd(rnd(p[0], F32) + p[1], F32)
    else:
        s = rnd(rnd(p[0], F32) + rnd(p[1], F32), F32)
    s = rnd(s + p[2], F32) if "1" in fused else rnd(s + rnd(p[2], F32), F32)
    return rnd(s + m[3], F32)


def encode(v):
    """trunc(clamp(v + 0.5, 0, 255)), the add a float32 operation."""
    return trunc(min(max(rnd(v + Fraction(1, 2), F32), 0), 255))


def color_byte(row, q, fused=()):
    return encode(color_value(row, q, fused))


def _color_scan(row, q2s):
    """variant -> (n, 3) triples of (all q0) x (all q1) x q2s whose byte differs from the
    unfused one: the float64 sieve (a float32 times a byte is exact in float64)."""
    m = _flushed(row)
    q = np.arange(256, dtype=np.float32)
    p32 = [m[k] * q for k in range(3)]
    p64 = [np.float64(m[k]) * q.astype(np.float64) for k in range(3)]
    s1 = {"": p32[0][:, None] + p32[1][None, :],
          "0L": (p64[0][:, None] + p32[1].astype(np.float64)[None, :]).astype(np.float32),
          "0R": (p32[0].astype(np.float64)[:, None] + p64[1][None, :]).astype(np.float32)}

    def byte(first, second):
        s = s1[first][:, :, None]
        s = (s.astype(np.float64) + p64[2][q2s]).astype(np.float32) if second else s + p32[2][q2s]
        return np.clip((s + m[3]) + np.float32(0.5), np.float32(0), np.float32(255)).astype(np.uint8)

    base = byte("", False)
    out = {}
    for name, sites in COLOR_VARIANTS.items():
        first = "0L" if "0L" in sites else "0R" if "0R" in sites else ""
        if (first == "0L" and m[0] == 0) or (first == "0R" and m[1] == 0) or ("1" in sites and not first and m[2] == 0):
            out[name] = np.zeros((0, 3), np.uint8)
            continue
        i = np.argwhere(byte(first, "1" in sites) != base)
        i[:, 2] = q2s[i[:, 2]]
        out[name] = i.astype(np.uint8)
    return out


@functools.lru_cache(None)
def color_witnesses():
    """(matrix name, row, variant) -> (found, kept (n <= KEEP, 3) triples), every kept one
    confirmed by the exact evaluator."""
    q2s = np.sort(np.random.default_rng(2024).choice(256, 64, replace=False))
    out = {}
    for name, m in color_matrices().items():
        for c in range(3):
            for variant, tri in _color_scan(m[c], q2s).items():
                sites = COLOR_VARIANTS[variant]
                pick = tri[np.linspace(0, len(tri) - 1, min(len(tri), KEEP)).astype(int)] if len(tri) else tri
                kept = [t for t in pick if color_byte(m[c], t) != color_byte(m[c], t, sites)]
                out[(name, c, variant)] = (len(tri), np.array(kept, np.uint8).reshape(-1, 3))
    return out


def pack_pixels(px):
    """(n, 3) pixels -> (k, 16, 16, 3): as few 16 x 16 images as hold them, zero padded."""
    px = np.asarray(px, np.uint8).reshape(-1, 3)
    k = max(1, -(-len(px) // 256))
    out = np.zeros((k * 256, 3), np.uint8)
    out[: len(px)] = px
    return out.reshape(k, 16, 16, 3)


def color_witness_images():
    """matrix name -> (k, 16, 16, 3): every kept triple of the matrix's rows and variants."""
    out = {}
    for name in color_matrices():
        px = [t for (n, c, v), (_, t) in color_witnesses().items() if n == name and len(t)]
        out[name] = pack_pixels(np.unique(np.concatenate(px), axis=0))
    return out


# -- mixup --

MIX_LAMS = (0.3, 0.5)  # test_gpu_mix.py::test_every_byte_pair_on_the_device
MIX_VARIANTS = {"FULL": "L", "R": "R"}


def mix_byte(a, b, lam, fused=""):
    l, m = fr(np.float32(float(lam))), fr(np.float32(1 - float(lam)))
    pa, pb = int(a) * l, int(b) * m
    if fused == "L":
        x = rnd(pa + rnd(pb, F32), F32)
    elif fused == "R":
        x = rnd(rnd(pa, F32) + pb, F32)
    else:
        x = rnd(rnd(pa, F32) + rnd(pb, F32), F32)
    return round(x)  # np.rint: half to even


@functools.lru_cache(None)
def mix_witnesses():
    """(lam, variant) -> (found, kept (n, 2) (own, partner) pairs) over all 65,536 byte pairs."""
    out = {}
    q = np.arange(256)
    for lam in MIX_LAMS:
        l, m = np.float32(float(lam)), np.float32(1 - float(lam))
        a32, b32 = q.astype(np.float32) * l, q.astype(np.float32) * m
        a64, b64 = q * np.float64(l), q * np.float64(m)
        base = np.rint(a32[:, None] + b32[None, :])
        for variant, site in MIX_VARIANTS.items():
            x = (a64[:, None] + b32.astype(np.float64)[None, :]) if site == "L" else (a32.astype(np.float64)[:, None] + b64[None, :])
            pairs = np.argwhere(np.rint(x.astype(np.float32)) != base)
            pick = pairs[np.linspace(0, len(pairs) - 1, min(len(pairs), KEEP)).astype(int)] if len(pairs) else pairs
            kept = [p for p in pick if mix_byte(p[0], p[1], lam) != mix_byte(p[0], p[1], lam, site)]
            out[(lam, variant)] = (len(pairs), np.array(kept, np.uint8).reshape(-1, 2))
    return out


def mix_witness_images(lam):
    """Two (16, 16, 3) images, own and partner, holding every kept pair of lam in all three channels."""
    pairs = np.unique(np.concatenate([p for (l, _), (_, p) in mix_witnesses().items() if l == lam]), axis=0)
    assert 0 < len(pairs) <= 256
    own, partner = (pack_pixels(np.repeat(pairs[:, k: k + 1], 3, axis=1))[0] for k in (0, 1))
    return own, partner


# -- the enhance blend --

def blend_byte(d, q, f, fused=False):
    """Exact: trunc (clipped for f outside [0, 1]) of (float32)D + f (float32)(q - D)."""
    f32 = np.float32(f)
    p = fr(f32) * (int(q) - int(d))
    x = rnd(int(d) + p, F32) if fused else rnd(int(d) + rnd(p, F32), F32)
    if not (0 <= f32 <= 1):
        x = min(max(x, 0), 255)
    return trunc(x)


@functools.lru_cache(None)
def blend_pairs():
    """factor -> (n, 2) (D, q): every pair of bytes at which the fused blend's byte differs."""
    out = {}
    v = np.arange(256)
    for f in T.BLEND_FACTORS:
        f32 = np.float32(f)
        diff = (v[None, :] - v[:, None]).astype(np.float32)
        d32 = v[:, None].astype(np.float32)
        unf = d32 + f32 * diff
        fus = (d32.astype(np.float64) + np.float64(f32) * diff.astype(np.float64)).astype(np.float32)
        if not (0 <= f32 <= 1):
            unf, fus = np.clip(unf, 0, 255), np.clip(fus, 0, 255)
        out[f] = np.argwhere(np.trunc(unf) != np.trunc(fus))
    return out


def _color_pixel(d, q):
    """An RGB pixel with luma d and a channel equal to q, or None."""
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for c in range(3):
        px = [a, b]
        px.insert(c, np.full_like(a, q))
        hit = np.argwhere(((19595 * px[0] + 38470 * px[1] + 7471 * px[2] + 32768) >> 16) == d)
        if len(hit):
            i, j = hit[len(hit) // 2]
            return c, (int(px[0][i, j]), int(px[1][i, j]), int(px[2][i, j]))
    return None


PER_FACTOR = 12


@functools.lru_cache(None)
def blend_witnesses():
    """(op, factor) -> (image, [(y, x, c, D, q)]): COLOR as pixels of luma D with a channel q,
    SHARPNESS as 3 x 3 tiles (centre q, neighbours n with (10 q + 16 n + 13) // 26 == D),
    kept where Pillow gives the unfused byte."""
    out = {}
    for f, pairs in blend_pairs().items():
        if not len(pairs):
            continue
        pick = pairs[np.linspace(0, len(pairs) - 1, min(len(pairs), 4 * PER_FACTOR)).astype(int)]
        img, at = np.zeros((16, 16, 3), np.uint8), []
        for d, q in pick:
            got = _color_pixel(int(d), int(q))
            if got and len(at) < PER_FACTOR:
                y, x = divmod(len(at), 16)
                img[y, x] = got[1]
                at.append((y, x, got[0], int(d), int(q)))
        out[(E.COLOR, f)] = _pillow_keeps(img, (E.COLOR, f), at)
        img, at = np.zeros((16, 16, 3), np.uint8), []
        for d, q in pick:
            ns = [n for n in range(256) if (10 * int(q) + 16 * n + 13) // 26 == d]
            if ns and len(at) < min(PER_FACTOR, 25):
                ty, tx = divmod(len(at), 5)
                img[3 * ty: 3 * ty + 3, 3 * tx: 3 * tx + 3] = ns[0]
                img[3 * ty + 1, 3 * tx + 1] = q
                at += [(3 * ty + 1, 3 * tx + 1, c, int(d), int(q)) for c in range(3)]
        out[(E.SHARPNESS, f)] = _pillow_keeps(img, (E.SHARPNESS, f), at)
    return {k: v for k, v in out.items() if v[1]}


def _pillow_keeps(img, enh, at):
    want = E.pillow_apply(img, enh)
    deg = E.degenerate(img, enh[0])
    return img, [(y, x, c, d, q) for y, x, c, d, q in at
                 if deg[y, x, c] == d and img[y, x, c] == q and want[y, x, c] == blend_byte(d, q, enh[1])]


# -- the warps --

def warp_matrices():
    return {"shear-x": W.shear(0.3, 0.0), "shear-y": W.shear(0.0, 0.3), "shear-xy": W.shear(-0.2, 0.15),
            "shear-gpu": W.shear(0.3, -0.1), "rotate-30": W.rotate_matrix(16, 16, 30.0)}


def warp_coords(m, w=16, h=16):
    """Pillow's source position of every output pixel, every operation a double one:
    inside (h, w), X, Y (floor of the position - 0.5) and the fractions dx, dy."""
    a = [np.float64(v) for v in m]
    xs, ys = np.arange(w) + 0.5, (np.arange(h) + 0.5)[:, None]
    sx = (a[0] * xs + a[1] * ys) + a[2]
    sy = (a[3] * xs + a[4] * ys) + a[5]
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    sx, sy = sx - 0.5, sy - 0.5
    X, Y = np.floor(sx).astype(int), np.floor(sy).astype(int)
    return inside, X, Y, sx - X, sy - Y


def lerp(a, b, d, fused=False):
    """Exact: a + (b - a) d in double, the subtraction exact (bytes or equal values)."""
    a, b = Fraction(a), Fraction(b)
    diff = rnd(b - a, F64)
    return rnd(a + diff * fr(d), F64) if fused else rnd(a + rnd(diff * fr(d), F64), F64)


def bilinear_byte(p0, p1, q0, q1, dx, dy, fused=()):
    v1 = lerp(p0, p1, dx, "h1" in fused)
    v2 = lerp(q0, q1, dx, "h2" in fused)
    return trunc(lerp(v1, v2, dy, "v" in fused))


BILINEAR_VARIANTS = {"FULL": ("h1", "h2", "v"), "h1": ("h1",), "h2": ("h2",), "v": ("v",)}


def cub(v, d, fused=()):
    """Exact: Pillow's BICUBIC macro as warp.cpp's cub states it, in double."""
    v1, v2, v3, v4 = (Fraction(int(x)) for x in v)
    d = fr(d)
    r = lambda x: rnd(x, F64)  # noqa: E731
    p2 = r(-v1 + v3)
    p3 = r(r(r(2 * r(v1 - v2)) + v3) - v4)
    p4 = r(r(r(-v1 + v2) - v3) + v4)
    t1 = r(p3 + d * p4) if "t1" in fused else r(p3 + r(d * p4))
    t3 = r(p2 + d * t1) if "t3" in fused else r(p2 + r(d * t1))
    return r(v2 + d * t3) if "r" in fused else r(v2 + r(d * t3))


def bicubic_byte(v, d, fused=()):
    """Four equal rows of v: the column pass of four equal values R returns R exactly."""
    x = cub(v, d, fused)
    return 0 if x <= 0 else 255 if x >= 255 else trunc(x)


CUBIC_VARIANTS = {"FULL": ("t1", "t3", "r"), "t1": ("t1",), "t3": ("t3",), "r": ("r",)}


LD = np.longdouble
# (where long double is no wider than double the sieves below find nothing and the warp tests say so)


def _fractions(m, axis):
    """(d, dx, dy, x, y, index) per distinct non-dyadic fraction d along `axis` (0: dx, 1: dy) of an
    inside pixel whose neighbourhood lies within the 16 x 16 image."""
    inside, X, Y, dx, dy = warp_coords(m)
    d, i = (dx, X) if axis == 0 else (dy, Y)
    ok = inside & (X >= 1) & (X <= 13) & (Y >= 1) & (Y <= 13) & (d * 1024 != np.floor(d * 1024))
    seen = {}
    for y, x in np.argwhere(ok):
        seen.setdefault(float(d[y, x]), (float(d[y, x]), float(dx[y, x]), float(dy[y, x]), int(x), int(y), int(i[y, x])))
    return list(seen.values())


def edge_image(values, index, axis):
    """16 x 16 gray, constant along the other axis.  Two values: lines (columns for axis 0, rows for
    axis 1) up to `index` hold the first, the others the second.  Four: lines up to index - 1, index,
    index + 1, and from index + 2 on."""
    k = np.clip(np.arange(16) - (index - 1 if len(values) == 4 else index), 0, len(values) - 1)
    line = np.asarray(values, np.uint8)[k]
    img = np.repeat(line[None, :], 16, axis=0) if axis == 0 else np.repeat(line[:, None], 16, axis=1)
    return np.ascontiguousarray(np.repeat(img[:, :, None], 3, axis=2))


def _pillow_warp(img, mode, m):
    res = Image.BICUBIC if mode == CUBIC else W.RESAMPLE[mode]
    return np.asarray(Image.fromarray(img).transform((16, 16), Image.AFFINE, tuple(float(v) for v in m), res, fillcolor=FILL))


PER_MATRIX = 12
_A, _B = (g.reshape(-1) for g in np.meshgrid(np.arange(256.0), np.arange(256.0), indexing="ij"))


@functools.lru_cache(None)
def bilinear_witnesses():
    """matrix name -> [(image, x, y, variants that differ)]: edge images (a up to the source line, b from
    the next) at which Pillow gives the unfused byte and at least one variant another.  The sieve
    over every (a, b) of every fraction is a long double fused multiply-add (a 9-bit by 53-bit
    product is exact in 64 bits)."""
    out = {}
    for name, m in warp_matrices().items():
        found = []
        for axis in (0, 1):
            for d, dx, dy, x, y, i in _fractions(m, axis):
                r = _A + (_B - _A) * d
                fused = (_A.astype(LD) + (_B - _A).astype(LD) * LD(d)).astype(np.float64)
                for k in np.flatnonzero(np.trunc(r) != np.trunc(fused))[:PER_MATRIX]:
                    p, q = int(_A[k]), int(_B[k])
                    pq = (p, q, p, q) if axis == 0 else (p, p, q, q)
                    base = bilinear_byte(*pq, dx, dy)
                    names = [v for v, s in BILINEAR_VARIANTS.items() if bilinear_byte(*pq, dx, dy, s) != base]
                    if "FULL" not in names or len(found) >= PER_MATRIX:
                        continue
                    img = edge_image((p, q), i, axis)
                    if _pillow_warp(img, W.BILINEAR, m)[y, x, 0] == base:
                        found.append((img, x, y, tuple(names)))
        out[name] = found
    return out


@functools.lru_cache(None)
def bicubic_witnesses():
    """matrix name -> [(image, x, y, variants that differ)]: edge images of four values around the source
    line; the quadruples searched are (a, a, b, b) for every a, b and 40,000 seeded ones per fraction,
    sieved in long double."""
    out = {}
    rng = np.random.default_rng(77)
    for name, m in warp_matrices().items():
        found = []
        for axis in (0, 1):
            for d, dx, dy, x, y, i in _fractions(m, axis):
                rand = rng.integers(0, 256, (40000, 4)).astype(np.float64)
                v = np.concatenate([np.stack([_A, _A, _B, _B], axis=1), rand])
                v1, v2, v3, v4 = v.T
                p2, p3, p4 = -v1 + v3, (2.0 * (v1 - v2) + v3) - v4, ((-v1 + v2) - v3) + v4
                r = v2 + d * (p2 + d * (p3 + d * p4))
                t1 = (p3.astype(LD) + LD(d) * p4.astype(LD)).astype(np.float64)
                t3 = (p2.astype(LD) + LD(d) * t1.astype(LD)).astype(np.float64)
                fused = (v2.astype(LD) + LD(d) * t3.astype(LD)).astype(np.float64)
                hit = (np.trunc(r) != np.trunc(fused)) & (r > 0) & (r < 255)
                for quad in v[hit][:PER_MATRIX].astype(int):
                    base = bicubic_byte(quad, d)
                    names = [n for n, s in CUBIC_VARIANTS.items() if bicubic_byte(quad, d, s) != base]
                    if "FULL" not in names or len(found) >= PER_MATRIX:
                        continue
                    img = edge_image(tuple(quad), i, axis)
                    if _pillow_warp(img, CUBIC, m)[y, x, 0] == base:
                        found.append((img, x, y, tuple(names)))
        out[name] = found
    return out


# -- gaussian blur --

BLUR_KERNELS = ((3, 2.0), (23, 2.0))
BLUR_IMAGES = {3: 6000, 23: 400}  # seeded 16 x 16 images searched per kernel size


def reflect(i, n):
    i = np.mod(np.asarray(i), 2 * (n - 1))
    return np.where(i < n, i, 2 * (n - 1) - i)


def blur_sites(k):
    r = (k - 1) // 2
    return [("h", d) for d in range(1, r + 1)] + [("v", d) for d in range(1, r + 1)]


def blur_bytes(imgs, w, fused=()):
    """The statement of blur_ref.blur_f32 on (n, h, w, 3) images with weights w, the sites of
    `fused` contracted through float64 (a sieve: the sum may round twice)."""
    w = np.asarray(w, np.float32)
    r = (len(w) - 1) // 2
    h_, w_ = imgs.shape[1:3]
    q = imgs.astype(np.int32)
    xs, ys = np.arange(w_), np.arange(h_)

    def add(acc, wt, pair, site):
        if site in fused:
            return (acc.astype(np.float64) + np.float64(wt) * pair.astype(np.float64)).astype(np.float32)
        return acc + wt * pair

    a = w[r] * q.astype(np.float32)
    for d in range(1, r + 1):
        pair = (q[:, :, reflect(xs - d, w_)] + q[:, :, reflect(xs + d, w_)]).astype(np.float32)
        a = add(a, w[r + d], pair, ("h", d))
    v = w[r] * a
    for d in range(1, r + 1):
        v = add(v, w[r + d], a[:, reflect(ys - d, h_)] + a[:, reflect(ys + d, h_)], ("v", d))
    assert v.dtype == np.float32
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def blur_byte(img, w, y, x, c, fused=()):
    """Exact: one result byte of the statement, the sites of `fused` contracted."""
    wt = [fr(v) for v in np.asarray(w, np.float32)]
    r = (len(wt) - 1) // 2
    h_, w_ = img.shape[:2]

    def add(acc, k, pair, site):
        return rnd(acc + wt[k] * pair, F32) if site in fused else rnd(acc + rnd(wt[k] * pair, F32), F32)

    @functools.lru_cache(None)
    def row(yy):
        a = rnd(wt[r] * int(img[yy, x, c]), F32)
        for d in range(1, r + 1):
            pair = int(img[yy, int(reflect(x - d, w_)), c]) + int(img[yy, int(reflect(x + d, w_)), c])
            a = add(a, r + d, pair, ("h", d))
        return a

    v = rnd(wt[r] * row(y), F32)
    for d in range(1, r + 1):
        pair = rnd(row(int(reflect(y - d, h_))) + row(int(reflect(y + d, h_))), F32)
        v = add(v, r + d, pair, ("v", d))
    return min(max(round(v), 0), 255)


def blur_witnesses(w, seed):
    """[(image, y, x, c, variants)] for weights w: of BLUR_IMAGES[k] seeded 16 x 16 images, up to eight
    with a FULL witness and the first with a witness of each single site not among those."""
    k = len(w)
    imgs = np.random.default_rng(seed).integers(0, 256, (BLUR_IMAGES[k], 16, 16, 3), dtype=np.uint8)
    base = blur_bytes(imgs, w)
    variants = {"FULL": tuple(blur_sites(k)), **{f"{p}{d}": ((p, d),) for p, d in blur_sites(k)}}
    out, counts = {}, {}
    for name, sites in variants.items():
        hits = np.argwhere(blur_bytes(imgs, w, sites) != base)
        counts[name] = len(hits)
        kept = 0
        for n, y, x, c in hits:
            if kept >= (8 if name == "FULL" else 1):
                break
            if blur_byte(imgs[n], w, y, x, c) != blur_byte(imgs[n], w, y, x, c, sites):
                out.setdefault((int(n), int(y), int(x), int(c)), []).append(name)
                kept += 1
    return [(imgs[n], y, x, c, tuple(v)) for (n, y, x, c), v in out.items()], counts
