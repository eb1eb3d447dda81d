"""NumPy restatement of the tone operations' arithmetic (DESIGN.md section 2;
include/mxd_amd.h, mxd_tone): the 3 x 256 byte table of an operation for the
RGB pixels it is given, and the pixels looked up in it.  Shares nothing with
csrc/tone.cpp or csrc/row_stage.hip.  The arithmetic is Pillow's, so
pillow_apply() -- the calls timm's and torchvision's PIL policies make -- is
the independent yardstick the tests hold both against."""
import numpy as np

NONE, POSTERIZE, SOLARIZE, AUTOCONTRAST, EQUALIZE, CONTRAST = range(6)
NAMES = ("none", "posterize", "solarize", "autocontrast", "equalize", "contrast")

POSTERIZE_BITS = tuple(range(1, 9))
SOLARIZE_THRESHOLDS = (0, 1, 128, 255, 256)
CONTRAST_FACTORS = (0, 0.1, 0.5, 0.9, 1, 1.3, 1.9, 3.7)
BLEND_FACTORS = (0, 0.05, 0.1, 0.3, 0.5, 0.7, 0.9, 0.95, 1, 1.05, 1.3, 1.9, 2.5, 3.7, 10)


def all_tones():
    """Every (op, arg, factor) the CPU tests run."""
    return ([(POSTERIZE, b, 0.0) for b in POSTERIZE_BITS] + [(SOLARIZE, t, 0.0) for t in SOLARIZE_THRESHOLDS] +
            [(AUTOCONTRAST, 0, 0.0), (EQUALIZE, 0, 0.0)] + [(CONTRAST, 0, f) for f in CONTRAST_FACTORS])


def luma(rgb):
    q = rgb.reshape(-1, 3).astype(np.int64)
    return (19595 * q[:, 0] + 38470 * q[:, 1] + 7471 * q[:, 2] + 32768) >> 16


def mean_luma(rgb):
    """m = (int)((double)S / (double)N + 0.5)."""
    l = luma(rgb)
    return int(np.float64(int(l.sum())) / np.float64(l.size) + 0.5)


def contrast_row(m, f):
    """The 256 bytes of CONTRAST's table for mean m and factor f: float32
    operations, each rounded."""
    f = np.float32(f)
    v = np.arange(256, dtype=np.int64)
    d = (v - m).astype(np.float32)
    x = np.float32(m) + f * d  # float32 * float32 and float32 + float32: NumPy rounds each
    assert x.dtype == np.float32
    if 0 <= f <= 1:
        return np.trunc(x).astype(np.int64).astype(np.uint8)
    return np.where(x <= 0, 0, np.where(x >= 255, 255, np.trunc(x))).astype(np.uint8)


def table(rgb, tone):
    """The (3, 256) uint8 table of tone = (op, arg, factor) for (..., 3) uint8 pixels."""
    op, arg, factor = tone
    v = np.arange(256, dtype=np.int64)
    ident = np.tile(v.astype(np.uint8), (3, 1))
    if op == NONE:
        return ident
    if op == POSTERIZE:
        return np.tile((v & ((0xFF << (8 - arg)) & 0xFF)).astype(np.uint8), (3, 1))
    if op == SOLARIZE:
        return np.tile(np.where(v < arg, v, 255 - v).astype(np.uint8), (3, 1))
    px = rgb.reshape(-1, 3)
    n = px.shape[0]
    if op == CONTRAST:
        return np.tile(contrast_row(mean_luma(px), factor), (3, 1))
    t = ident.copy()
    for c in range(3):
        hist = np.bincount(px[:, c], minlength=256).astype(np.int64)
        nz = np.flatnonzero(hist)
        if op == AUTOCONTRAST:
            lo, hi = int(nz[0]), int(nz[-1])
            if hi <= lo:
                continue
            scale = np.float64(255.0) / np.float64(hi - lo)
            offset = np.float64(-lo) * scale
            x = v.astype(np.float64) * scale + offset
            t[c] = np.clip(np.trunc(x), 0, 255).astype(np.uint8)
        else:
            if nz.size <= 1:
                continue
            step = (n - int(hist[nz[-1]])) // 255
            if step == 0:
                continue
            before = np.concatenate([[0], np.cumsum(hist)[:-1]])
            t[c] = np.minimum(255, (step // 2 + before) // step).astype(np.uint8)
    return t


def apply(rgb, tone):
    t = table(rgb, tone)
    return np.stack([t[c][rgb[..., c]] for c in range(3)], axis=-1)


def pillow_apply(rgb, tone):
    """The same operation by Pillow on an (H, W, 3) uint8 image."""
    from PIL import Image, ImageEnhance, ImageOps

    op, arg, factor = tone
    im = Image.fromarray(np.ascontiguousarray(rgb), "RGB")
    if op == POSTERIZE:
        im = ImageOps.posterize(im, arg)
    elif op == SOLARIZE:
        im = ImageOps.solarize(im, arg)
    elif op == AUTOCONTRAST:
        im = ImageOps.autocontrast(im)
    elif op == EQUALIZE:
        im = ImageOps.equalize(im)
    elif op == CONTRAST:
        im = ImageEnhance.Contrast(im).enhance(factor)
    return np.asarray(im)


def ref_images():
    """The seeded images of the CPU tests, by name."""
    rng = np.random.default_rng(1234)
    out = {
        "random-5x7": rng.integers(0, 256, (5, 7, 3), dtype=np.uint8),
        "mid-33x65": rng.integers(40, 200, (33, 65, 3), dtype=np.uint8),
        "random-224": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8),
        "random-300": rng.integers(0, 256, (300, 300, 3), dtype=np.uint8),
        "constant-9x9": np.full((9, 9, 3), 77, np.uint8),
        "two-level-16": two_level(),
        "gauss-64": np.clip(rng.normal(128, 6, (64, 64, 3)).round(), 0, 255).astype(np.uint8),
    }
    g = rng.integers(0, 256, (300, 300, 3), dtype=np.uint8)
    g[..., 1] = 255
    g[17, 203, 1] = 3
    out["green-255-but-one"] = g
    out["zeros-five-255"] = zeros_five()
    return out


def two_level(h=16, w=16):
    """20 and 220 in a checkerboard of 2 x 2 blocks."""
    y, x = np.mgrid[:h, :w]
    a = np.where(((y // 2) + (x // 2)) % 2 == 0, 20, 220).astype(np.uint8)
    return np.repeat(a[..., None], 3, axis=2)


def zeros_five(h=20, w=20):
    """Zeros with five pixels of 255: step = (400 - 5) / 255 = 1, so the level
    255 maps to (0 + 395) / 1 without the min(255)."""
    z = np.zeros((h, w, 3), np.uint8)
    for y, x in ((0, 0), (3, 17), (9, 9), (15, 2), (19, 19)):
        z[y, x] = 255
    return z
