"""What the enhance tests share: the NumPy restatement of an enhance op
(op, factor) on an (h, w, 3) uint8 image -- the definition in
include/mxd_amd.h, integer stencil and float32 blend -- and Pillow itself
(ImageEnhance.Sharpness / Color / Brightness) as the reference."""
import numpy as np
from PIL import Image, ImageEnhance

NONE, SHARPNESS, COLOR, BRIGHTNESS = 0, 1, 2, 3
OPS = [SHARPNESS, COLOR, BRIGHTNESS]
OP_IDS = ["sharpness", "color", "brightness"]
PIL_ENHANCER = {SHARPNESS: ImageEnhance.Sharpness, COLOR: ImageEnhance.Color, BRIGHTNESS: ImageEnhance.Brightness}


def degenerate(img, op):
    """The degenerate image D of the definition, as int32."""
    q = img.astype(np.int32)
    h, w = q.shape[:2]
    if op == BRIGHTNESS:
        return np.zeros_like(q)
    if op == COLOR:
        luma = (19595 * q[..., 0] + 38470 * q[..., 1] + 7471 * q[..., 2] + 32768) >> 16
        return np.repeat(luma[..., None], 3, axis=2)
    d = q.copy()
    if w >= 3 and h >= 3:
        s = 4 * q[1:-1, 1:-1]
        for dy in range(3):
            for dx in range(3):
                s = s + q[dy:dy + h - 2, dx:dx + w - 2]
        d[1:-1, 1:-1] = (2 * s + 13) // 26
    return d


def apply(img, enhance):
    """The restatement: x = (float32)D + f * (float32)(q - D), each operation rounded to float32."""
    op, factor = enhance
    if op == NONE:
        return img.copy()
    f = np.float32(factor)
    d = degenerate(img, op)
    diff = (img.astype(np.int32) - d).astype(np.float32)
    x = d.astype(np.float32) + (f * diff).astype(np.float32)
    assert x.dtype == np.float32
    if not (np.float32(0) <= f <= np.float32(1)):
        x = np.clip(x, np.float32(0), np.float32(255))
    return np.trunc(x).astype(np.uint8)


def pillow_apply(img, enhance):
    """ImageEnhance.<op>(image).enhance(factor) of an (h, w, 3) uint8 array."""
    op, factor = enhance
    if op == NONE:
        return img.copy()
    pil = Image.fromarray(np.ascontiguousarray(img))
    return np.asarray(PIL_ENHANCER[op](pil).enhance(float(factor)))


def inputs(w, h, seed):
    """name -> (h, w, 3) uint8: random bytes, 0 / 255 only (the clip branch for f > 1), a smooth ramp."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([(3 * xx + 5 * yy) % 256, (7 * xx + yy + 40) % 256, (xx + 2 * yy + 90) % 256], axis=2)
    return {
        "random": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
        "binary": (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8),
        "ramp": ramp.astype(np.uint8),
    }
