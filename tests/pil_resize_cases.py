"""What tests/test_pil_resize.py and tests/test_gpu_pil_resize.py share: the
geometries, an input maker and the reference, which is Pillow itself."""
import numpy as np
from PIL import Image

FILTERS = {"pil_bilinear": Image.BILINEAR, "pil_bicubic": Image.BICUBIC, "pil_lanczos": Image.LANCZOS}

# (src h, src w, resize w, resize h, crop (x, y, w, h) or None, flip, filters or None for all three)
GEOMS = [
    (70, 90, 24, 19, None, 0, None),      # both axes down, ratio ~3.7
    (16, 20, 45, 33, None, 0, None),      # upscale: 0 or 1 new source rows per output row
    (48, 64, 64, 24, None, 0, None),      # identity x axis
    (48, 64, 31, 48, None, 0, None),      # identity y axis
    (1, 5, 3, 7, None, 0, None),          # degenerate
    (5, 1, 4, 2, None, 0, None),
    (320, 24, 12, 20, None, 0, ("pil_lanczos",)),   # 16 : 1 down the rows: 97 vertical taps, the ring wraps
    (24, 320, 20, 12, None, 0, ("pil_lanczos",)),   # 16 : 1 along the rows: 97 horizontal taps
    (105, 207, 69, 35, None, 0, None),    # (kPilTX + 5) x (kPilTY + 3) = (64 + 5) x (32 + 3): two ragged tiles per axis
    (150, 200, 80, 60, (13, 7, 41, 29), 0, None),   # interior window, odd offsets, unaligned dst rows
    (150, 200, 80, 60, (13, 7, 41, 29), 1, None),
]
CASES = [(g, f) for g in GEOMS for f in (g[6] or FILTERS)]
IDS = ["%dx%d-%dx%d%s%s-%s" % (g[0], g[1], g[2], g[3], "-crop" if g[4] else "", "-flip" if g[5] else "", f)
       for g, f in CASES]


def image(h, w, c, seed=0):
    """Random bytes with saturated structure over them: the bicubic and Lanczos
    lobes then overshoot, so the clamp between the two passes shows."""
    a = np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)
    a[::3, ::2] = 255
    a[1::3, 1::2] = 0
    return a


def pillow(a, geom, filter):
    """Image.resize, then the crop window and the flip in NumPy; (h, w, c)."""
    _, _, rw, rh, crop, flip, _ = geom
    out = np.asarray(Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).resize((rw, rh), FILTERS[filter]))
    out = out.reshape(rh, rw, a.shape[2])
    x, y, w, h = crop or (0, 0, rw, rh)
    out = out[y:y + h, x:x + w]
    return np.ascontiguousarray(out[:, ::-1] if flip else out)
