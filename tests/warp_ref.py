"""What the warp tests share: Pillow as the reference of a warp (mode, fill,
matrix) on an (h, w, 3) uint8 image, Pillow's rotate matrix restated, and the
matrix families the sweeps use."""
import math

import numpy as np
from PIL import Image

NONE, NEAREST, BILINEAR = 0, 1, 2
RESAMPLE = {NEAREST: Image.NEAREST, BILINEAR: Image.BILINEAR}
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def fill3(fill):
    return (int(fill),) * 3 if np.isscalar(fill) else tuple(int(v) for v in fill)


def pillow_apply(img, warp):
    """Image.transform(size, AFFINE, matrix, resample, fillcolor=fill) of an (h, w, 3) uint8 array."""
    mode, fill, m = warp
    if mode == NONE:
        return img.copy()
    h, w = img.shape[:2]
    pil = Image.fromarray(np.ascontiguousarray(img))
    return np.asarray(pil.transform((w, h), Image.AFFINE, tuple(float(v) for v in m), RESAMPLE[mode],
                                    fillcolor=fill3(fill)))


def pillow_rotate(img, angle, mode, fill):
    return np.asarray(Image.fromarray(np.ascontiguousarray(img)).rotate(angle, RESAMPLE[mode], fillcolor=fill3(fill)))


def rotate_matrix(w, h, angle):
    """Image.rotate's matrix for expand=False and the centre (w / 2, h / 2), operation for operation."""
    r = -math.radians(angle % 360.0)
    c, s = round(math.cos(r), 15), round(math.sin(r), 15)
    cx, cy = w / 2.0, h / 2.0
    return (c, s, c * (-cx) + s * (-cy) + 0.0 + cx, -s, c, (-s) * (-cx) + c * (-cy) + 0.0 + cy)


def shear(x=0.0, y=0.0):
    return (1.0, float(x), 0.0, float(y), 1.0, 0.0)


def translate(x=0.0, y=0.0):
    return (1.0, 0.0, float(x), 0.0, 1.0, float(y))


def families(w, h, rng):
    """name -> matrix: the six families of the sweeps for a w x h image."""
    return {
        "shear-x": shear(0.3, 0.0), "shear-xy": shear(-0.2, 0.15),
        "translate-fraction": translate(2.5, -1.25), "translate-integer": translate(-3.0, 2.0),
        "rotate-30": rotate_matrix(w, h, 30.0), "rotate-random": rotate_matrix(w, h, float(rng.uniform(-180, 180))),
        "random": tuple(float(v) for v in rng.normal(0, 1, 6) * np.array([1, 1, w, 1, 1, h])),
        "scale": (0.7, 0.0, 1.3, 0.0, 1.4, -0.6),
    }


OUTSIDE = translate(1000.0, 0.0)  # every pixel maps outside: the result is all fill
