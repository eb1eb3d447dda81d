"""The reference of the mix stage: timm's FastCollateMixup on uint8 images, as
NumPy expressions.  MixUp is

    mixed = a.astype(np.float32) * lam + b.astype(np.float32) * (1 - lam); np.rint(mixed, out=mixed)

with a Python-float lam (NumPy multiplies a float32 array by a Python float in
float32, the scalar rounded to float32 first: lam, and 1 - lam computed in
double), and CutMix is mixed[yl:yh, xl:xh] = b[yl:yh, xl:xh].  Entries are the
tuples mlx_data_amd.capi.make_mixes takes."""
import numpy as np

NONE, MIXUP, CUTMIX = 0, 1, 2


def mixup(a, b, lam):
    """timm's expression on two (h, w, 3) uint8 images."""
    lam = float(lam)
    mixed = a.astype(np.float32) * lam + b.astype(np.float32) * (1 - lam)
    np.rint(mixed, out=mixed)
    return mixed.astype(np.uint8)


def cutmix(a, b, x0, y0, x1, y1):
    mixed = a.copy()
    mixed[y0:y1, x0:x1] = b[y0:y1, x0:x1]
    return mixed


def entry_mixup(partner, lam):
    return (MIXUP, int(partner), float(lam), 1.0 - float(lam))


def entry_cutmix(partner, x0, y0, x1, y1):
    return (CUTMIX, int(partner), int(x0), int(y0), int(x1), int(y1))


def apply(images, i, entry, lam=None):
    """What image i of the unmixed batch `images` becomes under `entry`.  A
    MixUp entry made by entry_mixup(partner, lam) is evaluated from lam itself
    when it is given, else from the entry's weights as float32 scalars."""
    if entry[0] == NONE:
        return images[i].copy()
    a, b = images[i], images[entry[1]]
    if entry[0] == CUTMIX:
        return cutmix(a, b, *entry[2:6])
    if lam is not None:
        return mixup(a, b, lam)
    mixed = a.astype(np.float32) * np.float32(entry[2]) + b.astype(np.float32) * np.float32(entry[3])
    np.rint(mixed, out=mixed)
    # (the header's min: reached only by weights that do not sum to one, which no lam gives)
    return np.minimum(mixed, 255).astype(np.uint8)


def byte_pair_grid():
    """Two 256 x 256 x 3 images holding every (own, partner) byte pair: own = the row, partner = the column."""
    q, r = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return (np.ascontiguousarray(np.repeat(q[:, :, None], 3, 2)), np.ascontiguousarray(np.repeat(r[:, :, None], 3, 2)))
