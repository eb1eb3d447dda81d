"""Random Erasing's noise in plain NumPy: Philox4x32-10,
a float64 Box-Muller of its words, and an erase applied to a float64 array.
The library's float32 normals must lie within BOUND of these."""
import numpy as np

CONST, COLOR, PIXEL = 0, 1, 2
BOUND = 2.0 ** -18  # |z - z64| <= BOUND * max(1, |z64|)

# (counter, key) -> words: the known answers of the Random123 distribution
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox(counter, key):
    """Philox4x32-10 of four broadcastable counter arrays and a two-word key -> four uint32 arrays."""
    c = [np.asarray(v, np.uint64) & 0xffffffff for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & 0xffffffff,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & 0xffffffff]
        k0, k1 = (k0 + 0x9E3779B9) & 0xffffffff, (k1 + 0xBB67AE85) & 0xffffffff
    return [v.astype(np.uint32) for v in c]


def normals(words):
    """The four float64 normals of four word arrays."""
    u = [((w >> 9).astype(np.float64) + 0.5) * 2.0 ** -23 for w in words]
    out = []
    for a, b in ((u[0], u[1]), (u[2], u[3])):
        r = np.sqrt(-2.0 * np.log(a))
        out += [r * np.cos(2 * np.pi * b), r * np.sin(2 * np.pi * b)]
    return out


def box_noise(mode, seed, b, box):
    """float64 fill of box b = (x0, y0, x1, y1) as (rows, columns, 3), for COLOR or PIXEL."""
    x0, y0, x1, y1 = box
    if mode == COLOR:
        z = normals(philox((0, 0, 0, 0x100 + b), seed))
        return np.broadcast_to(np.array([float(v) for v in z[:3]]), (y1 - y0, x1 - x0, 3))
    y, x, c = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), np.arange(3), indexing="ij")
    z = np.stack(normals(philox((x >> 2, y, c, b), seed)))
    return np.take_along_axis(z, (x & 3)[None], 0)[0]


def apply(img, erase):
    """erase = None or (mode, boxes, seed, value) on a float64 (h, w, 3) image: a new array."""
    out = np.array(img, np.float64)
    if erase is None:
        return out
    mode, boxes = erase[0], erase[1]
    for b, (x0, y0, x1, y1) in enumerate(boxes):  # in order: the highest-numbered box wins
        if mode == CONST:
            out[y0:y1, x0:x1] = np.broadcast_to(np.asarray(erase[3], np.float64), (3,))
        else:
            out[y0:y1, x0:x1] = box_noise(mode, erase[2], b, (x0, y0, x1, y1))
    return out
