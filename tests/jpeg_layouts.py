"""The sampling layouts the JPEG decoders are pinned on (test infrastructure;
tests/test_jpeg_sampling.py on the host, tests/test_gpu_jpeg_sampling.py on
the device): every integral layout family up to libjpeg's 10 blocks per
interleaved MCU that neither Pillow's encoder nor a 1x1 file reaches, written
by tests/jpeg_enc.py with per-component factors and tables.

A layout is (name, factors per component, Adobe transform or None).  Sizes are
the smallest at which the decoders change path: 1x1; 17x2 and 2x17 (a chroma
plane two samples wide or less turns h2v1 / h2v2 from fancy upsampling to
replication); 3x40; 61x83 (a multiple of no MCU); 100x129 (several MCU rows
and columns of every layout).  Restart intervals: none, every MCU, every 3."""
import functools
import io
import os
import zlib

import numpy as np

import jpeg_enc as J

_THREE = [
    ("440", [(1, 2), (1, 1), (1, 1)]),  # 4 blocks per MCU
    ("411", [(4, 1), (1, 1), (1, 1)]),  # 6
    ("410", [(4, 2), (1, 1), (1, 1)]),  # 10
    ("h3", [(3, 1), (1, 1), (1, 1)]),  # 5
    ("v3", [(1, 3), (1, 1), (1, 1)]),  # 5
    ("v4", [(1, 4), (1, 1), (1, 1)]),  # 6
    ("h2v4", [(2, 4), (1, 1), (1, 1)]),  # 10
    ("422x2", [(2, 2), (1, 2), (1, 2)]),  # 8: 4:2:2 with doubled luma rows
    ("mixed", [(2, 2), (2, 1), (1, 2)]),  # 8: Cb h1v2, Cr h2v1
    ("cbfull", [(2, 2), (2, 2), (1, 1)]),  # 9: Cb full, Cr quartered
    ("lumasub", [(1, 1), (2, 2), (2, 2)]),  # 9: luma subsampled
]
_FOUR = [
    ("22111122", [(2, 2), (1, 1), (1, 1), (2, 2)]),  # 10: what Photoshop writes
    ("11111122", [(1, 1), (1, 1), (1, 1), (2, 2)]),  # 7
    ("22111111", [(2, 2), (1, 1), (1, 1), (1, 1)]),  # 7
    ("21111121", [(2, 1), (1, 1), (1, 1), (2, 1)]),  # 6
    ("12111112", [(1, 2), (1, 1), (1, 1), (1, 2)]),  # 6
    ("32111111", [(3, 2), (1, 1), (1, 1), (1, 1)]),  # 9
    ("22211112", [(2, 2), (2, 1), (1, 1), (1, 2)]),  # 9
    ("22211212", [(2, 2), (2, 1), (1, 2), (1, 2)]),  # 10
]
_ONE = [("11", [(1, 1)]), ("22", [(2, 2)]), ("41", [(4, 1)]), ("13", [(1, 3)]), ("44", [(4, 4)])]

LAYOUTS = ([(f"c3_{n}_ycc", s, None) for n, s in _THREE] + [(f"c3_{n}_rgb", s, 0) for n, s in _THREE] +
           [(f"c4_{n}_cmyk", s, 0) for n, s in _FOUR] + [(f"c4_{n}_ycck", s, 2) for n, s in _FOUR] +
           [(f"c1_{n}", s, None) for n, s in _ONE])
SIZES = [(1, 1), (17, 2), (2, 17), (3, 40), (61, 83), (100, 129)]  # (width, height)
RESTARTS = [0, 1, 3]
GOLDEN_SIZES = [(61, 83), (17, 2)]


def blocks_per_mcu(sampling):
    return 1 if len(sampling) == 1 else sum(h * v for h, v in sampling)


def smooth(rng, h, w, c=3, noise=10):
    """A smooth random image with noise: every coefficient band in use."""
    gh, gw = h // 16 + 2, w // 16 + 2
    grid = rng.integers(0, 256, (gh, gw, c)).astype(np.float32)
    yi = np.minimum(np.arange(h) * (gh - 1) // max(1, h - 1), gh - 2)
    xi = np.minimum(np.arange(w) * (gw - 1) // max(1, w - 1), gw - 2)
    f = grid[yi][:, xi] * 0.6 + grid[yi + 1][:, xi + 1] * 0.4 + rng.normal(0, noise, (h, w, c))
    return np.clip(f, 0, 255).astype(np.uint8)


def write(pixels, sampling, adobe=None, restart=0, q=8, distinct=True):
    """The file of `pixels` (H, W, C) in this layout.  distinct: every
    component its own quantiser and DC / AC Huffman tables (four components:
    eight Huffman tables in the scan), a one-component file ids 3 / 2 / 1;
    else one of each."""
    nc = len(sampling)
    a = pixels[:, :, 0] if nc == 1 else pixels
    if not distinct:
        return J.encode(a, q=q, restart_mcus=restart, adobe=adobe, sampling=sampling)
    qs = [q, q + 1, np.arange(64) % 5 + q, q + 3]
    ids = [(3, 2, 1)] if nc == 1 else [(i, i, i) for i in range(nc)]
    return J.encode(a, q=qs, dc=J.DC_TABLES, ac=J.AC_TABLES, restart_mcus=restart, adobe=adobe, sampling=sampling,
                    tables=ids)


def image(name, w, h, seed=0, noise=10):
    """The layout's picture at this size: seeded by the name, the size and `seed`."""
    nc = int(name[1])
    return smooth(np.random.default_rng([zlib.crc32(name.encode()), w, h, seed]), h, w, nc, noise)


class Case:
    def __init__(self, name, sampling, adobe, w, h, restart, distinct, data):
        self.name, self.sampling, self.adobe, self.w, self.h = name, sampling, adobe, w, h
        self.restart, self.distinct, self.data = restart, distinct, data
        self.ncomp = len(sampling)
        self.id = f"{name}_{w}x{h}_r{restart}"


@functools.lru_cache(maxsize=None)
def cases():
    """Every layout x size x restart interval, one file each; tables are
    distinct per component in every other (layout, size) pair."""
    out = []
    for li, (name, sampling, adobe) in enumerate(LAYOUTS):
        for si, (w, h) in enumerate(SIZES):
            px = image(name, w, h)
            for r in RESTARTS:
                d = (li + si) % 2 == 0
                out.append(Case(name, sampling, adobe, w, h, r, d, write(px, sampling, adobe, r, distinct=d)))
    return out


TOO_LARGE = "Sampling factors too large for interleaved scan"  # jdinput.c per_scan_setup (JERR_BAD_MCU_SIZE)
FRACTIONAL = "Fractional sampling not implemented yet"  # jdsample.c jinit_upsampler (JERR_FRACT_SAMPLE_NOTIMPL)
# Files libjpeg refuses: (name, factors, Adobe transform, its message).
REFUSED = [
    ("12_blocks", [(2, 2), (2, 2), (2, 2)], None, TOO_LARGE),
    ("11_blocks", [(3, 3), (1, 1), (1, 1)], None, TOO_LARGE),
    ("11_blocks_cmyk", [(2, 2), (2, 2), (1, 1), (2, 1)], 0, TOO_LARGE),
    ("12_blocks_and_fractional", [(3, 3), (2, 1), (1, 1)], None, TOO_LARGE),  # the scan's check comes first
    ("fractional_cb", [(3, 1), (2, 1), (1, 1)], None, FRACTIONAL),
    ("fractional_rows", [(2, 3), (1, 2), (1, 1)], 0, FRACTIONAL),
    ("fractional_k_only_cmyk", [(3, 1), (3, 1), (1, 1), (2, 1)], 0, FRACTIONAL),
    ("fractional_k_only_ycck", [(3, 1), (3, 1), (1, 1), (2, 1)], 2, FRACTIONAL),
]


def refused_files():
    return [(name, msg, write(image("c%d_%s" % (len(s), name), 37, 29), s, adobe, restart=r, distinct=bool(r)))
            for r, (name, s, adobe, msg) in zip([0, 3] * 4, REFUSED)]


def golden():
    """tests/golden/jpeg_sampling.npz: (key, file bytes, libjpeg-turbo's pixels) per file."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_sampling.npz"))
    return [(k[:-4], g[k].tobytes(), g[k[:-4] + "_rgb"]) for k in g.files if k.endswith("_jpg")]


def pillow_pixels(data):
    """libjpeg-turbo's decode through Pillow as the (H, W, 3) the project
    returns: RGB; of a four-component file the first three channels of
    libjpeg's CMYK output (Pillow inverts Adobe files' CMYK: 255 - it)."""
    from PIL import Image

    im = Image.open(io.BytesIO(data))
    if im.mode == "CMYK":
        return 255 - np.asarray(im)[:, :, :3]
    return np.asarray(im.convert("RGB"))
