"""Generates tests/golden/jpeg_sampling.npz: for every sampling layout of
tests/jpeg_layouts.py its 61x83 and 17x2 files (written by tests/jpeg_enc.py
with per-component factors; restart intervals and per-component tables vary
with the layout) and the pixels libjpeg-turbo decodes from them through
Pillow, as the project returns them (RGB; four components: the first three
channels of libjpeg's CMYK output), so the host decoder stays pinned to these
bytes whatever Pillow is installed later.  A coarse quantiser and little noise
keep the file small.

    python tests/golden/make_jpeg_sampling_golden.py
"""
import os
import sys

import numpy as np
from PIL import features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_layouts as L  # noqa: E402

Q = 24


def main():
    out = {"libjpeg_version": np.array(features.version("libjpeg_turbo") or "", dtype="U16")}
    for li, (name, sampling, adobe) in enumerate(L.LAYOUTS):
        for si, (w, h) in enumerate(L.GOLDEN_SIZES):
            px = L.image(name, w, h, seed=1, noise=4)
            data = L.write(px, sampling, adobe, restart=L.RESTARTS[(li + si) % 3], q=Q, distinct=(li + si) % 2 == 1)
            out[f"{name}_{w}x{h}_jpg"] = np.frombuffer(data, np.uint8)
            out[f"{name}_{w}x{h}_rgb"] = L.pillow_pixels(data)
    path = os.path.join(HERE, "jpeg_sampling.npz")
    np.savez_compressed(path, **out)
    print(len(out) // 2, "files,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
