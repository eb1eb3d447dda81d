"""The JPEG chunk layout of the host path (hostjpeg.cpp jpeg_chunk: entropy
jobs, planes and images, staged offsets) is pure host arithmetic, so it is
pinned without a device: tests/native/jpeg_layout.cpp lays out one chunk over
the committed fixtures and prints a fingerprint per table and every offset,
compared with tests/golden/jpeg_chunk_layout.json (recorded from the layout
code as it was before it was split into functions).  An offset that moves
here is an out-of-bounds device access there."""
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mlx-data_amd")
GOLD = np.load(os.path.join(HERE, "golden", "jpeg.npz"))
with open(os.path.join(HERE, "golden", "jpeg_chunk_layout.json")) as f:
    WANT = json.load(f)

SEQUENTIAL = ["sub0_prog0", "sub1_prog0", "sub2_prog0", "sub2_q30_opt", "sub2_q100", "grey", "rst_blocks1",
              "rgb_adobe0", "cmyk", "tiny_1x1", "tiny_3x2", "tall_40x3", "caltech_300x200", "truncated_rst"]
PROGRESSIVE = ["sub0_prog1", "grey_prog", "rst_rows1_prog"]
CASES = {
    # footprints are whole images
    "sequential": (SEQUENTIAL, {}, {}),
    # host-decoded and pending images share a chunk; one image needs only its centre 100x100
    "mixed": (SEQUENTIAL + PROGRESSIVE, {"caltech_300x200": "100,199,50,149"}, {}),
    # 32-bit subsequences: caltech_300x200 (~8,500 of them) is cut into several
    # jobs, rst_blocks1 has cuts moved to segment starts
    "bits32": (SEQUENTIAL, {}, {"MXD_TUNE_HUFF_BITS": "32"}),
}


@pytest.fixture(scope="module")
def program():
    b = subprocess.run(["make", "-s", "-C", PKG, "layout"], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    return os.path.join(PKG, "build", "native", "jpeg_layout")


def layout(program, tmp_path, names, foot, env):
    args = []
    for k in names:
        p = tmp_path / f"{k}.jpg"
        p.write_bytes(GOLD[f"{k}_jpg"].tobytes())
        args.append(f"{p}:{foot[k]}" if k in foot else str(p))
    r = subprocess.run([program] + args, capture_output=True, text=True, timeout=60, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        w = line.split()
        out[w[0]] = int(w[1]) if len(w) == 2 else [int(w[1]), w[2]]
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_jpeg_chunk_layout_is_unchanged(program, tmp_path, case):
    got = layout(program, tmp_path, *CASES[case])
    assert got == WANT[case], {k: (got.get(k), WANT[case].get(k)) for k in set(got) | set(WANT[case])
                               if got.get(k) != WANT[case].get(k)}
