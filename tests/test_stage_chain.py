"""The stage chain behind the resize (batch_layout.cpp): the upload and the
launches of every combination of format, colours, tones, warps and enhances
are the recorded ones, byte for byte.  CPU only: build_layout is device-free.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mlx-data_amd")
HIPCC = "/opt/rocm/bin/hipcc"
GOLDEN = os.path.join(HERE, "golden", "stage_chain_layouts.txt")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_stage_chain_layouts(tmp_path):
    """tests/cpp/stage_chain_unit.cpp: the 32 null / non-null combinations of
    {fmt, colors, tones, warps, enhances} over a seven-image batch of mixed
    routes, under MXD_POLICY_AUTO and MXD_POLICY_PREFER_BAND.  Every line
    (digest of the uploaded bytes before and after add_scratch, scratch
    offsets, launch parameters) equals the golden's, which was recorded
    before the chain replaced the per-stage special cases."""
    exe = str(tmp_path / "stage_chain_unit")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-I", os.path.join(os.path.dirname(HERE), "include"), "-I",
                    os.path.join(PKG, "csrc"), os.path.join(HERE, "cpp", "stage_chain_unit.cpp"), "-L", PKG,
                    "-lmxd_amd", "-Wl,-rpath," + PKG, "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.splitlines()
    want = open(GOLDEN).read().splitlines()
    assert len(want) == 64 and len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"layout {k}"
