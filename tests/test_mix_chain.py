"""The stage chain of a mix call (batch_layout.cpp): the mix stage is the last
of up to four, the rows alternate, and every entry's partner address is the
partner's own row address.  CPU only: build_layout is device-free.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mlx-data_amd")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mix_layouts(tmp_path):
    """tests/cpp/mix_layout_unit.cpp: the 32 null / non-null combinations of
    {fmt, colors, tones, warps, enhances} with mixes over a seven-image batch
    of mixed routes (two pairs, a chain, two self partners, a NONE), under
    MXD_POLICY_AUTO and MXD_POLICY_PREFER_BAND.  The program checks the
    invariants itself; here: it ran all 64 layouts, and the chains have 1 to
    4 stages with the mix stage reading rows A and rows B equally often."""
    exe = str(tmp_path / "mix_layout_unit")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-I", os.path.join(os.path.dirname(HERE), "include"), "-I",
                    os.path.join(PKG, "csrc"), os.path.join(HERE, "cpp", "mix_layout_unit.cpp"), "-L", PKG,
                    "-lmxd_amd", "-Wl,-rpath," + PKG, "-o", exe], check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and len(lines) == 65
    fields = [dict(f.split("=") for f in line.split()) for line in lines[:-1]]
    assert sorted({int(f["stages"]) for f in fields}) == [1, 2, 3, 4]
    for f in fields:
        stages = int(f["stages"])
        assert f["reads"] == ("A" if stages % 2 else "B")
        assert (int(f["b_at"]) > 0) == (stages >= 2)
        # 7 images of 33, 224, 40, 224, 221, 40 and 16 rows, 8 rows a workgroup
        assert int(f["blocks"]) == 5 + 28 + 5 + 28 + 28 + 5 + 2
    assert sum(f["reads"] == "A" for f in fields) == sum(f["reads"] == "B" for f in fields)
