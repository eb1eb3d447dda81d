"""bench.py on the GPU: a plain run measures the headline alone, and
`--dump-outputs` writes the batch its last timed step computed.  The batch is
rebuilt here from the benchmark's own seed and checked like every other C2
batch (tests/test_gpu_parity.py): f32 bit-exact q/255 of a uint8 result that is
within +-1 of the oracle, and bit-exact to the same call made directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import center_geom, compare, oracle_out, run_device

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LUT = np.load(os.path.join(HERE, "golden", "golden.npz"))["lut"]
MAX_FRAC = 2e-3  # fraction of channels allowed to differ by exactly 1 (tests/test_gpu_parity.py)
BATCH, STEPS, WARMUP = 5, 3, 1


def test_plain_run_headline_and_dump(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--batch", str(BATCH), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "u8->f32"
    assert line["ms_per_step"] > 0
    # value = images / wall of the timed steps (both rounded in the line)
    assert abs(line["value"] - BATCH * 1e3 / line["ms_per_step"]) / line["value"] < 0.02
    # a plain run takes no measurement but the headline
    for k in ("roofline", "cpu_baseline", "e2e", "e2e_jpeg", "workloads"):
        assert line[k] is None, k

    assert os.listdir(tmp_path) == ["output.npy"]
    out = np.load(tmp_path / "output.npy")
    assert out.dtype == np.float32 and out.shape == (BATCH, 224, 224, 3)
    # the benchmark's C2 inputs: seed 1000 + rank, images packed back to back
    per = 1280 * 960 * 3
    host = np.random.default_rng(1000).integers(0, 256, BATCH * per, dtype=np.uint8)
    imgs = [host[i * per:(i + 1) * per].reshape(960, 1280, 3) for i in range(BATCH)]
    geoms = [center_geom(im) for im in imgs]
    direct = run_device(imgs, geoms, f32=True)
    for i in range(BATCH):
        assert np.array_equal(out[i].view(np.uint32), direct[i].view(np.uint32))
        q = np.rint(out[i] * 255).astype(np.uint8)
        assert np.array_equal(out[i].view(np.uint32), LUT[q].view(np.uint32))
    for i in (0, BATCH - 1):
        m, f = compare(np.rint(out[i] * 255).astype(np.uint8), oracle_out(imgs[i], geoms[i]))
        assert m <= 1 and f <= MAX_FRAC, (i, m, f)
