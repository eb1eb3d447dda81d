"""GPU: batch_mix on the operator surface.  The expectation is timm's NumPy
expression (tests/mix_ref.py) on the uint8 batch of the same chain without
batch_mix, with the entries _batch_mix_draws gives under the same seed, then
the NumPy statement of the output format; compared as integer bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mix_ref as M
from gpu_util import synth
from mlx_data_amd import _pipeline
from mlx_data_amd import data as dx
from out_format_util import IMAGENET_MEAN, IMAGENET_STD
from test_gpu_tone_surface import bits, chain, formatted, samples

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 29, 33  # chain()'s crop


@pytest.fixture(autouse=True)
def one_device():
    before = dx.devices()
    dx.set_devices([0])
    yield
    dx.set_devices(before)


def draws(seed, sizes, h=H, w=W, **kw):
    """The entries of consecutive batches of the given sizes under one seed."""
    dx.set_state(seed)
    return [_pipeline._batch_mix_draws(n, h, w, **kw) for n in sizes]


def mixed(u8, entries):
    """timm's expression on the unmixed uint8 batch, entry by entry."""
    out = []
    for i, e in enumerate(entries):
        entry = (e[0],) if e[0] == M.NONE else (e[0], e[1], e[2], e[3]) if e[0] == M.MIXUP else (e[0], e[1]) + tuple(e[4:8])
        out.append(M.apply(u8, i, entry))
    return np.stack(out)


def check_keys(s, entries):
    assert s["mix_lam"].dtype == np.float32 and s["mix_partner"].dtype == np.int64
    assert np.array_equal(s["mix_lam"], np.float32([e[8] for e in entries]))
    assert np.array_equal(s["mix_partner"], np.int64([e[1] for e in entries]))


@pytest.mark.parametrize("kw", [dict(mixup_alpha=1.0), dict(cutmix_alpha=1.0, mode="pair"),
                                dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", prob=0.7)],
                         ids=["mixup batch", "cutmix pair", "both elem"])
def test_host_and_device_batches_agree_with_numpy(kw):
    b = chain(dx.buffer_from_vector(samples(6, 3)))
    u8 = b.batch(6)[0]["image"]
    (entries,) = draws(21, [6], **kw)
    want = mixed(u8, entries)
    assert not np.array_equal(want, u8)
    dx.set_state(21)
    s = b.batch_mix(6, "image", **kw)[0]
    assert s["image"].dtype == np.uint8 and np.array_equal(s["image"], want)
    check_keys(s, entries)
    assert np.array_equal(s["label"], np.arange(6))  # the other keys batch as in batch
    dx.set_state(21)
    d = b.batch_mix(6, "image", device=0, **kw)[0]
    assert np.array_equal(d["image"].numpy(), want)
    check_keys(d, entries)
    # image_to_float and image_normalize compose: the mix is on the bytes beneath them
    dx.set_state(21)
    f = b.image_to_float("image").batch_mix(6, "image", **kw)[0]["image"]
    assert np.array_equal(bits(f), formatted(want, "float32"))
    n = b.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="float16", layout="chw")
    ref = formatted(want, "float16", IMAGENET_MEAN, IMAGENET_STD, "chw")
    dx.set_state(21)
    assert np.array_equal(bits(n.batch_mix(6, "image", **kw)[0]["image"]), ref)
    dx.set_state(21)
    assert np.array_equal(bits(n.batch_mix(6, "image", device=0, **kw)[0]["image"].numpy()), ref)
    # a stream gives the same batch
    dx.set_state(21)
    st = b.to_stream().batch_mix(6, "image", **kw).next()
    assert np.array_equal(st["image"], want)


def test_an_odd_short_last_batch_and_custom_keys():
    """7 samples in batches of 4: the last holds 3, its middle image is its own partner."""
    b = chain(dx.buffer_from_vector(samples(7, 5)))
    u8 = [b.batch(4)[k]["image"] for k in range(2)]
    kw = dict(mixup_alpha=1.0, cutmix_alpha=1.0, mode="pair")
    first, last = draws(9, [4, 3], **kw)
    assert [e[1] for e in last] == [2, 1, 0]
    dx.set_state(9)
    bm = b.batch_mix(4, "image", lam_key="lam", partner_key="other", **kw)
    s0, s1 = bm[0], bm[1]
    assert np.array_equal(s0["image"], mixed(u8[0], first)) and np.array_equal(s1["image"], mixed(u8[1], last))
    assert s1["image"].shape == (3, H, W, 3)
    assert np.array_equal(s1["other"], [2, 1, 0]) and np.array_equal(s1["lam"], np.float32([e[8] for e in last]))
    if last[1][0] == M.MIXUP:  # its own partner: the arithmetic as written
        assert np.array_equal(s1["image"][1], M.apply(u8[1], 1, (M.MIXUP, 1, last[1][2], last[1][3])))


def test_a_batch_with_jpeg_and_raw_sources(tmp_path):
    """JPEG files are decoded by the batch launch, PNG files are raw arrays:
    the two shares run unmixed into a device block, then one mix call."""
    from PIL import Image

    files = []
    for i in range(6):
        p = tmp_path / (f"img{i}.jpg" if i % 2 else f"img{i}.png")
        Image.fromarray(synth(80, 120, 3, 400 + i)).save(p, **(dict(quality=92) if i % 2 else {}))
        files.append(dict(image=str(p).encode()))
    b = chain(dx.buffer_from_vector(files).load_image("image"))
    u8 = b.batch(6)[0]["image"]
    kw = dict(mixup_alpha=1.0, mode="elem")
    (entries,) = draws(33, [6], **kw)
    want = mixed(u8, entries)
    _pipeline._run_on_stats(True)
    dx.set_state(33)
    got = b.batch_mix(6, "image", **kw)[0]["image"]
    calls, jpegs = _pipeline._run_on_stats(True)
    assert (calls, jpegs) == (1, 3)
    assert np.array_equal(got, want)
    n = b.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="float16", layout="chw")
    dx.set_state(33)
    assert np.array_equal(bits(n.batch_mix(6, "image", device=0, **kw)[0]["image"].numpy()),
                          formatted(want, "float16", IMAGENET_MEAN, IMAGENET_STD, "chw"))


def test_a_mixed_batch_is_never_split_over_devices():
    """set_devices([0, 0]): batch would cut 128 images into two slices of 64; batch_mix makes one call."""
    b = chain(dx.buffer_from_vector(samples(128, 40)))
    dx.set_devices([0, 0])
    _pipeline._run_on_stats(True)
    u8 = b.batch(128)[0]["image"]
    assert _pipeline._run_on_stats(True)[0] == 2
    kw = dict(cutmix_alpha=1.0, mode="elem")
    (entries,) = draws(5, [128], **kw)
    dx.set_state(5)
    got = b.batch_mix(128, "image", **kw)[0]["image"]
    assert _pipeline._run_on_stats(True)[0] == 1
    assert np.array_equal(got, mixed(u8, entries))


CONSUMER = r"""
import json, sys
import numpy as np
import torch                      # torch first: its HIP runtime is the one libmxd_amd.so binds
torch.zeros(1, device="cuda")
sys.path[:0] = [{repo!r}, {repo!r} + "/tests", {repo!r} + "/oracle", {repo!r} + "/mlx-data_amd"]
from mlx_data_amd import data as dx
from test_gpu_mix_surface import draws, mixed
from test_gpu_tone_surface import chain, formatted, samples
from out_format_util import IMAGENET_MEAN, IMAGENET_STD
b = chain(dx.buffer_from_vector(samples(8, 11)))
u8 = b.batch(8)[0]["image"]
kw = dict(mixup_alpha=1.0, cutmix_alpha=1.0, mode="pair")
(entries,) = draws(17, [8], **kw)
dx.set_state(17)
s = (b.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="bfloat16", layout="chw")
     .batch_mix(8, "image", device=0, **kw)[0])
dev = s["image"]
x = torch.from_dlpack(dev)
got = x.cpu().view(torch.int16).numpy().view(np.uint16)
m = mixed(u8, entries)
want = formatted(m, "bfloat16", IMAGENET_MEAN, IMAGENET_STD, "chw")
print(json.dumps(dict(cuda=bool(x.is_cuda), dtype=str(x.dtype), shape=list(x.shape), ptr=x.data_ptr() == dev.data_ptr,
                      same=bool(np.array_equal(got, want)), moved=bool(not np.array_equal(m, u8)),
                      lam=bool(np.array_equal(s["mix_lam"], np.float32([e[8] for e in entries]))))))
"""


@pytest.mark.timeout(300)
def test_normalised_bfloat16_chw_device_batch_through_dlpack():
    r = subprocess.run([sys.executable, "-c", CONSUMER.format(repo=REPO)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == dict(cuda=True, dtype="torch.bfloat16", shape=[8, 3, H, W], ptr=True, same=True, moved=True, lam=True), res


def test_each_runtime_error_names_what_is_wrong():
    kw = dict(mixup_alpha=1.0)
    raw = dx.buffer_from_vector(samples(4, 1))
    cases = [
        (chain(raw).batch_mix(4, "image", dim={"image": 0}, **kw), "batch_mix: key <image>: no dim for the mixed key"),
        (raw.batch_mix(4, "image", **kw), "batch_mix: key <image>: sample 0 is a materialised array, not a pending image"),
        (raw.image_resize_smallest_side("image", 44).batch_mix(4, "image", **kw), "(a ragged batch)"),
        (chain(dx.buffer_from_vector([dict(image=synth(60, 80, c, k)) for k, c in enumerate((3, 3, 1, 3))]))
         .batch_mix(4, "image", **kw), "batch_mix: key <image>: sample 2 has 1 channels, not 3"),
        (dx.buffer_from_vector([dict(image=np.zeros((2, 40, 50, 3), np.uint8))] * 2).image_resize("image", 20, 10)
         .batch_mix(2, "image", **kw), "is a video"),
        (chain(raw).batch_mix(4, "pixels", **kw), "batch_mix: key <pixels> is not in the samples"),
    ]
    for b, word in cases:
        with pytest.raises(RuntimeError) as err:
            b[0]
        assert word in str(err.value), str(err.value)
