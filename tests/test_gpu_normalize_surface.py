"""GPU: image_normalize on the Buffer / Stream surface (mlx_data_amd/data.py).

The op marks the pending image with an output format; ``batch(n, device=d)``
then writes the normalised float32 / float16 / bfloat16 batch, (B, H, W, C) or
(B, C, H, W), from the resize launch itself (mxd_*_to_device_fmt), and a host
batch is the same device result copied back once.  Expected values never come
from the code under test: they are the NumPy / torch expression of
include/mxd_amd.h applied to the uint8 batch of the same chain
(out_format_util.expected_table), compared as integer bits."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_util import synth
from mlx_data_amd import data as dx
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expected_table

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def one_device():
    before = dx.devices()
    yield
    dx.set_devices(before)


def samples(n, seed=0, channels=3):
    shapes = [(375, 500), (960, 1280), (200, 300), (500, 375)]
    return [dict(image=synth(*shapes[i % 4], channels, seed + i), label=i) for i in range(n)]


def chain(b):
    return b.image_resize_smallest_side("image", 256).image_center_crop("image", 224, 224)


def want_bits(u8, elem, mean=None, std=None, layout="hwc"):
    """Integer bits of the normalised form of a (..., H, W, C) uint8 array."""
    c = u8.shape[-1]
    table = expected_table(elem, c, mean, std)
    out = np.stack([table[k][u8[..., k]] for k in range(c)], axis=-1)
    return np.moveaxis(out, -1, -3) if layout == "chw" else out


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


BF16_CONSUMER = r"""
import json, sys
import numpy as np
import torch                      # torch first: its HIP runtime is the one libmxd_amd.so binds
torch.zeros(1, device="cuda")
sys.path[:0] = [{repo!r}, {repo!r} + "/tests", {repo!r} + "/oracle", {repo!r} + "/mlx-data_amd"]
from mlx_data_amd import data as dx
from gpu_util import synth
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expected_table
shapes = [(375, 500), (960, 1280), (200, 300), (500, 375)]
imgs = [dict(image=synth(*shapes[i % 4], 3, 11 + i)) for i in range(8)]
b = dx.buffer_from_vector(imgs).image_resize_smallest_side("image", 256).image_center_crop("image", 224, 224)
u8 = b.batch(8)[0]["image"]
dev = (b.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="bfloat16", layout="chw")
       .batch(8, device=0)[0]["image"])
t = torch.from_dlpack(dev)
table = expected_table("bfloat16", 3, IMAGENET_MEAN, IMAGENET_STD)
want = np.stack([table[k][u8[..., k]] for k in range(3)], axis=1)       # (B, C, H, W) bits
got = t.cpu().view(torch.int16).numpy().view(np.uint16)
# the torch statement of the same thing, on the CPU
x = torch.from_numpy(u8.astype("float32") / np.float32(255))
ref = (x - torch.tensor(IMAGENET_MEAN)) / torch.tensor(IMAGENET_STD)
ref = ref.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)
s = float(t.float().sum().item())   # a torch kernel reading the batch in place
print(json.dumps(dict(cuda=bool(t.is_cuda), dtype=str(t.dtype), shape=list(t.shape), ptr=t.data_ptr() == dev.data_ptr,
                      repr_dtype=str(dev.dtype), same=bool(np.array_equal(got, want)),
                      torch_same=bool(np.array_equal(got, ref)), finite=bool(np.isfinite(s)))))
"""


@pytest.mark.timeout(300)
def test_bfloat16_chw_device_batch_through_dlpack():
    """batch(8, device=0) of a bfloat16 CHW chain: torch.from_dlpack gives a
    zero-copy torch.bfloat16 (8, 3, 224, 224) tensor whose bits are the
    expression's applied to the uint8 batch of the same chain (a process that
    imported torch first, the one-HIP-runtime configuration)."""
    r = subprocess.run([sys.executable, "-c", BF16_CONSUMER.format(repo=REPO)], capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == dict(cuda=True, dtype="torch.bfloat16", shape=[8, 3, 224, 224], ptr=True, repr_dtype="bfloat16",
                       same=True, torch_same=True, finite=True), res


def test_float16_hwc_host_batch_equals_the_numpy_expression():
    b = chain(dx.buffer_from_vector(samples(6)))
    u8 = b.batch(6)[0]["image"]
    got = b.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="float16").batch(6)[0]["image"]
    assert isinstance(got, np.ndarray) and got.dtype == np.float16 and got.shape == (6, 224, 224, 3)
    mean, std = np.float32(IMAGENET_MEAN), np.float32(IMAGENET_STD)
    want = (((u8.astype("float32") / np.float32(255)) - mean) / std).astype("float16")
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got), want_bits(u8, "float16", IMAGENET_MEAN, IMAGENET_STD))


@pytest.mark.parametrize("dtype,layout,mean,std", [
    ("float32", "chw", 0.5, 0.25),
    ("float32", "hwc", None, None),
    ("float16", "chw", IMAGENET_MEAN, None),
])
def test_host_and_device_batches_and_direct_reads_agree(dtype, layout, mean, std):
    b = chain(dx.buffer_from_vector(samples(5, seed=3)))
    u8 = b.batch(5)[0]["image"]
    n = b.image_normalize("image", mean=mean, std=std, dtype=dtype, layout=layout)
    want = want_bits(u8, dtype, mean, std, layout)
    host = n.batch(5)[0]["image"]
    assert host.dtype == np.dtype(dtype) and host.shape == ((5, 3, 224, 224) if layout == "chw" else (5, 224, 224, 3))
    assert np.array_equal(bits(host), want)
    dev = n.batch(5, device=0)[0]["image"]
    assert isinstance(dev, dx.DeviceArray) and dev.dtype == np.dtype(dtype) and dev.shape == host.shape
    assert dev.nbytes == host.nbytes
    assert np.array_equal(bits(dev.numpy()), want)
    one = n[1]["image"]  # an unbatched normalised image read directly: a launch of its own
    assert one.dtype == np.dtype(dtype) and np.array_equal(bits(one), want[1])


def test_output_key_and_if_forms():
    b = chain(dx.buffer_from_vector(samples(3, seed=7)))
    u8 = b.batch(3)[0]["image"]
    x = b.image_normalize("image", mean=0.5, std=0.5, dtype="float16", layout="chw", output_key="x").batch(3)[0]
    assert np.array_equal(x["image"], u8)  # the input key keeps its uint8 batch
    assert np.array_equal(bits(x["x"]), want_bits(u8, "float16", 0.5, 0.5, "chw"))
    assert np.array_equal(b.image_normalize_if(False, "image", mean=0.5).batch(3)[0]["image"], u8)
    on = b.image_normalize_if(True, "image", mean=0.5, std=0.5).batch(3)[0]["image"]
    assert np.array_equal(bits(on), want_bits(u8, "float32", 0.5, 0.5))
    s = (chain(dx.buffer_from_vector(samples(3, seed=7)).to_stream())
         .image_normalize_if(True, "image", None, None, "float16", "hwc").batch(3))
    assert np.array_equal(bits(next(iter(s))["image"]), want_bits(u8, "float16"))


class _DLDataType(ctypes.Structure):
    _fields_ = [("code", ctypes.c_uint8), ("bits", ctypes.c_uint8), ("lanes", ctypes.c_uint16)]


class _DLTensor(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("device_type", ctypes.c_int32), ("device_id", ctypes.c_int32),
                ("ndim", ctypes.c_int32), ("dtype", _DLDataType), ("shape", ctypes.POINTER(ctypes.c_int64)),
                ("strides", ctypes.POINTER(ctypes.c_int64)), ("byte_offset", ctypes.c_uint64)]


def _dl(img):
    cap = img.__dlpack__()
    get = ctypes.pythonapi.PyCapsule_GetPointer
    get.restype = ctypes.c_void_p
    get.argtypes = [ctypes.py_object, ctypes.c_char_p]
    t = _DLTensor.from_address(get(cap, b"dltensor"))
    out = (t.dtype.code, t.dtype.bits, t.dtype.lanes), [t.shape[i] for i in range(t.ndim)], t.data
    del cap  # unconsumed: the capsule frees its tensor
    return out


def test_bfloat16_has_no_host_form_and_dlpack_names_the_16_bit_types():
    b = chain(dx.buffer_from_vector(samples(2)))
    bf = b.image_normalize("image", mean=0.5, std=0.5, dtype="bfloat16", layout="chw")
    with pytest.raises(RuntimeError, match=r"device=.*DLPack"):
        bf.batch(2)[0]
    with pytest.raises(RuntimeError, match=r"device=.*DLPack"):
        bf[0]
    dev = bf.batch(2, device=0)[0]["image"]
    assert dev.dtype == "bfloat16" and dev.shape == (2, 3, 224, 224) and dev.nbytes == 2 * 3 * 224 * 224 * 2
    with pytest.raises(RuntimeError, match=r"device=.*DLPack"):
        dev.numpy()
    assert _dl(dev) == ((4, 16, 1), [2, 3, 224, 224], dev.data_ptr)  # kDLBfloat
    half = b.image_normalize("image", dtype="float16").batch(2, device=0)[0]["image"]
    assert _dl(half) == ((2, 16, 1), [2, 224, 224, 3], half.data_ptr)  # kDLFloat


def test_unequal_formats_and_channel_counts_in_one_batch_raise():
    from mlx_data_amd import _pipeline

    def norm(seed, channels=3, **kw):
        return chain(dx.buffer_from_vector(samples(1, seed, channels))).image_normalize("image", **kw)

    a = norm(0, mean=0.5, std=0.25, dtype="float16", layout="chw")
    for device in (None, 0):
        with pytest.raises(RuntimeError, match="different output formats"):
            _pipeline._merge([a, norm(1, mean=0.5, std=0.2, dtype="float16", layout="chw")], 0, device)
        with pytest.raises(RuntimeError, match="different channel counts"):
            _pipeline._merge([a, norm(1, 1, mean=0.5, std=0.25, dtype="float16", layout="chw")], 0, device)
        ok = _pipeline._merge([a, norm(1, mean=0.5, std=0.25, dtype="float16", layout="chw")], 0, device)["image"]
        assert ok.shape == (2, 3, 224, 224)


def small_samples(n, seed):
    shapes = [(96, 128), (75, 100), (100, 75), (80, 120)]
    return [dict(image=synth(*shapes[i % 4], 3, seed + i)) for i in range(n)]


def test_batch_split_over_devices_matches_the_unsplit_batch():
    """set_devices([0, 0]) with 128 images: two slices of 64 from two host
    threads, each its own device block and copy back, the same format."""
    from mlx_data_amd import _pipeline

    assert len(_pipeline._split_batch(128, 2)) == 2
    raw = small_samples(128, seed=60)

    def run(devs, **kw):
        dx.set_devices(devs)
        d = (dx.buffer_from_vector(raw).image_resize_smallest_side("image", 72).image_random_crop("image", 64, 64)
             .image_random_h_flip("image", 0.5))
        dx.set_state(9)
        u8 = d.batch(128)[0]["image"]
        dx.set_state(9)
        return u8, d.image_normalize("image", **kw).batch(128)[0]["image"]

    kw = dict(mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="float16", layout="chw")
    u1, n1 = run([0], **kw)
    u2, n2 = run([0, 0], **kw)
    assert np.array_equal(u1, u2) and n1.shape == (128, 3, 64, 64)
    assert np.array_equal(bits(n1), bits(n2))
    assert np.array_equal(bits(n1), want_bits(u1, "float16", IMAGENET_MEAN, IMAGENET_STD, "chw"))


def test_ragged_batches_pad_and_videos_take_hwc():
    raw = [dict(image=synth(40 + 7 * i, 50 + 5 * i, 3, i)) for i in range(4)]
    b = dx.buffer_from_vector(raw)
    n = b.image_normalize("image", mean=0.5, std=0.5, dtype="float16", layout="chw")
    for got in (n.batch(4)[0]["image"], n.batch(4, device=0)[0]["image"].numpy()):
        assert got.shape == (4, 3, 61, 65) and got.dtype == np.float16
        for i, s in enumerate(raw):
            h, w, _ = s["image"].shape
            assert np.array_equal(bits(got[i, :, :h, :w]), want_bits(s["image"], "float16", 0.5, 0.5, "chw"))
            assert not got[i, :, h:, :].any() and not got[i, :, :, w:].any()  # zeros, as uint8 batches pad
    padded = n.batch(4, pad={"image": 1.5})[0]["image"]
    assert padded[0, 0, 60, 64] == np.float16(1.5)
    video = np.stack([synth(48, 64, 3, 20 + i) for i in range(3)])
    v = dx.buffer_from_vector([dict(image=video)]).image_resize("image", 32, 24)
    u8 = v[0]["image"]
    got = v.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="float16")[0]["image"]
    assert got.shape == (3, 24, 32, 3) and np.array_equal(bits(got), want_bits(u8, "float16", IMAGENET_MEAN, IMAGENET_STD))
    with pytest.raises(RuntimeError, match="chw"):
        v.image_normalize("image", layout="chw")[0]
