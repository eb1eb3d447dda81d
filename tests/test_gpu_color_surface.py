"""GPU: the colour ops of the operator surface (image_color_twist,
image_color_matrix, image_random_color_twist).  The expectation is always the
NumPy expression of the colour map (tests/color_ref.py) with the matrix _plan
reports, applied to the uint8 result of the same chain without the op, then
the NumPy / torch statement of the output format; compared as integer bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import color_ref as R
from gpu_util import synth
from mlx_data_amd import _pipeline, capi
from mlx_data_amd import data as dx
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expected_table

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(61, 97), (97, 61), (80, 80), (50, 120)]


def samples(n, seed=0):
    return [dict(image=synth(*SHAPES[i % 4], 3, seed + i), label=i) for i in range(n)]


def chain(b):
    return b.image_resize_smallest_side("image", 44).image_center_crop("image", 33, 29)


def bits(a):
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def formatted(u8, elem, mean=None, std=None, layout="hwc"):
    table = expected_table(elem, 3, mean, std)
    out = np.stack([table[k][u8[..., k]] for k in range(3)], axis=-1)
    return np.moveaxis(out, -1, -3) if layout == "chw" else out


def matrix(b, i=0, key="image"):
    return np.float32(_pipeline._plan(b, i, key)["color"])


@pytest.fixture(autouse=True)
def one_device():
    before = dx.devices()
    dx.set_devices([0])
    yield
    dx.set_devices(before)


TWIST = dict(brightness=1.15, contrast=0.8, saturation=1.6, hue=25.0)

CONSUMER = r"""
import json, sys
import numpy as np
import torch                      # torch first: its HIP runtime is the one libmxd_amd.so binds
torch.zeros(1, device="cuda")
sys.path[:0] = [{repo!r}, {repo!r} + "/tests", {repo!r} + "/oracle", {repo!r} + "/mlx-data_amd"]
from mlx_data_amd import data as dx, _pipeline
import color_ref as R
from test_gpu_color_surface import TWIST, chain, formatted, samples
from out_format_util import IMAGENET_MEAN, IMAGENET_STD
b = chain(dx.buffer_from_vector(samples(8, 11)))
u8 = b.batch(8)[0]["image"]
t = b.image_color_twist("image", **TWIST)
m = np.float32(_pipeline._plan(t, 0, "image")["color"])
dev = (t.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="bfloat16", layout="chw")
       .batch(8, device=0)[0]["image"])
x = torch.from_dlpack(dev)
got = x.cpu().view(torch.int16).numpy().view(np.uint16)
want = formatted(R.apply_ref(u8, m), "bfloat16", IMAGENET_MEAN, IMAGENET_STD, "chw")
print(json.dumps(dict(cuda=bool(x.is_cuda), dtype=str(x.dtype), shape=list(x.shape), ptr=x.data_ptr() == dev.data_ptr,
                      same=bool(np.array_equal(got, want)), moved=bool(not np.array_equal(R.apply_ref(u8, m), u8)))))
"""


@pytest.mark.timeout(300)
def test_twist_normalize_device_batch_through_dlpack():
    """twist -> image_normalize(bfloat16, chw) -> batch(8, device=0) ->
    torch.from_dlpack: the batch tensor written in place by the colour call."""
    r = subprocess.run([sys.executable, "-c", CONSUMER.format(repo=REPO)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == dict(cuda=True, dtype="torch.bfloat16", shape=[8, 3, 29, 33], ptr=True, same=True, moved=True), res


def test_host_batches_direct_reads_and_device_batches_agree():
    b = chain(dx.buffer_from_vector(samples(6, 3)))
    u8 = b.batch(6)[0]["image"]
    t = b.image_color_twist("image", **TWIST)
    m = matrix(t)
    assert np.array_equal(m, capi.color_twist_matrix(**TWIST))
    want = R.apply_ref(u8, m)
    assert not np.array_equal(want, u8)
    host = t.batch(6)[0]["image"]
    assert host.dtype == np.uint8 and host.shape == (6, 29, 33, 3) and np.array_equal(host, want)
    assert np.array_equal(t[2]["image"], want[2])  # a direct read: a launch of its own
    assert np.array_equal(t.batch(6, device=0)[0]["image"].numpy(), want)
    f = t.image_to_float("image")
    assert np.array_equal(bits(f.batch(6)[0]["image"]), formatted(want, "float32"))
    assert np.array_equal(bits(f[1]["image"]), formatted(want[1], "float32"))
    assert np.array_equal(bits(f.batch(6, device=0)[0]["image"].numpy()), formatted(want, "float32"))
    n = t.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="float16", layout="chw")
    assert np.array_equal(bits(n.batch(6)[0]["image"]), formatted(want, "float16", IMAGENET_MEAN, IMAGENET_STD, "chw"))
    # the matrix op, a channel swap with an offset; crops and flips after the op commute with it
    mm = np.array([[0, 0, 1, 0.1], [0, 1, 0, 0], [1, 0, 0, -0.1]])
    c = (dx.buffer_from_vector(samples(6, 3)).image_resize_smallest_side("image", 44)
         .image_color_matrix("image", mm).image_center_crop("image", 33, 29).image_random_h_flip("image", 1.0))
    assert np.array_equal(c.batch(6)[0]["image"], R.apply_ref(u8[:, :, ::-1], R.to_bytes_units(mm)))
    # a ragged host batch (rows strided in the batch) and an output key
    r = dx.buffer_from_vector(samples(4, 5)).image_resize_smallest_side("image", 30)
    plain = r.batch(4)[0]["image"]
    rag = r.image_color_twist("image", saturation=0.0, output_key="grey").batch(4)[0]
    assert plain.shape[1] != plain.shape[2] and np.array_equal(rag["image"], plain)
    grey = matrix(r.image_color_twist("image", saturation=0.0))
    for k, s in enumerate(samples(4, 5)):
        h, w = (30 * np.array(s["image"].shape[:2]) / min(s["image"].shape[:2])).round().astype(int)
        assert np.array_equal(rag["grey"][k, :h, :w], R.apply_ref(plain[k, :h, :w], grey)), k
        assert not rag["grey"][k, h:].any() and not rag["grey"][k, :, w:].any()


def test_if_form_on_half_the_samples_uses_the_identity_for_the_rest():
    bufs, wants = [], []
    for k in range(4):
        b = chain(dx.buffer_from_vector(samples(1, 20 + k)))
        u8 = b[0]["image"]
        t = b.image_color_twist_if(k % 2 == 0, "image", **TWIST)
        assert (_pipeline._plan(t, 0, "image")["color"] is not None) == (k % 2 == 0)
        bufs.append(t)
        wants.append(R.apply_ref(u8, capi.color_twist_matrix(**TWIST)) if k % 2 == 0 else u8)
    for device in (None, 0):
        got = _pipeline._merge(bufs, 0, device)["image"]
        got = got.numpy() if device is not None else got
        assert np.array_equal(got, np.stack(wants)), device


def test_second_colour_op_and_resize_materialise_the_first():
    b = chain(dx.buffer_from_vector(samples(2, 30)))
    u8 = b.batch(2)[0]["image"]
    one = R.apply_ref(u8, capi.color_twist_matrix(contrast=1.7))
    two = b.image_color_twist("image", contrast=1.7).image_color_twist("image", brightness=0.5)
    assert np.array_equal(matrix(two), capi.color_twist_matrix(brightness=0.5))  # the plan holds the second only
    assert _pipeline._plan(two, 0, "image")["src_shape"] == [29, 33, 3]
    assert np.array_equal(two.batch(2)[0]["image"], R.apply_ref(one, capi.color_twist_matrix(brightness=0.5)))
    rs = b.image_color_twist("image", contrast=1.7).image_resize("image", 20, 16)
    p = _pipeline._plan(rs, 0, "image")
    assert p["color"] is None and p["src_shape"] == [29, 33, 3] and p["resize"] == (20, 16)
    want = dx.buffer_from_vector([dict(image=one[0])]).image_resize("image", 20, 16)[0]["image"]
    assert np.array_equal(rs[0]["image"], want)


def test_random_twist_equals_the_matrices_the_plan_reports():
    b = chain(dx.buffer_from_vector(samples(6, 40)))
    u8 = b.batch(6)[0]["image"]
    r = b.image_random_color_twist("image", brightness=(0.6, 1.4), contrast=(0.6, 1.4), saturation=(0.0, 2.0),
                                   hue=(-40.0, 40.0))
    dx.set_state(17)
    mats = [matrix(r, i) for i in range(6)]
    assert len({m.tobytes() for m in mats}) == 6
    dx.set_state(17)
    got = r.image_normalize("image", dtype="float16").batch(6, device=0)[0]["image"].numpy()
    for k in range(6):
        assert np.array_equal(bits(got[k]), formatted(R.apply_ref(u8[k], mats[k]), "float16")), k
    dx.set_state(17)
    assert np.array_equal(r.batch(6)[0]["image"], np.stack([R.apply_ref(u8[k], mats[k]) for k in range(6)]))


def test_a_batch_split_over_two_slices_carries_each_slice_s_matrices():
    """set_devices([0, 0]): 128 images in two slices of 64, each with its own matrix."""
    n = 128
    b = dx.buffer_from_vector([dict(image=synth(24, 28, 3, 500 + i)) for i in range(n)]).image_resize("image", 20, 16)
    r = b.image_random_color_twist("image", brightness=(0.5, 1.5), hue=(-90.0, 90.0))
    u8 = b.batch(n)[0]["image"]
    dx.set_state(23)
    mats = [matrix(r, i) for i in range(n)]
    want = np.stack([R.apply_ref(u8[k], mats[k]) for k in range(n)])
    dx.set_devices([0, 0])
    dx.set_state(23)
    assert np.array_equal(r.batch(n)[0]["image"], want)
    dx.set_state(23)
    f = r.image_normalize("image", mean=0.4, std=0.3, dtype="float16", layout="chw").batch(n)[0]["image"]
    assert np.array_equal(bits(f), formatted(want, "float16", 0.4, 0.3, "chw"))


def test_video_frames_share_one_matrix():
    video = np.stack([synth(20, 24, 3, 60 + k) for k in range(3)])
    assert video.shape == (3, 20, 24, 3)
    b = dx.buffer_from_vector([dict(image=video)])
    m = capi.color_twist_matrix(**TWIST)
    assert np.array_equal(b.image_color_twist("image", **TWIST)[0]["image"], R.apply_ref(video, m))
    r = b.image_random_color_twist("image", saturation=(0.0, 2.0), hue=(-60.0, 60.0))
    dx.set_state(9)
    got = r[0]["image"]
    # one draw for the whole video: a single image after the same set_state draws the same matrix
    dx.set_state(9)
    one = matrix(dx.buffer_from_vector([dict(image=video[0])])
                 .image_random_color_twist("image", saturation=(0.0, 2.0), hue=(-60.0, 60.0)))
    assert got.shape == video.shape and np.array_equal(got, R.apply_ref(video, one))
    f = b.image_resize("image", 12, 10).image_color_twist("image", **TWIST).image_to_float("image")[0]["image"]
    small = b.image_resize("image", 12, 10)[0]["image"]
    assert np.array_equal(bits(f), formatted(R.apply_ref(small, m), "float32"))
