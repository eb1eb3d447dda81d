"""GPU: the enhance ops of the operator surface (image_sharpness, image_color,
image_brightness and their random forms).  The expectation is always Pillow
(tests/enhance_ref.py: ImageEnhance.*) on the uint8 result of the same chain
without the op, then Pillow's tone op and the NumPy statements of the colour
map and the output format; compared as integer bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import color_ref as C
import enhance_ref as E
import tone_ref as T
import warp_ref as W
from gpu_util import synth
from mlx_data_amd import _pipeline, capi
from mlx_data_amd import data as dx
from out_format_util import IMAGENET_MEAN, IMAGENET_STD
from test_gpu_tone_surface import EQ, bits, chain, formatted, plan, samples

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {E.SHARPNESS: "sharpness", E.COLOR: "color", E.BRIGHTNESS: "brightness"}


def enhanced(batch, op, factor):
    """ImageEnhance.<op>(image).enhance(factor) on every (H, W, 3) image of a batch."""
    return np.stack([E.pillow_apply(np.ascontiguousarray(x), (op, factor)) for x in batch])


def apply_op(b, op, factor, **kw):
    return getattr(b, "image_" + NAMES[op])("image", factor, **kw)


@pytest.fixture(autouse=True)
def one_device():
    before = dx.devices()
    dx.set_devices([0])
    yield
    dx.set_devices(before)


CONSUMER = r"""
import json, sys
import numpy as np
import torch                      # torch first: its HIP runtime is the one libmxd_amd.so binds
torch.zeros(1, device="cuda")
sys.path[:0] = [{repo!r}, {repo!r} + "/tests", {repo!r} + "/oracle", {repo!r} + "/mlx-data_amd"]
from mlx_data_amd import data as dx, _pipeline
import color_ref as C
import enhance_ref as E
import tone_ref as T
from test_gpu_enhance_surface import enhanced
from test_gpu_tone_surface import EQ, chain, formatted, samples
from out_format_util import IMAGENET_MEAN, IMAGENET_STD
b = chain(dx.buffer_from_vector(samples(8, 11)))
u8 = b.batch(8)[0]["image"]
t = (b.image_sharpness("image", 1.9).image_equalize("image").image_color_twist("image", 1.1, 0.9, 1.3, 15.0))
m = np.float32(_pipeline._plan(t, 0, "image")["color"])
dev = (t.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="bfloat16", layout="chw")
       .batch(8, device=0)[0]["image"])
x = torch.from_dlpack(dev)
got = x.cpu().view(torch.int16).numpy().view(np.uint16)
s = enhanced(u8, E.SHARPNESS, 1.9)
eq = np.stack([T.pillow_apply(q, EQ) for q in s])
want = formatted(C.apply_ref(eq, m), "bfloat16", IMAGENET_MEAN, IMAGENET_STD, "chw")
print(json.dumps(dict(cuda=bool(x.is_cuda), dtype=str(x.dtype), shape=list(x.shape), ptr=x.data_ptr() == dev.data_ptr,
                      same=bool(np.array_equal(got, want)), moved=bool(not np.array_equal(s, u8)))))
"""


@pytest.mark.timeout(300)
def test_sharpness_equalize_twist_normalize_device_batch_through_dlpack():
    """sharpness -> equalize -> colour twist -> image_normalize(bfloat16, chw)
    -> batch(8, device=0) -> torch.from_dlpack: the batch tensor written in
    place by the enhance call."""
    r = subprocess.run([sys.executable, "-c", CONSUMER.format(repo=REPO)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == dict(cuda=True, dtype="torch.bfloat16", shape=[8, 3, 29, 33], ptr=True, same=True, moved=True), res


@pytest.mark.parametrize("op", E.OPS, ids=E.OP_IDS)
def test_host_batches_direct_reads_and_device_batches_agree_with_pillow(op):
    b = chain(dx.buffer_from_vector(samples(6, 3)))
    u8 = b.batch(6)[0]["image"]
    for factor in (0.3, 1.9):
        t = apply_op(b, op, factor)
        want = enhanced(u8, op, factor)
        assert not np.array_equal(want, u8)
        host = t.batch(6)[0]["image"]
        assert host.dtype == np.uint8 and host.shape == (6, 29, 33, 3) and np.array_equal(host, want), plan(t)["enhance"]
        assert np.array_equal(t[2]["image"], want[2])  # a direct read: a launch of its own
        assert np.array_equal(t.batch(6, device=0)[0]["image"].numpy(), want)
    t = apply_op(b, op, 1.9)
    want = enhanced(u8, op, 1.9)
    f = t.image_to_float("image")
    assert np.array_equal(bits(f.batch(6)[0]["image"]), formatted(want, "float32"))
    assert np.array_equal(bits(f.batch(6, device=0)[0]["image"].numpy()), formatted(want, "float32"))
    # equalize (of the enhanced bytes), a colour twist and image_normalize after the op
    tw = t.image_equalize("image").image_color_twist("image", 1.15, 0.8, 1.6, 25.0)
    m = np.float32(plan(tw)["color"])
    eq = np.stack([T.pillow_apply(q, EQ) for q in want])
    assert np.array_equal(tw.batch(6)[0]["image"], C.apply_ref(eq, m))
    n = tw.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="float16", layout="chw")
    ref = formatted(C.apply_ref(eq, m), "float16", IMAGENET_MEAN, IMAGENET_STD, "chw")
    assert np.array_equal(bits(n.batch(6)[0]["image"]), ref)
    assert np.array_equal(bits(n.batch(6, device=0)[0]["image"].numpy()), ref)
    # behind a warp of the same launch
    fill = (124, 116, 104)
    rw = apply_op(b.image_affine_rotate("image", 30.0, resample="bilinear", fill=fill), op, 1.9)
    assert plan(rw)["warp"] is not None and plan(rw)["enhance"] is not None
    rot = np.stack([W.pillow_rotate(x, 30.0, W.BILINEAR, fill) for x in u8])
    assert np.array_equal(rw.batch(6)[0]["image"], enhanced(rot, op, 1.9))


@pytest.mark.parametrize("op", E.OPS, ids=E.OP_IDS)
def test_a_flip_and_a_crop_after_the_op(op):
    r = dx.buffer_from_vector(samples(4, 7)).image_resize("image", 48, 40)
    u8 = r.batch(4)[0]["image"]
    t = apply_op(r, op, 1.9)
    want = enhanced(u8, op, 1.9)
    # a flip composes after all three: the same bytes as the flip of the enhanced image
    f = t.image_random_h_flip("image", 1.0)
    assert plan(f)["enhance"] is not None and plan(f)["flip"] and plan(f)["src_shape"] != [40, 48, 3]
    assert np.array_equal(f.batch(4)[0]["image"], want[:, :, ::-1])
    # a crop: composes after color and brightness, runs the pending sharpness first; the bytes are the crop of the whole
    a = t.image_center_crop("image", 20, 16)
    p = plan(a)
    assert p["crop"][2:] == (20, 16)
    if op == E.SHARPNESS:
        assert p["enhance"] is None and p["src_shape"] == [40, 48, 3] and p["crop"] == (14, 12, 20, 16)
    else:
        assert p["enhance"] is not None and p["src_shape"] != [40, 48, 3]
    assert np.array_equal(a.batch(4)[0]["image"], want[:, 12:28, 14:34])
    # a crop before the op: the op of the window (sharpness: its own ring)
    c = apply_op(r.image_center_crop("image", 20, 16), op, 1.9)
    assert plan(c)["enhance"] is not None and plan(c)["crop"][2:] == (20, 16)
    assert np.array_equal(c.batch(4)[0]["image"], enhanced(u8[:, 12:28, 14:34], op, 1.9))
    if op == E.SHARPNESS:
        assert not np.array_equal(c.batch(4)[0]["image"], want[:, 12:28, 14:34])


def test_what_materialises_the_pending_plan():
    r = dx.buffer_from_vector(samples(4, 7)).image_resize("image", 48, 40)
    u8 = r.batch(4)[0]["image"]
    t = r.image_sharpness("image", 1.9)
    want = enhanced(u8, E.SHARPNESS, 1.9)
    # a resize, image_rotate, a warp and a second enhance op after an enhance op
    rs = t.image_resize("image", 20, 16)
    assert plan(rs)["enhance"] is None and plan(rs)["src_shape"] == [40, 48, 3] and plan(rs)["resize"] == (20, 16)
    ref = dx.buffer_from_vector([dict(image=want[0])]).image_resize("image", 20, 16)[0]["image"]
    assert np.array_equal(rs[0]["image"], ref)
    ro = t.image_rotate("image", 90.0)[0]["image"]
    assert np.array_equal(ro, dx.buffer_from_vector([dict(image=want[0])]).image_rotate("image", 90.0)[0]["image"])
    tw = t.image_shear("image", 0.3, fill=9)
    assert plan(tw)["enhance"] is None and plan(tw)["warp"] is not None and plan(tw)["src_shape"] == [40, 48, 3]
    sheared = np.stack([W.pillow_apply(x, (W.NEAREST, 9, W.shear(0.3, 0.0))) for x in want])
    assert np.array_equal(tw.batch(4)[0]["image"], sheared)
    ee = t.image_color("image", 0.3)
    assert plan(ee)["enhance"] == ("color", float(np.float32(0.3))) and plan(ee)["src_shape"] == [40, 48, 3]
    assert np.array_equal(ee.batch(4)[0]["image"], enhanced(want, E.COLOR, 0.3))
    # an enhance op after a tone op and after a colour op: what is pending runs first, as written
    te = r.image_equalize("image").image_brightness("image", 1.9)
    p = plan(te)
    assert p["tone"] is None and p["enhance"] is not None and p["src_shape"] == [40, 48, 3]
    eq = np.stack([T.pillow_apply(q, EQ) for q in u8])
    assert np.array_equal(te.batch(4)[0]["image"], enhanced(eq, E.BRIGHTNESS, 1.9))
    m = capi.color_twist_matrix(1.2, 0.7)
    ce = r.image_color_twist("image", 1.2, 0.7).image_sharpness("image", 0.3)
    assert plan(ce)["color"] is None and plan(ce)["enhance"] is not None
    assert np.array_equal(ce.batch(4)[0]["image"], enhanced(C.apply_ref(u8, m), E.SHARPNESS, 0.3))


def test_if_form_on_half_the_samples_and_output_key():
    bufs, wants = [], []
    for k in range(4):
        b = chain(dx.buffer_from_vector(samples(1, 20 + k)))
        u8 = b[0]["image"]
        t = b.image_sharpness_if(k % 2 == 0, "image", 1.9)
        assert (plan(t)["enhance"] is not None) == (k % 2 == 0)
        bufs.append(t)
        wants.append(E.pillow_apply(u8, (E.SHARPNESS, 1.9)) if k % 2 == 0 else u8)
    for device in (None, 0):
        got = _pipeline._merge(bufs, 0, device)["image"]
        got = got.numpy() if device is not None else got
        assert np.array_equal(got, np.stack(wants)), device
    b = chain(dx.buffer_from_vector(samples(4, 50)))
    u8 = b.batch(4)[0]["image"]
    o = b.image_color("image", 0.3, output_key="grey").batch(4)[0]
    assert np.array_equal(o["image"], u8) and np.array_equal(o["grey"], enhanced(u8, E.COLOR, 0.3))


def test_a_ragged_host_batch():
    r = dx.buffer_from_vector(samples(4, 5)).image_resize_smallest_side("image", 30)
    plain = r.batch(4)[0]["image"]
    rag = r.image_sharpness("image", 1.9, output_key="sharp").batch(4)[0]
    assert plain.shape[1] != plain.shape[2] and np.array_equal(rag["image"], plain)
    for k, s in enumerate(samples(4, 5)):
        h, w = (30 * np.array(s["image"].shape[:2]) / min(s["image"].shape[:2])).round().astype(int)
        want = E.pillow_apply(np.ascontiguousarray(plain[k, :h, :w]), (E.SHARPNESS, 1.9))
        assert np.array_equal(rag["sharp"][k, :h, :w], want), k
        assert not rag["sharp"][k, h:].any() and not rag["sharp"][k, :, w:].any()


def test_a_batch_split_over_two_slices_carries_each_slice_s_entries():
    """set_devices([0, 0]): 128 images in two slices of 64; every fourth image
    untouched, the others with one of the three ops at a factor of their own."""
    n = 128
    bufs, want = [], []
    for i in range(n):
        b = dx.buffer_from_vector([dict(image=synth(24, 28, 3, 500 + i))]).image_resize("image", 20, 16)
        q = b[0]["image"]
        f = 0.02 * i
        bufs.append([b, b.image_sharpness("image", f), b.image_color("image", f), b.image_brightness("image", f)][i % 4])
        want.append(q if i % 4 == 0 else E.pillow_apply(q, (i % 4, float(np.float32(f)))))
    dx.set_devices([0, 0])
    assert np.array_equal(_pipeline._merge(bufs, 0, None)["image"], np.stack(want))


def test_a_video_whose_frames_differ_draws_once():
    video = np.stack([synth(20, 24, 3, 60), synth(20, 24, 3, 61), synth(20, 24, 3, 62)])
    b = dx.buffer_from_vector([dict(image=video)])
    for seed, op in ((5, E.SHARPNESS), (6, E.COLOR), (7, E.BRIGHTNESS)):
        dx.set_state(seed)
        got = getattr(b, "image_random_" + NAMES[op])("image", factor=(0.2, 1.8))[0]["image"]
        words = np.random.RandomState(seed)
        r0, r1 = (int(words.randint(0, 2 ** 32, dtype=np.uint64)) for _ in range(2))
        f = (float(r0) + float(r1) * 4294967296.0) / 18446744073709551616.0 * (1.8 - 0.2) + 0.2
        assert got.shape == video.shape and np.array_equal(got, enhanced(video, op, float(np.float32(f))))
        assert np.array_equal(apply_op(b, op, f)[0]["image"], got)


def test_the_random_ops_equal_the_fixed_ops_with_the_restated_draws():
    b = chain(dx.buffer_from_vector(samples(4, 40)))
    u8 = b.batch(4)[0]["image"]
    # batch() prepares its samples in order on this thread: image k takes draw k
    for seed, op in ((9, E.SHARPNESS), (10, E.COLOR), (11, E.BRIGHTNESS)):
        dx.set_state(seed)
        got = getattr(b, "image_random_" + NAMES[op])("image", factor=(0.1, 1.9)).batch(4)[0]["image"]
        words = np.random.RandomState(seed)
        want = []
        for k in range(4):
            r0, r1 = (int(words.randint(0, 2 ** 32, dtype=np.uint64)) for _ in range(2))
            f = (float(r0) + float(r1) * 4294967296.0) / 18446744073709551616.0 * (1.9 - 0.1) + 0.1
            want.append(E.pillow_apply(u8[k], (op, float(np.float32(f)))))
        assert np.array_equal(got, np.stack(want)), NAMES[op]


def test_batches_without_an_enhanced_plan_make_the_calls_they_made():
    """The _enhance calls refuse everything but three channels: one- and
    four-channel batches, and warped, toned and coloured RGB batches, still run as before."""
    for c in (1, 4):
        imgs = [synth(40, 60, c, 80 + k) for k in range(3)]
        b = dx.buffer_from_vector([dict(image=i) for i in imgs]).image_resize("image", 30, 20)
        assert plan(b)["enhance"] is None
        host = b.batch(3)[0]["image"]
        assert host.shape == (3, 20, 30, c) and np.array_equal(b.batch(3, device=0)[0]["image"].numpy(), host)
    b = chain(dx.buffer_from_vector(samples(3, 70)))
    u8 = b.batch(3)[0]["image"]
    m = capi.color_twist_matrix(1.2, 0.7)
    assert np.array_equal(b.image_color_twist("image", 1.2, 0.7).batch(3)[0]["image"], C.apply_ref(u8, m))
    assert np.array_equal(b.image_equalize("image").batch(3)[0]["image"], np.stack([T.pillow_apply(q, EQ) for q in u8]))
    sheared = np.stack([W.pillow_apply(x, (W.NEAREST, 0, W.shear(0.3, 0.0))) for x in u8])
    assert np.array_equal(b.image_shear("image", 0.3).batch(3)[0]["image"], sheared)
