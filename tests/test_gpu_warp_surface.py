"""GPU: the warp ops of the operator surface (image_affine, image_shear,
image_translate, image_affine_rotate and their random forms).  The expectation
is always Pillow (tests/warp_ref.py) on the uint8 result of the same chain
without the op, then Pillow's tone op and the NumPy statements of the colour
map and the output format; compared as integer bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import color_ref as C
import tone_ref as T
import warp_ref as W
from gpu_util import synth
from mlx_data_amd import _pipeline, capi
from mlx_data_amd import data as dx
from out_format_util import IMAGENET_MEAN, IMAGENET_STD
from test_gpu_tone_surface import EQ, bits, chain, formatted, plan, samples

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = (124, 116, 104)


def rot(batch, angle, mode, fill=FILL):
    """Image.rotate on every (H, W, 3) image of a batch."""
    return np.stack([W.pillow_rotate(x, angle, mode, fill) for x in batch])


def warped(batch, mode, m, fill=FILL):
    """Image.transform(AFFINE) on every (H, W, 3) image of a batch."""
    return np.stack([W.pillow_apply(x, (mode, fill, m)) for x in batch])


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
import tone_ref as T
import warp_ref as W
from test_gpu_warp_surface import FILL, rot
from test_gpu_tone_surface import EQ, chain, formatted, samples
from out_format_util import IMAGENET_MEAN, IMAGENET_STD
b = chain(dx.buffer_from_vector(samples(8, 11)))
u8 = b.batch(8)[0]["image"]
t = (b.image_affine_rotate("image", 30.0, resample="bilinear", fill=FILL).image_equalize("image")
     .image_color_twist("image", 1.1, 0.9, 1.3, 15.0))
m = np.float32(_pipeline._plan(t, 0, "image")["color"])
dev = (t.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="bfloat16", layout="chw")
       .batch(8, device=0)[0]["image"])
x = torch.from_dlpack(dev)
got = x.cpu().view(torch.int16).numpy().view(np.uint16)
r = rot(u8, 30.0, W.BILINEAR)
eq = np.stack([T.pillow_apply(q, EQ) for q in r])
want = formatted(C.apply_ref(eq, m), "bfloat16", IMAGENET_MEAN, IMAGENET_STD, "chw")
print(json.dumps(dict(cuda=bool(x.is_cuda), dtype=str(x.dtype), shape=list(x.shape), ptr=x.data_ptr() == dev.data_ptr,
                      same=bool(np.array_equal(got, want)), moved=bool(not np.array_equal(r, u8)))))
"""


@pytest.mark.timeout(300)
def test_rotate_equalize_twist_normalize_device_batch_through_dlpack():
    """bilinear rotate -> equalize -> colour twist -> image_normalize(bfloat16,
    chw) -> batch(8, device=0) -> torch.from_dlpack: the batch tensor written
    in place by the warp call."""
    r = subprocess.run([sys.executable, "-c", CONSUMER.format(repo=REPO)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == dict(cuda=True, dtype="torch.bfloat16", shape=[8, 3, 29, 33], ptr=True, same=True, moved=True), res


def test_host_batches_direct_reads_and_device_batches_agree_with_pillow():
    b = chain(dx.buffer_from_vector(samples(6, 3)))
    u8 = b.batch(6)[0]["image"]
    for mode, name in ((W.NEAREST, "nearest"), (W.BILINEAR, "bilinear")):
        kw = dict(resample=name, fill=FILL)
        for t, want in ((b.image_shear("image", 0.3, -0.1, **kw), warped(u8, mode, W.shear(0.3, -0.1))),
                        (b.image_translate("image", 2.5, -1.25, **kw), warped(u8, mode, W.translate(2.5, -1.25))),
                        (b.image_affine("image", (0.9, 0.2, 1.5, -0.1, 1.1, -2.0), **kw),
                         warped(u8, mode, (0.9, 0.2, 1.5, -0.1, 1.1, -2.0))),
                        (b.image_affine_rotate("image", 30.0, **kw), rot(u8, 30.0, mode)),
                        (b.image_affine_rotate("image", -90.0, **kw), rot(u8, -90.0, mode))):
            assert not np.array_equal(want, u8)
            host = t.batch(6)[0]["image"]
            assert host.dtype == np.uint8 and host.shape == (6, 29, 33, 3) and np.array_equal(host, want), plan(t)["warp"]
            assert np.array_equal(t[2]["image"], want[2])  # a direct read: a launch of its own
            assert np.array_equal(t.batch(6, device=0)[0]["image"].numpy(), want)
    t = b.image_affine_rotate("image", 30.0, resample="bilinear", fill=FILL)
    want = rot(u8, 30.0, W.BILINEAR)
    f = t.image_to_float("image")
    assert np.array_equal(bits(f.batch(6)[0]["image"]), formatted(want, "float32"))
    assert np.array_equal(bits(f.batch(6, device=0)[0]["image"].numpy()), formatted(want, "float32"))
    # equalize (the fill pixels count), a colour twist and image_normalize after the warp
    tw = t.image_equalize("image").image_color_twist("image", 1.15, 0.8, 1.6, 25.0)
    m = np.float32(plan(tw)["color"])
    eq = np.stack([T.pillow_apply(q, EQ) for q in want])
    assert np.array_equal(tw.batch(6)[0]["image"], C.apply_ref(eq, m))
    n = tw.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="float16", layout="chw")
    ref = formatted(C.apply_ref(eq, m), "float16", IMAGENET_MEAN, IMAGENET_STD, "chw")
    assert np.array_equal(bits(n.batch(6)[0]["image"]), ref)
    assert np.array_equal(bits(n.batch(6, device=0)[0]["image"].numpy()), ref)


def test_what_materialises_the_pending_warp():
    r = dx.buffer_from_vector(samples(4, 7)).image_resize("image", 48, 40)
    u8 = r.batch(4)[0]["image"]
    w = r.image_affine_rotate("image", 30.0, resample="bilinear", fill=FILL)
    want = rot(u8, 30.0, W.BILINEAR)
    # a crop after a warp: the warp of the whole, then the crop
    a = w.image_center_crop("image", 20, 16)
    p = plan(a)
    assert p["warp"] is None and p["src_shape"] == [40, 48, 3] and p["crop"] == (14, 12, 20, 16)
    assert np.array_equal(a.batch(4)[0]["image"], want[:, 12:28, 14:34])
    # a crop before it: the warp of the window, about its own centre
    c = r.image_center_crop("image", 20, 16).image_affine_rotate("image", 30.0, resample="bilinear", fill=FILL)
    assert plan(c)["warp"] is not None and plan(c)["crop"] == (14, 12, 20, 16)
    assert np.array_equal(c.batch(4)[0]["image"], rot(u8[:, 12:28, 14:34], 30.0, W.BILINEAR))
    # a flip, a resize and image_rotate after a warp
    f = w.image_random_h_flip("image", 1.0)
    assert plan(f)["warp"] is None and plan(f)["flip"] and plan(f)["src_shape"] == [40, 48, 3]
    assert np.array_equal(f.batch(4)[0]["image"], want[:, :, ::-1])
    rs = w.image_resize("image", 20, 16)
    assert plan(rs)["warp"] is None and plan(rs)["src_shape"] == [40, 48, 3] and plan(rs)["resize"] == (20, 16)
    ref = dx.buffer_from_vector([dict(image=want[0])]).image_resize("image", 20, 16)[0]["image"]
    assert np.array_equal(rs[0]["image"], ref)
    ro = w.image_rotate("image", 90.0)[0]["image"]
    assert np.array_equal(ro, dx.buffer_from_vector([dict(image=want[0])]).image_rotate("image", 90.0)[0]["image"])
    # a warp after a tone op, a colour op and a warp: what is pending runs first, as written
    tw = r.image_equalize("image").image_shear("image", 0.3, fill=FILL)
    p = plan(tw)
    assert p["tone"] is None and p["warp"] is not None and p["src_shape"] == [40, 48, 3]
    eq = np.stack([T.pillow_apply(q, EQ) for q in u8])
    assert np.array_equal(tw.batch(4)[0]["image"], warped(eq, W.NEAREST, W.shear(0.3, 0.0)))
    m = capi.color_twist_matrix(1.2, 0.7)
    cw = r.image_color_twist("image", 1.2, 0.7).image_translate("image", 3.5, 2.0, resample="bilinear")
    assert plan(cw)["color"] is None and plan(cw)["warp"] is not None
    assert np.array_equal(cw.batch(4)[0]["image"], warped(C.apply_ref(u8, m), W.BILINEAR, W.translate(3.5, 2.0), 0))
    ww = w.image_shear("image", 0.0, 0.2, resample="bilinear", fill=9)
    assert plan(ww)["warp"][2] == W.shear(0.0, 0.2) and plan(ww)["src_shape"] == [40, 48, 3]
    assert np.array_equal(ww.batch(4)[0]["image"], warped(want, W.BILINEAR, W.shear(0.0, 0.2), 9))


def test_if_form_on_half_the_samples_and_output_key():
    bufs, wants = [], []
    for k in range(4):
        b = chain(dx.buffer_from_vector(samples(1, 20 + k)))
        u8 = b[0]["image"]
        t = b.image_affine_rotate_if(k % 2 == 0, "image", 30.0, resample="bilinear", fill=FILL)
        assert (plan(t)["warp"] is not None) == (k % 2 == 0)
        bufs.append(t)
        wants.append(W.pillow_rotate(u8, 30.0, W.BILINEAR, FILL) if k % 2 == 0 else u8)
    for device in (None, 0):
        got = _pipeline._merge(bufs, 0, device)["image"]
        got = got.numpy() if device is not None else got
        assert np.array_equal(got, np.stack(wants)), device
    b = chain(dx.buffer_from_vector(samples(4, 50)))
    u8 = b.batch(4)[0]["image"]
    o = b.image_shear("image", 0.3, fill=FILL, output_key="sheared").batch(4)[0]
    assert np.array_equal(o["image"], u8) and np.array_equal(o["sheared"], warped(u8, W.NEAREST, W.shear(0.3, 0.0)))


def test_a_ragged_host_batch():
    r = dx.buffer_from_vector(samples(4, 5)).image_resize_smallest_side("image", 30)
    plain = r.batch(4)[0]["image"]
    rag = r.image_affine_rotate("image", 30.0, resample="bilinear", fill=FILL, output_key="rot").batch(4)[0]
    assert plain.shape[1] != plain.shape[2] and np.array_equal(rag["image"], plain)
    for k, s in enumerate(samples(4, 5)):
        h, w = (30 * np.array(s["image"].shape[:2]) / min(s["image"].shape[:2])).round().astype(int)
        want = W.pillow_rotate(np.ascontiguousarray(plain[k, :h, :w]), 30.0, W.BILINEAR, FILL)
        assert np.array_equal(rag["rot"][k, :h, :w], want), k
        assert not rag["rot"][k, h:].any() and not rag["rot"][k, :, w:].any()


def test_a_batch_split_over_two_slices_carries_each_slice_s_warps():
    """set_devices([0, 0]): 128 images in two slices of 64; every fourth image
    untouched, the others with one of three warps."""
    n = 128
    bufs, want = [], []
    for i in range(n):
        b = dx.buffer_from_vector([dict(image=synth(24, 28, 3, 500 + i))]).image_resize("image", 20, 16)
        q = b[0]["image"]
        a = float(i)
        bufs.append([b, b.image_affine_rotate("image", a, resample="bilinear", fill=FILL),
                     b.image_shear("image", 0.01 * i, fill=FILL), b.image_translate("image", 0.1 * i, -2.0, fill=FILL)][i % 4])
        want.append([q, W.pillow_rotate(q, a, W.BILINEAR, FILL), W.pillow_apply(q, (W.NEAREST, FILL, W.shear(0.01 * i, 0.0))),
                     W.pillow_apply(q, (W.NEAREST, FILL, W.translate(0.1 * i, -2.0)))][i % 4])
    dx.set_devices([0, 0])
    assert np.array_equal(_pipeline._merge(bufs, 0, None)["image"], np.stack(want))


def test_a_video_draws_once_and_its_frames_share_the_matrix():
    video = np.stack([synth(20, 24, 3, 60), synth(20, 24, 3, 61), synth(20, 24, 3, 62)])
    b = dx.buffer_from_vector([dict(image=video)])
    dx.set_state(5)
    got = b.image_random_affine_rotate("image", (-30, 30), resample="bilinear", fill=FILL)[0]["image"]
    words = np.random.RandomState(5)
    r0, r1 = (int(words.randint(0, 2 ** 32, dtype=np.uint64)) for _ in range(2))
    angle = (float(r0) + float(r1) * 4294967296.0) / 18446744073709551616.0 * 60.0 + -30.0
    assert got.shape == video.shape and np.array_equal(got, rot(video, angle, W.BILINEAR))
    fixed = b.image_affine_rotate("image", angle, resample="bilinear", fill=FILL)[0]["image"]
    assert np.array_equal(fixed, got)


def test_the_random_ops_equal_the_fixed_ops_with_the_restated_draws():
    b = chain(dx.buffer_from_vector(samples(4, 40)))
    u8 = b.batch(4)[0]["image"]

    def draws(seed, ranges):
        words = np.random.RandomState(seed)
        out = []
        for lo, hi in ranges:
            r0, r1 = (int(words.randint(0, 2 ** 32, dtype=np.uint64)) for _ in range(2))
            out.append((float(r0) + float(r1) * 4294967296.0) / 18446744073709551616.0 * (float(hi) - float(lo)) + float(lo))
        return out

    # batch() prepares its samples in order on this thread: image k takes draws 2k and 2k + 1
    dx.set_state(9)
    got = b.image_random_shear("image", x=(-0.3, 0.3), y=(-0.2, 0.2), resample="bilinear", fill=FILL).batch(4)[0]["image"]
    d = draws(9, [(-0.3, 0.3), (-0.2, 0.2)] * 4)
    want = np.stack([W.pillow_apply(u8[k], (W.BILINEAR, FILL, W.shear(d[2 * k], d[2 * k + 1]))) for k in range(4)])
    assert np.array_equal(got, want)
    dx.set_state(10)
    got = b.image_random_translate("image", x=(-8, 8), fill=FILL).batch(4)[0]["image"]
    d = draws(10, [(-8, 8)] * 4)
    assert np.array_equal(got, np.stack([W.pillow_apply(u8[k], (W.NEAREST, FILL, W.translate(d[k], 0.0))) for k in range(4)]))
    dx.set_state(11)
    got = b.image_random_affine_rotate("image", (-45, 45), fill=FILL).batch(4)[0]["image"]
    d = draws(11, [(-45, 45)] * 4)
    assert np.array_equal(got, np.stack([W.pillow_rotate(u8[k], d[k], W.NEAREST, FILL) for k in range(4)]))


def test_batches_without_a_warped_plan_make_the_calls_they_made():
    """The _warp calls refuse everything but three channels: one- and
    four-channel batches, and toned and coloured RGB batches, still run as before."""
    for c in (1, 4):
        imgs = [synth(40, 60, c, 80 + k) for k in range(3)]
        b = dx.buffer_from_vector([dict(image=i) for i in imgs]).image_resize("image", 30, 20)
        assert plan(b)["warp"] is None
        host = b.batch(3)[0]["image"]
        assert host.shape == (3, 20, 30, c) and np.array_equal(b.batch(3, device=0)[0]["image"].numpy(), host)
    b = chain(dx.buffer_from_vector(samples(3, 70)))
    u8 = b.batch(3)[0]["image"]
    m = capi.color_twist_matrix(1.2, 0.7)
    assert np.array_equal(b.image_color_twist("image", 1.2, 0.7).batch(3)[0]["image"], C.apply_ref(u8, m))
    assert np.array_equal(b.image_equalize("image").batch(3)[0]["image"], np.stack([T.pillow_apply(q, EQ) for q in u8]))
