"""GPU: the tone ops of the operator surface (image_posterize, image_solarize,
image_autocontrast, image_equalize, image_contrast).  The expectation is
always Pillow (tests/tone_ref.py: pillow_apply) on the uint8 result of the same
chain without the op, then the NumPy statements of the colour map and the
output format; compared as integer bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import color_ref as C
import tone_ref as T
from gpu_util import synth
from mlx_data_amd import _pipeline, capi
from mlx_data_amd import data as dx
from out_format_util import IMAGENET_MEAN, IMAGENET_STD, expected_table

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(61, 97), (97, 61), (80, 80), (50, 120)]
EQ, AC, CON = (T.EQUALIZE, 0, 0.0), (T.AUTOCONTRAST, 0, 0.0), (T.CONTRAST, 0, 1.4)


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


def pil(batch, tone):
    """Pillow's op on every (H, W, 3) image of a batch: each with its own statistics."""
    return np.stack([T.pillow_apply(x, tone) for x in batch])


def plan(b, i=0, key="image"):
    return _pipeline._plan(b, i, key)


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
from test_gpu_tone_surface import EQ, chain, formatted, pil, samples
from out_format_util import IMAGENET_MEAN, IMAGENET_STD
b = chain(dx.buffer_from_vector(samples(8, 11)))
u8 = b.batch(8)[0]["image"]
t = b.image_equalize("image").image_color_twist("image", 1.1, 0.9, 1.3, 15.0)
m = np.float32(_pipeline._plan(t, 0, "image")["color"])
dev = (t.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="bfloat16", layout="chw")
       .batch(8, device=0)[0]["image"])
x = torch.from_dlpack(dev)
got = x.cpu().view(torch.int16).numpy().view(np.uint16)
eq = pil(u8, EQ)
want = formatted(C.apply_ref(eq, m), "bfloat16", IMAGENET_MEAN, IMAGENET_STD, "chw")
print(json.dumps(dict(cuda=bool(x.is_cuda), dtype=str(x.dtype), shape=list(x.shape), ptr=x.data_ptr() == dev.data_ptr,
                      same=bool(np.array_equal(got, want)), moved=bool(not np.array_equal(eq, u8)))))
"""


@pytest.mark.timeout(300)
def test_equalize_twist_normalize_device_batch_through_dlpack():
    """equalize -> colour twist -> image_normalize(bfloat16, chw) ->
    batch(8, device=0) -> torch.from_dlpack: the batch tensor written in place
    by the tone call."""
    r = subprocess.run([sys.executable, "-c", CONSUMER.format(repo=REPO)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == dict(cuda=True, dtype="torch.bfloat16", shape=[8, 3, 29, 33], ptr=True, same=True, moved=True), res


def test_host_batches_direct_reads_and_device_batches_agree_with_pillow():
    b = chain(dx.buffer_from_vector(samples(6, 3)))
    u8 = b.batch(6)[0]["image"]
    for make, tone in ((lambda x: x.image_equalize("image"), EQ), (lambda x: x.image_autocontrast("image"), AC),
                       (lambda x: x.image_contrast("image", 1.4), CON),
                       (lambda x: x.image_posterize("image", 3), (T.POSTERIZE, 3, 0.0)),
                       (lambda x: x.image_solarize("image", 90), (T.SOLARIZE, 90, 0.0))):
        t = make(b)
        want = pil(u8, tone)
        assert not np.array_equal(want, u8)
        host = t.batch(6)[0]["image"]
        assert host.dtype == np.uint8 and host.shape == (6, 29, 33, 3) and np.array_equal(host, want), T.NAMES[tone[0]]
        assert np.array_equal(t[2]["image"], want[2])  # a direct read: a launch of its own
        assert np.array_equal(t.batch(6, device=0)[0]["image"].numpy(), want)
    t = b.image_equalize("image")
    want = pil(u8, EQ)
    f = t.image_to_float("image")
    assert np.array_equal(bits(f.batch(6)[0]["image"]), formatted(want, "float32"))
    assert np.array_equal(bits(f.batch(6, device=0)[0]["image"].numpy()), formatted(want, "float32"))
    # a colour twist and image_normalize after image_equalize (float16 here: bfloat16 has no NumPy type
    # and goes through DLPack in the test above)
    tw = t.image_color_twist("image", 1.15, 0.8, 1.6, 25.0)
    m = np.float32(plan(tw)["color"])
    assert plan(tw)["tone"] == ("equalize", None)
    assert np.array_equal(tw.batch(6)[0]["image"], C.apply_ref(want, m))
    n = tw.image_normalize("image", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="float16", layout="chw")
    ref = formatted(C.apply_ref(want, m), "float16", IMAGENET_MEAN, IMAGENET_STD, "chw")
    assert np.array_equal(bits(n.batch(6)[0]["image"]), ref)
    assert np.array_equal(bits(n.batch(6, device=0)[0]["image"].numpy()), ref)


def test_crops_and_flips_after_a_tone_op():
    r = dx.buffer_from_vector(samples(4, 7)).image_resize("image", 48, 40)
    u8 = r.batch(4)[0]["image"]
    # autocontrast then a crop: Pillow's autocontrast of the whole, then the crop (the crop materialises the op)
    a = r.image_autocontrast("image").image_center_crop("image", 20, 16)
    p = plan(a)
    assert p["tone"] is None and p["src_shape"] == [40, 48, 3] and p["crop"] == (14, 12, 20, 16)
    want = pil(u8, AC)[:, 12:28, 14:34]
    assert np.array_equal(a.batch(4)[0]["image"], want)
    assert not np.array_equal(want, pil(u8[:, 12:28, 14:34], AC))  # (the other order differs)
    for make in (lambda x: x.image_equalize("image"), lambda x: x.image_contrast("image", 0.5)):
        q = plan(make(r).image_random_crop("image", 9, 7))
        assert q["tone"] is None and q["src_shape"] == [40, 48, 3]
    # a crop before the op: the statistics of the window
    c = r.image_center_crop("image", 20, 16).image_equalize("image")
    assert plan(c)["tone"] == ("equalize", None)
    assert np.array_equal(c.batch(4)[0]["image"], pil(u8[:, 12:28, 14:34], EQ))
    # posterize then a crop composes; a flip after any tone op composes and leaves the statistics alone
    ps = r.image_posterize("image", 2).image_center_crop("image", 20, 16)
    assert plan(ps)["tone"] == ("posterize", 2) and plan(ps)["resize"] == (48, 40)
    assert np.array_equal(ps.batch(4)[0]["image"], pil(u8, (T.POSTERIZE, 2, 0.0))[:, 12:28, 14:34])
    fl = r.image_equalize("image").image_random_h_flip("image", 1.0)
    assert plan(fl)["tone"] == ("equalize", None) and plan(fl)["flip"]
    assert np.array_equal(fl.batch(4)[0]["image"], pil(u8, EQ)[:, :, ::-1])
    assert np.array_equal(fl.batch(4, device=0)[0]["image"].numpy(), pil(u8, EQ)[:, :, ::-1])


def test_what_materialises_the_pending_op():
    b = chain(dx.buffer_from_vector(samples(2, 30)))
    u8 = b.batch(2)[0]["image"]
    # a second tone op: the plan holds the second only, over the first's bytes
    two = b.image_equalize("image").image_contrast("image", 1.7)
    p = plan(two)
    assert p["tone"] == ("contrast", np.float32(1.7)) and p["src_shape"] == [29, 33, 3] and p["resize"] == (33, 29)
    assert np.array_equal(two.batch(2)[0]["image"], pil(pil(u8, EQ), (T.CONTRAST, 0, 1.7)))
    # a tone op on a coloured plan: colour first, as written
    m = capi.color_twist_matrix(1.2, 0.7)
    ct = b.image_color_twist("image", 1.2, 0.7).image_autocontrast("image")
    p = plan(ct)
    assert p["tone"] == ("autocontrast", None) and p["color"] is None and p["src_shape"] == [29, 33, 3]
    assert np.array_equal(ct.batch(2)[0]["image"], pil(C.apply_ref(u8, m), AC))
    # a resize on a toned plan
    rs = b.image_solarize("image", 100).image_resize("image", 20, 16)
    p = plan(rs)
    assert p["tone"] is None and p["src_shape"] == [29, 33, 3] and p["resize"] == (20, 16)
    one = pil(u8, (T.SOLARIZE, 100, 0.0))
    want = dx.buffer_from_vector([dict(image=one[0])]).image_resize("image", 20, 16)[0]["image"]
    assert np.array_equal(rs[0]["image"], want)


def test_if_form_on_half_the_samples_and_output_key():
    bufs, wants = [], []
    for k in range(4):
        b = chain(dx.buffer_from_vector(samples(1, 20 + k)))
        u8 = b[0]["image"]
        t = b.image_equalize_if(k % 2 == 0, "image")
        assert (plan(t)["tone"] is not None) == (k % 2 == 0)
        bufs.append(t)
        wants.append(T.pillow_apply(u8, EQ) if k % 2 == 0 else u8)
    for device in (None, 0):
        got = _pipeline._merge(bufs, 0, device)["image"]
        got = got.numpy() if device is not None else got
        assert np.array_equal(got, np.stack(wants)), device
    b = chain(dx.buffer_from_vector(samples(4, 50)))
    u8 = b.batch(4)[0]["image"]
    o = b.image_contrast("image", 1.4, output_key="punchy").batch(4)[0]
    assert np.array_equal(o["image"], u8) and np.array_equal(o["punchy"], pil(u8, CON))


def test_a_ragged_host_batch():
    r = dx.buffer_from_vector(samples(4, 5)).image_resize_smallest_side("image", 30)
    plain = r.batch(4)[0]["image"]
    rag = r.image_equalize("image", output_key="eq").batch(4)[0]
    assert plain.shape[1] != plain.shape[2] and np.array_equal(rag["image"], plain)
    for k, s in enumerate(samples(4, 5)):
        h, w = (30 * np.array(s["image"].shape[:2]) / min(s["image"].shape[:2])).round().astype(int)
        assert np.array_equal(rag["eq"][k, :h, :w], T.pillow_apply(np.ascontiguousarray(plain[k, :h, :w]), EQ)), k
        assert not rag["eq"][k, h:].any() and not rag["eq"][k, :, w:].any()


def test_a_batch_split_over_two_slices_carries_each_slice_s_tones():
    """set_devices([0, 0]): 128 images in two slices of 64; every fourth image
    untouched, the others with one of three ops."""
    n = 128
    tones = [None, EQ, CON, (T.POSTERIZE, 2, 0.0)]
    bufs = []
    for i in range(n):
        b = dx.buffer_from_vector([dict(image=synth(24, 28, 3, 500 + i))]).image_resize("image", 20, 16)
        bufs.append([b, b.image_equalize("image"), b.image_contrast("image", 1.4), b.image_posterize("image", 2)][i % 4])
    plain = np.stack([dx.buffer_from_vector([dict(image=synth(24, 28, 3, 500 + i))]).image_resize("image", 20, 16)[0]["image"]
                      for i in range(n)])
    want = np.stack([plain[i] if tones[i % 4] is None else T.pillow_apply(plain[i], tones[i % 4]) for i in range(n)])
    dx.set_devices([0, 0])
    assert np.array_equal(_pipeline._merge(bufs, 0, None)["image"], want)


def test_video_frames_each_use_their_own_statistics():
    video = np.stack([synth(20, 24, 3, 60), synth(20, 24, 3, 61) // 2, synth(20, 24, 3, 62) // 3 + 90])
    assert video.shape == (3, 20, 24, 3)
    b = dx.buffer_from_vector([dict(image=video)])
    for make, tone in ((lambda x: x.image_autocontrast("image"), AC), (lambda x: x.image_equalize("image"), EQ),
                       (lambda x: x.image_contrast("image", 1.4), CON)):
        got = make(b)[0]["image"]
        want = pil(video, tone)
        assert got.shape == video.shape and np.array_equal(got, want), T.NAMES[tone[0]]
    # the whole video's statistics would give another result
    whole = T.apply(video.reshape(60, 24, 3), AC).reshape(video.shape)
    assert not np.array_equal(whole, pil(video, AC))
    small = b.image_resize("image", 12, 10)[0]["image"]
    f = b.image_resize("image", 12, 10).image_equalize("image").image_to_float("image")[0]["image"]
    assert np.array_equal(bits(f), formatted(pil(small, EQ), "float32"))


def test_batches_without_a_toned_plan_make_the_untoned_calls():
    """The _tone calls refuse everything but three channels: one- and
    four-channel batches, and a coloured RGB batch, still run as before."""
    for c in (1, 4):
        imgs = [synth(40, 60, c, 80 + k) for k in range(3)]
        b = dx.buffer_from_vector([dict(image=i) for i in imgs]).image_resize("image", 30, 20)
        assert plan(b)["tone"] is None
        host = b.batch(3)[0]["image"]
        assert host.shape == (3, 20, 30, c) and np.array_equal(b.batch(3, device=0)[0]["image"].numpy(), host)
    b = chain(dx.buffer_from_vector(samples(3, 70)))
    u8 = b.batch(3)[0]["image"]
    m = capi.color_twist_matrix(1.2, 0.7)
    assert np.array_equal(b.image_color_twist("image", 1.2, 0.7).batch(3)[0]["image"], C.apply_ref(u8, m))
