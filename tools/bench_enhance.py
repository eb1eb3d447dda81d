"""What the enhance stage costs and what it saves: per-launch time of the resize
launch ending in normalised bfloat16 CHW, the same launch with a sharpness or
a color op per image in front of the format, and the route a user has today.

  python tools/bench_enhance.py [--rounds 3] [--out profiles/r12/enhance_ab.jsonl]

bench.py's method (its C2 and C4 workloads, resident device sets and
launch_windows: device events around windows of >= 100 launches and >= 20 ms,
3 per round), every variant warmed first, the variants alternated in one
process for --rounds rounds (3 rounds: 9 windows each):

  a, a2   mxd_resize_crop_batch_fmt, bfloat16 CHW normalised (twice: the
          spread between the two is the spread the comparison is held to)
  b       mxd_resize_crop_batch_enhance, MXD_ENHANCE_SHARPNESS 1.5 for every
          image, the same format (the stencil path of enhance_rows)
  c       as b with MXD_ENHANCE_COLOR 1.5 (the pointwise path)
  n       as b with MXD_ENHANCE_NONE (the stage as a copy: its fixed cost)
  d       what a user runs today: the u8 mxd_resize_crop_batch, then torch on
          the same stream -- depthwise conv2d with the / 13 kernel, the ring
          copy, the blend, truncate, clamp, / 255, normalise, permute and cast
          to bfloat16

--op blur times the Gaussian blur in the same A/B shape:

  b       mxd_resize_crop_batch_enhance, MXD_ENHANCE_GAUSSIAN_BLUR with k = 23
          and sigma 2.0 for every image (blur_rows), the same format
  bS_T    as b with S output rows per segment and T source rows per step
          (mxd_blur_shape), one variant per entry of --blur-shapes S:T,...
  d       the u8 mxd_resize_crop_batch, then torch on the same stream: reflect
          pad, depthwise conv2d with the outer product of the same weights,
          round, clamp, / 255, normalise, permute and cast to bfloat16
  a, a2, n as above; c is not run

--op pilblur times Pillow's GaussianBlur:

  p       mxd_resize_crop_batch_enhance, MXD_ENHANCE_PIL_GAUSSIAN_BLUR with
          radius 2 for every image (pilblur_rows), the same format
  p16     as p with radius 16: the design claims a cost that does not grow
          with the radius beyond the wider halo
  g       MXD_ENHANCE_GAUSSIAN_BLUR with k = 23 and sigma 2.0 (blur_rows) on
          the same images
  d       the u8 mxd_resize_crop_batch, then torch on the same stream: the six
          box passes (torch_pil_blur: replicate pad, a ones convolution, the
          8.24 weights in int64, the byte rounding after every pass), / 255,
          normalise, permute and cast to bfloat16
  a, a2, n as above

--op hue times Pillow's HSV hue shift:

  h       mxd_resize_crop_batch_enhance, MXD_ENHANCE_PIL_HUE with shift 25 for
          every image (hue_rows), the same format
  r       MXD_ENHANCE_BRIGHTNESS 1.5 on the same images: the pointwise path of
          enhance_rows, the same bytes moved -- the yardstick for h
  d       the u8 mxd_resize_crop_batch, then torch on the same stream: the two
          conversions as elementwise float32 / float64 ops (torch_pil_hue),
          / 255, normalise, permute and cast to bfloat16
  a, a2, n as above

--variants picks a subset (a profiler run of the enhance call alone: --variants b).
--lib times another build of the library: enhance.hip compiled with
-DMXD_ENH_LDS stages the tile and its halo in LDS instead of reading the
stencil's neighbours straight from the rows (DESIGN.md section 5k has both rows).

One JSON line per (workload, variant): median ms per launch over every window
of every round, min, max, the windows; then one summary line per workload."""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "mlx-data_amd"))

import bench  # noqa: E402

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
FACTOR = 1.5


BLUR_K, BLUR_SIGMA = 23, 2.0
PIL_RADIUS, PIL_RADIUS_WIDE = 2.0, 16.0


def torch_pil_blur(torch, x, R, ww, fw, passes):
    """Pillow's box passes on a float32 (B, C, H, W) tensor of byte values: the sums
    stay below 2^24, so float32 holds them exactly; the weights apply in int64."""
    import torch.nn.functional as F

    C = x.shape[1]
    ones = torch.ones((C, 1, 1, 2 * R + 1), dtype=torch.float32, device=x.device)
    for axis in (3, 2):
        for _ in range(passes):
            t = x if axis == 3 else x.transpose(2, 3)
            tp = F.pad(t, (R + 1, R + 1, 0, 0), mode="replicate")
            box = F.conv2d(tp[..., 1:-1], ones, groups=C)
            far = tp[..., :-2 * (R + 1)] + tp[..., 2 * (R + 1):]
            t = ((box.long() * ww + far.long() * fw + (1 << 23)) >> 24).float()
            x = t if axis == 3 else t.transpose(2, 3)
    return x


HUE_SHIFT = 25


def torch_pil_hue(torch, u8, shift):
    """MXD_ENHANCE_PIL_HUE's statement (include/mxd_amd.h) on a (..., 3) uint8 tensor:
    every operation at the statement's precision; returns float64 byte values."""
    x = u8.int()
    r, g, b = x.unbind(-1)
    maxc, minc = x.amax(-1), x.amin(-1)
    grey = maxc == minc
    cr = torch.where(grey, 1, maxc - minc).float()
    s = (maxc - minc).float() / torch.where(grey, 1, maxc).float()
    rc, gc, bc = ((maxc - c).float() / cr for c in (r, g, b))
    h = torch.where(r == maxc, (bc - gc).double(),
                    torch.where(g == maxc, 2.0 + rc.double() - bc.double(), 4.0 + gc.double() - rc.double())).float()
    xh = h.double() / 6.0 + 1.0
    h = (xh - xh.floor()).float()
    H = (h.double() * 255.0).int().clamp(max=255)
    S = (s.double() * 255.0).int().clamp(max=255)
    hf = ((H + shift) & 255).float().double() * 6.0 / 255.0
    i = hf.floor()
    f = (hf - i).float()
    fs = (S.double() / 255.0).float()
    V = maxc.double()
    p = torch.floor(V * (1.0 - fs.double()) + 0.5)  # (C's round of a value that is never negative)
    q = torch.floor(V * (1.0 - (fs * f).double()) + 0.5)
    t = torch.floor(V * (1.0 - fs.double() * (1.0 - f.double())) + 0.5)
    pick = torch.tensor([[0, 1, 2], [3, 0, 2], [2, 0, 1], [2, 3, 0], [1, 2, 0], [0, 2, 3]], device=u8.device)  # of V, t, p, q
    out = torch.gather(torch.stack([V, t, p, q], -1), -1, pick[i.long() % 6]).clamp(0, 255)
    return torch.where((S == 0).unsqueeze(-1), V.unsqueeze(-1), out)


def run_workload(name, capi, torch, rounds, emit, only, op="sharpness", blur_shapes=()):
    import torch.nn.functional as F

    dev = 0
    L = capi.lib()
    B = bench.WORKLOADS[name]["batch"]
    sizes, geoms, _ = bench.make_workload(capi, name, B, 0)
    C, cw, ch = bench.C, 224, 224
    assert all(g[4] == cw and g[5] == ch for g in geoms)
    stream = capi.Stream(dev)
    hs = ctypes.c_void_p(stream.handle)
    sets, _ = bench.device_sets(capi, dev, sizes, geoms, False, 2, 3000)
    ext = torch.cuda.ExternalStream(stream.handle, device=torch.device("cuda:0"))
    u8s = [torch.empty((B, ch, cw, C), dtype=torch.uint8, device="cuda:0") for _ in sets]
    outs = [torch.empty((B, C, ch, cw), dtype=torch.bfloat16, device="cuda:0") for _ in sets]
    arrays = {"u8": [], "chw16": []}
    for (src, dst, imgs, n), x, y in zip(sets, u8s, outs):
        for kind in arrays:
            arr = (capi.MxdImage * n)()
            ctypes.memmove(arr, imgs, ctypes.sizeof(arr))
            for i in range(n):
                arr[i].dst = x.data_ptr() + i * ch * cw * C if kind == "u8" else y.data_ptr() + i * C * ch * cw * 2
                arr[i].dst_stride = cw * C if kind == "u8" else cw * 2
            arrays[kind].append(arr)
    fmt = capi.make_out_format(capi.MXD_ELEM_BF16, capi.MXD_LAYOUT_CHW, MEAN, STD, plane_stride=ch * cw * 2)
    sharp = capi.make_enhances([(capi.MXD_ENHANCE_SHARPNESS, FACTOR)] * B)
    color = capi.make_enhances([(capi.MXD_ENHANCE_COLOR, FACTOR)] * B)
    none = capi.make_enhances([(capi.MXD_ENHANCE_NONE, 0.0)] * B)
    smooth = torch.tensor([[1.0, 1.0, 1.0], [1.0, 5.0, 1.0], [1.0, 1.0, 1.0]], device="cuda:0") / 13.0
    smooth = smooth.view(1, 1, 3, 3).expand(C, 1, 3, 3).contiguous()
    mean_t = torch.tensor(MEAN, device="cuda:0").view(1, 3, 1, 1)
    std_t = torch.tensor(STD, device="cuda:0").view(1, 3, 1, 1)

    def call(rc):
        if rc != 0:
            raise RuntimeError(L.mxd_last_error().decode())

    def a(i):
        call(L.mxd_resize_crop_batch_fmt(arrays["chw16"][i % 2], B, ctypes.byref(fmt), dev, hs))

    def enhance_call(enhs):
        def f(i):
            call(L.mxd_resize_crop_batch_enhance(arrays["chw16"][i % 2], None, enhs, None, None, B, capi.MXD_U8,
                                                 ctypes.byref(fmt), dev, hs))
        return f

    def d(i):
        call(L.mxd_resize_crop_batch(arrays["u8"][i % 2], B, capi.MXD_U8, dev, hs))
        with torch.cuda.stream(ext):
            x = u8s[i % 2].permute(0, 3, 1, 2).float()
            deg = x.clone()
            deg[:, :, 1:-1, 1:-1] = torch.floor(F.conv2d(x, smooth, groups=C) + 0.5)
            y = torch.clamp(torch.trunc(deg + FACTOR * (x - deg)), 0, 255)
            ((y / 255 - mean_t) / std_t).to(torch.bfloat16)

    every = {"a": a, "b": enhance_call(sharp), "c": enhance_call(color), "n": enhance_call(none), "d": d, "a2": a}
    if op == "blur":
        blur = capi.make_enhances([(capi.MXD_ENHANCE_GAUSSIAN_BLUR, BLUR_SIGMA, BLUR_K)] * B)
        w1 = torch.from_numpy(capi.gaussian_weights(BLUR_SIGMA, BLUR_K).copy()).to("cuda:0")
        w2 = torch.outer(w1, w1).view(1, 1, BLUR_K, BLUR_K).expand(C, 1, BLUR_K, BLUR_K).contiguous()

        def shaped(seg, step):
            f = enhance_call(blur)

            def g(i):
                capi.blur_shape(seg, step)
                f(i)
                capi.blur_shape(0, 0)
            return g

        def d_blur(i):
            call(L.mxd_resize_crop_batch(arrays["u8"][i % 2], B, capi.MXD_U8, dev, hs))
            with torch.cuda.stream(ext):
                x = F.pad(u8s[i % 2].permute(0, 3, 1, 2).float(), (BLUR_K // 2,) * 4, mode="reflect")
                y = torch.clamp(torch.round(F.conv2d(x, w2, groups=C)), 0, 255)
                ((y / 255 - mean_t) / std_t).to(torch.bfloat16)

        every = {"a": a, "b": enhance_call(blur), "n": enhance_call(none), "d": d_blur, "a2": a}
        every.update({f"b{seg}_{step}": shaped(seg, step) for seg, step in blur_shapes})
    if op == "pilblur":
        gauss = capi.MXD_ENHANCE_PIL_GAUSSIAN_BLUR
        fr, ww, fw, passes = capi.pil_blur_params(gauss, PIL_RADIUS)

        def d_pil(i):
            call(L.mxd_resize_crop_batch(arrays["u8"][i % 2], B, capi.MXD_U8, dev, hs))
            with torch.cuda.stream(ext):
                y = torch_pil_blur(torch, u8s[i % 2].permute(0, 3, 1, 2).float(), int(fr), ww, fw, passes)
                ((y / 255 - mean_t) / std_t).to(torch.bfloat16)

        every = {"a": a, "p": enhance_call(capi.make_enhances([(gauss, PIL_RADIUS)] * B)),
                 "p16": enhance_call(capi.make_enhances([(gauss, PIL_RADIUS_WIDE)] * B)),
                 "g": enhance_call(capi.make_enhances([(capi.MXD_ENHANCE_GAUSSIAN_BLUR, BLUR_SIGMA, BLUR_K)] * B)),
                 "n": enhance_call(none), "d": d_pil, "a2": a}
    if op == "hue":
        def d_hue(i):
            call(L.mxd_resize_crop_batch(arrays["u8"][i % 2], B, capi.MXD_U8, dev, hs))
            with torch.cuda.stream(ext):
                y = torch_pil_hue(torch, u8s[i % 2], HUE_SHIFT).float().permute(0, 3, 1, 2)
                ((y / 255 - mean_t) / std_t).to(torch.bfloat16)

        every = {"a": a, "h": enhance_call(capi.make_enhances([(capi.MXD_ENHANCE_PIL_HUE, 0.0, HUE_SHIFT)] * B)),
                 "r": enhance_call(capi.make_enhances([(capi.MXD_ENHANCE_BRIGHTNESS, FACTOR)] * B)),
                 "n": enhance_call(none), "d": d_hue, "a2": a}
    variants = {k: f for k, f in every.items() if not only or k in only}
    try:
        for f in variants.values():  # every shape and variant warmed first
            for i in range(10):
                f(i)
        stream.synchronize()
        windows = {k: [] for k in variants}
        for _ in range(rounds):
            for k, f in variants.items():
                windows[k] += bench.launch_windows(capi, stream, f, stream.synchronize)[2]
        med = {}
        for k, w in windows.items():
            med[k] = statistics.median(w)
            emit({"workload": name, "variant": k, "images": B, "ms_per_launch": round(med[k], 5), "min": min(w),
                  "max": max(w), "windows": w})
        if not only and op == "hue":
            lo = min(med["a"], med["a2"])
            emit({"workload": name, "summary": True, "op": "pil_hue", "shift": HUE_SHIFT,
                  "h_over_a": round(med["h"] / lo, 4), "r_over_a": round(med["r"] / lo, 4), "n_over_a": round(med["n"] / lo, 4),
                  "h_over_r": round(med["h"] / med["r"], 4), "d_over_h": round(med["d"] / med["h"], 2),
                  "a_spread": round(abs(med["a"] - med["a2"]) / lo, 4)})
        elif not only and op == "pilblur":
            lo = min(med["a"], med["a2"])
            emit({"workload": name, "summary": True, "op": "pil_gaussian_blur", "radius": PIL_RADIUS,
                  "p_over_a": round(med["p"] / lo, 4), "n_over_a": round(med["n"] / lo, 4),
                  "p_over_g": round(med["p"] / med["g"], 4), "d_over_p": round(med["d"] / med["p"], 2),
                  "p16_over_p": round(med["p16"] / med["p"], 4), "a_spread": round(abs(med["a"] - med["a2"]) / lo, 4)})
        elif not only and op == "blur":
            lo = min(med["a"], med["a2"])
            emit({"workload": name, "summary": True, "op": "gaussian_blur", "k": BLUR_K, "sigma": BLUR_SIGMA,
                  "b_over_a": round(med["b"] / lo, 4), "n_over_a": round(med["n"] / lo, 4),
                  "d_over_b": round(med["d"] / med["b"], 2), "a_spread": round(abs(med["a"] - med["a2"]) / lo, 4),
                  "shapes_over_a": {k: round(m / lo, 4) for k, m in med.items() if k.startswith("b") and k != "b"}})
        elif not only:
            lo = min(med["a"], med["a2"])
            emit({"workload": name, "summary": True, "b_over_a": round(med["b"] / lo, 4), "c_over_a": round(med["c"] / lo, 4),
                  "n_over_a": round(med["n"] / lo, 4), "d_over_b": round(med["d"] / med["b"], 2),
                  "d_over_c": round(med["d"] / med["c"], 2), "a_spread": round(abs(med["a"] - med["a2"]) / lo, 4)})
    finally:
        stream.synchronize()
        for src, dst, _, _ in sets:
            src.free()
            dst.free()
        stream.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default="c2,c4")
    ap.add_argument("--variants", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--op", default="sharpness", choices=("sharpness", "blur", "pilblur", "hue"))
    ap.add_argument("--blur-shapes", default="", help="--op blur: segment rows : rows per step, e.g. 32:8,112:8,56:4")
    ap.add_argument("--lib", default="", help="another build of libmxd_amd.so to time (a compile-time variant)")
    args = ap.parse_args()
    import torch  # torch first: its HIP runtime is the one the libraries bind

    torch.zeros(1, device="cuda:0")
    from mlx_data_amd import capi

    if args.lib:
        capi.LIB_PATH = os.path.abspath(args.lib)
    capi.check(capi.lib().mxd_set_device(0))
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    name, arch, cus = capi.device_properties(0)
    emit({"device": name, "arch": arch, "cus": cus, "rounds": args.rounds, "torch": torch.__version__,
          "lib": os.path.basename(args.lib) if args.lib else "product",
          "method": "bench.launch_windows: device events, windows >= 100 launches and >= 20 ms, 3 per round"})
    only = set(args.variants.split(",")) if args.variants else set()
    for wl in args.workloads.split(","):
        shapes = [tuple(int(v) for v in s.split(":")) for s in args.blur_shapes.split(",") if s]
        run_workload(wl, capi, torch, args.rounds, emit, only, args.op, shapes)


if __name__ == "__main__":
    main()
