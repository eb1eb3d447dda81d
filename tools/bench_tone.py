"""What the tone call costs and what it saves: per-launch time of the resize
launch ending in normalised bfloat16 CHW with a per-image colour twist, with
a tone op in front of the twist, and with the passes users run today.

  python tools/bench_tone.py [--rounds 3] [--out profiles/r10/tone_ab.jsonl]

bench.py's method (its C2 and C4 workloads, resident device sets and
launch_windows: device events around windows of >= 100 launches and >= 20 ms,
3 per round), every variant warmed first, the variants alternated in one
process for --rounds rounds (so >= 6 windows each):

  a, a2   mxd_resize_crop_batch_color with a random twist per image, bfloat16
          CHW normalised (twice: the spread between the two is the spread the
          comparison is held to)
  b       mxd_resize_crop_batch_tone, MXD_TONE_EQUALIZE, same matrices and format
  bp      as b with MXD_TONE_CONTRAST (adds the luma histogram)
  c       what a user runs today: the u8 mxd_resize_crop_batch, then torch on
          the same stream -- per-image histograms (bincount), cumulative sum,
          the equalize table, gather, then baddbmm, + 0.5, clamp, floor, / 255,
          normalise, permute, cast to bfloat16

then, with every source byte set to one value (every lane of tone_hist adds
to one bin per channel), a_const and b_const.  --variants picks a subset (a
profiler run of the tone call alone: --variants b).

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

import numpy as np  # noqa: E402

import bench  # noqa: E402

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def run_workload(name, capi, torch, rounds, emit, only):
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
    rng = np.random.default_rng(9)
    mats = [capi.color_twist_matrix(rng.uniform(0.6, 1.4), rng.uniform(0.6, 1.4), rng.uniform(0.6, 1.4),
                                    rng.uniform(-18, 18)) for _ in range(B)]
    colors = capi.make_colors(mats)
    equalize = capi.make_tones([(capi.MXD_TONE_EQUALIZE, 0, 0.0)] * B)
    contrast = capi.make_tones([(capi.MXD_TONE_CONTRAST, 0, float(rng.uniform(0.6, 1.4))) for _ in range(B)])
    m = torch.tensor(np.stack(mats), device="cuda:0")  # (B, 3, 4), byte units
    mt = m[:, :, :3].transpose(1, 2).contiguous()      # x @ mt = (M x)^T
    off = m[:, :, 3].unsqueeze(1).contiguous()         # (B, 1, 3)
    mean_t = torch.tensor(MEAN, device="cuda:0")
    std_t = torch.tensor(STD, device="cuda:0")
    bins = (torch.arange(B, device="cuda:0").view(B, 1, 1) * 768 + torch.arange(3, device="cuda:0").view(1, 1, 3) * 256)
    ident = torch.arange(256, device="cuda:0").expand(B, 3, 256)
    npix = ch * cw

    def call(rc):
        if rc != 0:
            raise RuntimeError(L.mxd_last_error().decode())

    def a(i):
        call(L.mxd_resize_crop_batch_color(arrays["chw16"][i % 2], colors, B, capi.MXD_U8, ctypes.byref(fmt), dev, hs))

    def b(i):
        call(L.mxd_resize_crop_batch_tone(arrays["chw16"][i % 2], equalize, colors, B, capi.MXD_U8, ctypes.byref(fmt),
                                          dev, hs))

    def bp(i):
        call(L.mxd_resize_crop_batch_tone(arrays["chw16"][i % 2], contrast, colors, B, capi.MXD_U8, ctypes.byref(fmt),
                                          dev, hs))

    def c(i):
        call(L.mxd_resize_crop_batch(arrays["u8"][i % 2], B, capi.MXD_U8, dev, hs))
        with torch.cuda.stream(ext):
            idx = u8s[i % 2].view(B, npix, C).long() + bins
            hist = torch.bincount(idx.flatten(), minlength=B * 768).view(B, 3, 256)
            before = hist.cumsum(-1) - hist
            top = 255 - (hist > 0).flip(-1).long().argmax(-1, keepdim=True)
            step = (npix - hist.gather(-1, top)) // 255
            lut = torch.clamp((step // 2 + before) // step.clamp(min=1), max=255)
            lut = torch.where(step == 0, ident, lut)
            x = lut.view(-1)[idx].float()
            y = torch.baddbmm(off, x, mt)
            y = torch.floor(torch.clamp(y + 0.5, 0, 255))
            y = ((y / 255 - mean_t) / std_t).view(B, ch, cw, C)
            y.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous()

    variants = {k: f for k, f in {"a": a, "b": b, "bp": bp, "c": c, "a2": a}.items() if not only or k in only}

    def measure(vs, suffix=""):
        for f in vs.values():  # every shape and variant warmed first
            for i in range(10):
                f(i)
        stream.synchronize()
        windows = {k: [] for k in vs}
        for _ in range(rounds):
            for k, f in vs.items():
                windows[k] += bench.launch_windows(capi, stream, f, stream.synchronize)[2]
        med = {}
        for k, w in windows.items():
            med[k + suffix] = statistics.median(w)
            emit({"workload": name, "variant": k + suffix, "images": B, "ms_per_launch": round(med[k + suffix], 5),
                  "min": min(w), "max": max(w), "windows": w})
        return med

    try:
        med = measure(variants)
        if not only:
            for src, _, _, _ in sets:
                src.memset(0x80)
            stream.synchronize()
            med.update(measure({"a": a, "b": b}, "_const"))
            lo = min(med["a"], med["a2"])
            spread = abs(med["a"] - med["a2"]) / lo
            emit({"workload": name, "summary": True, "b_over_a": round(med["b"] / lo, 4),
                  "bp_over_a": round(med["bp"] / lo, 4), "b_over_c": round(med["b"] / med["c"], 4),
                  "c_over_b": round(med["c"] / med["b"], 2), "a_spread": round(spread, 4),
                  "b_const_over_a_const": round(med["b_const"] / med["a_const"], 4),
                  "b_const_over_b": round(med["b_const"] / med["b"], 4)})
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
        run_workload(wl, capi, torch, args.rounds, emit, only)


if __name__ == "__main__":
    main()
