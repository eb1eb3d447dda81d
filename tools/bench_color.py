"""What the colour call costs and what it saves: per-launch time of the
resize launch ending in normalised bfloat16 CHW, without colour, with a
per-image colour twist, and with the second pass users run today.

  python tools/bench_color.py [--rounds 3] [--out profiles/r09/color_ab.jsonl]

bench.py's method (its C2 and C4 workloads, resident device sets and
launch_windows: device events around windows of >= 100 launches and >= 20 ms,
3 per round), every variant warmed first, the variants alternated in one
process for --rounds rounds (so >= 6 windows each):

  a, a2   mxd_resize_crop_batch_fmt, bfloat16 CHW normalised (no colour; twice:
          the spread between the two is the spread the comparison is held to)
  b       mxd_resize_crop_batch_color with a random twist per image, same format
  c       what a user runs today: the u8 mxd_resize_crop_batch, then torch on the
          device batch -- per-image baddbmm, + 0.5, clamp, floor, / 255,
          normalise, permute, cast to bfloat16 -- on the same stream

One JSON line per (workload, variant): median ms per launch over every window
of every round, min, max, the windows; then one summary line per workload with
b / a (the cost of the second pass) and whether b is slower than c beyond
the a / a2 spread."""
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


def run_workload(name, capi, torch, rounds, emit):
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
    # per set: the u8 batch variant c's torch pass reads, and the bfloat16 CHW batch a / b write
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
    m = torch.tensor(np.stack(mats), device="cuda:0")  # (B, 3, 4), byte units
    mt = m[:, :, :3].transpose(1, 2).contiguous()      # x @ mt = (M x)^T
    off = m[:, :, 3].unsqueeze(1).contiguous()         # (B, 1, 3)
    mean_t = torch.tensor(MEAN, device="cuda:0")
    std_t = torch.tensor(STD, device="cuda:0")

    def call(rc):
        if rc != 0:
            raise RuntimeError(L.mxd_last_error().decode())

    def a(i):
        call(L.mxd_resize_crop_batch_fmt(arrays["chw16"][i % 2], B, ctypes.byref(fmt), dev, hs))

    def b(i):
        call(L.mxd_resize_crop_batch_color(arrays["chw16"][i % 2], colors, B, capi.MXD_U8, ctypes.byref(fmt), dev, hs))

    def c(i):
        call(L.mxd_resize_crop_batch(arrays["u8"][i % 2], B, capi.MXD_U8, dev, hs))
        with torch.cuda.stream(ext):
            x = u8s[i % 2].view(B, ch * cw, C).float()
            y = torch.baddbmm(off, x, mt)
            y = torch.floor(torch.clamp(y + 0.5, 0, 255))
            y = ((y / 255 - mean_t) / std_t).view(B, ch, cw, C)
            y.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous()

    variants = {"a": a, "b": b, "c": c, "a2": a}
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
        spread = abs(med["a"] - med["a2"]) / min(med["a"], med["a2"])
        emit({"workload": name, "summary": True, "b_over_a": round(med["b"] / min(med["a"], med["a2"]), 4),
              "b_over_c": round(med["b"] / med["c"], 4), "a_spread": round(spread, 4),
              "b_not_slower_than_c": bool(med["b"] <= med["c"] * (1 + spread)),
              "scratch_mb": round(B * ((cw * C + 15) // 16 * 16) * ch / 1e6, 1)})
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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # torch first: its HIP runtime is the one the libraries bind

    torch.zeros(1, device="cuda:0")
    from mlx_data_amd import capi

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
          "method": "bench.launch_windows: device events, windows >= 100 launches and >= 20 ms, 3 per round"})
    for wl in args.workloads.split(","):
        run_workload(wl, capi, torch, args.rounds, emit)


if __name__ == "__main__":
    main()
