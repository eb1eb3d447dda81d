"""What the mix stage costs and what it saves: per-launch time of the resize
launch ending in normalised bfloat16 CHW, the same batch through the mix call
(MixUp, CutMix), and the route a user has today.

  python tools/bench_mix.py [--rounds 3] [--out profiles/r14/mix_ab.jsonl]

bench.py's method (its C2 and C4 workloads, resident device sets and
launch_windows: device events around windows of >= 100 launches and >= 20 ms,
3 per round), every variant warmed first, the variants alternated in one
process for --rounds rounds (3 rounds: 9 windows each):

  a, a2   mxd_resize_crop_batch_fmt, bfloat16 CHW normalised (twice: the
          spread between the two is the spread the comparison is held to)
  b       mxd_resize_crop_batch_mix, MXD_MIX_MIXUP with lam 0.3 for every image
          and the partner n - 1 - i, the same format
  bc      as b with MXD_MIX_CUTMIX, a centred box of half the window's sides
  n       as b with MXD_MIX_NONE (the stage as a formatting copy: its fixed cost)
  c       what a user runs today: the u8 mxd_resize_crop_batch, then torch on
          the same stream -- flip, two float multiplies, add, round, / 255,
          normalise, permute and cast to bfloat16

--variants picks a subset (a profiler run of the mix call alone: --variants b).
--lib times another build of the library.

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
LAM = 0.3


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
    mixup = capi.make_mixes([capi.mixup(B - 1 - i, LAM) for i in range(B)])
    cutmix = capi.make_mixes([capi.cutmix(B - 1 - i, cw // 4, ch // 4, cw - cw // 4, ch - ch // 4) for i in range(B)])
    none = capi.make_mixes([(capi.MXD_MIX_NONE,)] * B)
    mean_t = torch.tensor(MEAN, device="cuda:0").view(1, 3, 1, 1)
    std_t = torch.tensor(STD, device="cuda:0").view(1, 3, 1, 1)

    def call(rc):
        if rc != 0:
            raise RuntimeError(L.mxd_last_error().decode())

    def a(i):
        call(L.mxd_resize_crop_batch_fmt(arrays["chw16"][i % 2], B, ctypes.byref(fmt), dev, hs))

    def mix_call(mixes):
        def f(i):
            call(L.mxd_resize_crop_batch_mix(arrays["chw16"][i % 2], None, None, None, None, mixes, B, capi.MXD_U8,
                                             ctypes.byref(fmt), dev, hs))
        return f

    def c(i):
        call(L.mxd_resize_crop_batch(arrays["u8"][i % 2], B, capi.MXD_U8, dev, hs))
        with torch.cuda.stream(ext):
            x = u8s[i % 2]
            mixed = torch.round(x.float() * LAM + x.flip(0).float() * (1 - LAM))
            ((mixed.permute(0, 3, 1, 2) / 255 - mean_t) / std_t).to(torch.bfloat16)

    every = {"a": a, "b": mix_call(mixup), "bc": mix_call(cutmix), "n": mix_call(none), "c": c, "a2": a}
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
        if not only:
            lo = min(med["a"], med["a2"])
            emit({"workload": name, "summary": True, "b_over_a": round(med["b"] / lo, 4), "bc_over_a": round(med["bc"] / lo, 4),
                  "n_over_a": round(med["n"] / lo, 4), "c_over_b": round(med["c"] / med["b"], 2),
                  "c_over_bc": round(med["c"] / med["bc"], 2), "a_spread": round(abs(med["a"] - med["a2"]) / lo, 4),
                  "b_max_below_c_min": max(windows["b"]) < min(windows["c"])})
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
