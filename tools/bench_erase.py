"""What Random Erasing costs inside the batch call and what it saves: per-launch
time of the resize launch ending in normalised bfloat16 CHW, the same batch
through the erase call, and the route a user has today.

  python tools/bench_erase.py [--rounds 3] [--out profiles/r16/erase_ab.jsonl]

bench.py's method (its C2 and C4 workloads, resident device sets and
launch_windows: device events around windows of >= 100 launches and >= 20 ms,
3 per round), every variant warmed first, the variants alternated in one
process for --rounds rounds (3 rounds: 9 windows each).  Fill rule: every image
is erased with one 94 x 94 box (0.175 H W, the mean of timm's area range) at a
place of its own; the recipes' prob = 0.25 would do a quarter of this work.

  a, a2   mxd_resize_crop_batch_fmt, bfloat16 CHW normalised (twice: the
          spread between the two is the spread the comparison is held to)
  b       mxd_resize_crop_batch_erase, MXD_ERASE_PIXEL, the same format
  bc      as b with MXD_ERASE_CONST
  n       as b with every count 0 (no erase launch: the call's fixed cost)
  c       what a user runs today: the formatted launch, then timm's
          RandomErasing loop in torch on the same stream -- per image a slice
          and a normal_() of the box

--variants picks a subset.  --lib times another build of the library.

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
SIDE = 94  # 94 * 94 = 8836, 0.176 of 224 * 224


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
    outs = [torch.empty((B, C, ch, cw), dtype=torch.bfloat16, device="cuda:0") for _ in sets]
    arrays = []
    for (src, dst, imgs, n), y in zip(sets, outs):
        arr = (capi.MxdImage * n)()
        ctypes.memmove(arr, imgs, ctypes.sizeof(arr))
        for i in range(n):
            arr[i].dst = y.data_ptr() + i * C * ch * cw * 2
            arr[i].dst_stride = cw * 2
        arrays.append(arr)
    fmt = capi.make_out_format(capi.MXD_ELEM_BF16, capi.MXD_LAYOUT_CHW, MEAN, STD, plane_stride=ch * cw * 2)
    places = [((i * 53) % (cw - SIDE), (i * 37) % (ch - SIDE)) for i in range(B)]
    boxes = [[(x, y, x + SIDE, y + SIDE)] for x, y in places]
    pixel = capi.make_erases([(capi.MXD_ERASE_PIXEL, bx, (1000 + i, 7)) for i, bx in enumerate(boxes)])
    const = capi.make_erases([(capi.MXD_ERASE_CONST, bx, None, 0.0) for bx in boxes])
    none = capi.make_erases([None] * B)

    def call(rc):
        if rc != 0:
            raise RuntimeError(L.mxd_last_error().decode())

    def a(i):
        call(L.mxd_resize_crop_batch_fmt(arrays[i % 2], B, ctypes.byref(fmt), dev, hs))

    def erase_call(erases):
        def f(i):
            call(L.mxd_resize_crop_batch_erase(arrays[i % 2], None, None, None, None, None, erases, B, capi.MXD_U8,
                                               ctypes.byref(fmt), dev, hs))
        return f

    def c(i):
        a(i)
        with torch.cuda.stream(ext):
            y = outs[i % 2]
            for k, (left, top) in enumerate(places):  # timm.data.RandomErasing._erase, mode 'pixel'
                y[k, :, top:top + SIDE, left:left + SIDE] = torch.empty((C, SIDE, SIDE), dtype=y.dtype,
                                                                        device=y.device).normal_()

    every = {"a": a, "b": erase_call(pixel), "bc": erase_call(const), "n": erase_call(none), "c": c, "a2": a}
    variants = {k: f for k, f in every.items() if not only or k in only}
    try:
        for f in variants.values():  # every shape and variant warmed first
            for i in range(4):
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
            spread = abs(med["a"] - med["a2"])
            emit({"workload": name, "summary": True, "fill": "one 94 x 94 box in every image (0.175 H W; prob 0.25 does a quarter)",
                  "b_over_a": round(med["b"] / lo, 4), "bc_over_a": round(med["bc"] / lo, 4),
                  "n_over_a": round(med["n"] / lo, 4), "c_over_b": round(med["c"] / med["b"], 2),
                  "a_spread": round(spread / lo, 4),
                  "b_max_below_c_min_by_more_than_a_spread": min(windows["c"]) - max(windows["b"]) > spread})
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
