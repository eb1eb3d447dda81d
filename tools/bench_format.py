"""What the fused formatted output buys: per-launch time of the resize launch
ending in each output form, against the second pass users run today.

  python tools/bench_format.py [--parent tools/libmxd_amd_var_parent.so] \
      [--rounds 3] [--out profiles/r07/format_ab.jsonl]

bench.py's method (its workloads, resident device sets and launch_windows:
device events around windows of >= 100 launches and >= 20 ms, median of 3),
every variant warmed first, the variants alternated in one process for
--rounds rounds.  On C2 (256 x 1280x960 -> 224^2):

  a         today's MXD_F32_DIV255 launch (this tree)
  a_parent  the same call from the parent commit's library (--parent; loaded
            beside the product like tools/lib_ab.py's variants): the spread of
            its rounds is the box's spread that `a` is held to
  b         float32 HWC normalised (mxd_resize_crop_batch_fmt)
  c         bfloat16 CHW normalised
  d         launch `a`, then torch's ((x - mean) / std).permute(0, 3, 1, 2)
            .to(torch.bfloat16).contiguous() on the device batch, on the same
            stream: what users run today
and a / c on C4's shapes.  One JSON line per (workload, variant): median ms
per launch over every window of every round, min, max, the windows."""
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


def run_workload(name, capi, torch, parent, rounds, emit):
    dev = 0
    L = capi.lib()
    B = bench.WORKLOADS[name]["batch"]
    sizes, geoms, _ = bench.make_workload(capi, name, B, 0)
    C, cw, ch = bench.C, 224, 224
    assert all(g[4] == cw and g[5] == ch for g in geoms)
    stream = capi.Stream(dev)
    hs = ctypes.c_void_p(stream.handle)
    # two resident source sets (bench layout); the batches are torch tensors, so
    # variant d's second pass reads what the launch wrote
    sets, _ = bench.device_sets(capi, dev, sizes, geoms, True, 2, 3000)
    ext = torch.cuda.ExternalStream(stream.handle, device=torch.device("cuda:0"))
    batches = [torch.empty((B, ch, cw, C), dtype=torch.float32, device="cuda:0") for _ in sets]
    arrays = {"f32": [], "chw16": []}
    for (src, dst, imgs, n), x in zip(sets, batches):
        for kind in arrays:
            arr = (capi.MxdImage * n)()
            ctypes.memmove(arr, imgs, ctypes.sizeof(arr))
            for i in range(n):
                arr[i].dst = x.data_ptr() + i * ch * cw * C * 4
                arr[i].dst_stride = cw * C * 4 if kind == "f32" else cw * 2
            arrays[kind].append(arr)
    fb = capi.make_out_format(capi.MXD_ELEM_F32, capi.MXD_LAYOUT_HWC, MEAN, STD)
    fc = capi.make_out_format(capi.MXD_ELEM_BF16, capi.MXD_LAYOUT_CHW, MEAN, STD, plane_stride=ch * cw * 2)
    mean_t = torch.tensor(MEAN, device="cuda:0")
    std_t = torch.tensor(STD, device="cuda:0")

    def call(lib, rc):
        if rc != 0:
            raise RuntimeError(lib.mxd_last_error().decode())

    def a(i, lib=L):
        call(lib, lib.mxd_resize_crop_batch(arrays["f32"][i % 2], B, capi.MXD_F32_DIV255, dev, hs))

    def b(i):
        call(L, L.mxd_resize_crop_batch_fmt(arrays["f32"][i % 2], B, ctypes.byref(fb), dev, hs))

    def c(i):
        call(L, L.mxd_resize_crop_batch_fmt(arrays["chw16"][i % 2], B, ctypes.byref(fc), dev, hs))

    def d(i):
        a(i)
        with torch.cuda.stream(ext):
            ((batches[i % 2] - mean_t) / std_t).permute(0, 3, 1, 2).to(torch.bfloat16).contiguous()

    variants = {"a": a}
    if parent is not None:
        variants["a_parent"] = lambda i: a(i, parent)
    if name == "c2":
        variants.update(b=b, c=c, d=d)
    else:
        variants.update(c=c)
    try:
        for f in variants.values():  # every shape and variant warmed first
            for i in range(10):
                f(i)
        stream.synchronize()
        windows = {k: [] for k in variants}
        for _ in range(rounds):
            for k, f in variants.items():
                windows[k] += bench.launch_windows(capi, stream, f, stream.synchronize)[2]
        for k, w in windows.items():
            emit({"workload": name, "variant": k, "images": B, "ms_per_launch": round(statistics.median(w), 5),
                  "min": min(w), "max": max(w), "windows": w})
    finally:
        stream.synchronize()
        for src, dst, _, _ in sets:
            src.free()
            dst.free()
        stream.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="the parent commit's libmxd_amd.so (variant a_parent)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--workloads", default="c2,c4")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # torch first: its HIP runtime is the one the libraries bind

    torch.zeros(1, device="cuda:0")
    from mlx_data_amd import capi

    capi.check(capi.lib().mxd_set_device(0))
    parent = None
    if args.parent:
        parent = ctypes.CDLL(os.path.abspath(args.parent), mode=os.RTLD_LOCAL | os.RTLD_NOW)
        parent.mxd_last_error.restype = ctypes.c_char_p
        if parent.mxd_set_device(0) != 0:
            raise RuntimeError("parent library: mxd_set_device failed")
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
        run_workload(wl, capi, torch, parent, args.rounds, emit)


if __name__ == "__main__":
    main()
