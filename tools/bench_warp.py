"""What the warp stage costs and what it saves: per-launch time of the resize
launch ending in normalised bfloat16 CHW, the same launch with a 30 degree
rotation per image in front of the format, and the route a user has today.

  python tools/bench_warp.py [--rounds 3] [--out profiles/r11/warp_ab.jsonl]

bench.py's method (its C2 and C4 workloads, resident device sets and
launch_windows: device events around windows of >= 100 launches and >= 20 ms,
3 per round), every variant warmed first, the variants alternated in one
process for --rounds rounds (3 rounds: 9 windows each):

  a, a2   mxd_resize_crop_batch_fmt, bfloat16 CHW normalised (twice: the
          spread between the two is the spread the comparison is held to)
  b       mxd_resize_crop_batch_warp, MXD_WARP_BILINEAR, Pillow's 30 degree
          rotate matrix for every image, the same format
  c       as b with MXD_WARP_NEAREST (the 16.16 fixed-point path)
  t       as c with a fractional translate (the table path and warp_tab)
  d       what a user runs today: the u8 mxd_resize_crop_batch, then torch on
          the same stream -- affine_grid, grid_sample (bilinear, zeros), / 255,
          normalise, cast to bfloat16 (the result is CHW already)
  q, q2   as b with MXD_WARP_BICUBIC (warp_cubic.hip; twice, for its own spread)
  g       as q through the diagnostic build with warp_cubic.hip's LDS route off
          (make -C mlx-data_amd cubic_gather), loaded beside the product build
          as tools/lib_ab.py loads its variants; its output must equal q's
  e       as d with grid_sample(mode="bicubic"): another kernel (a = -0.75) and
          other bytes, the route a bicubic policy has without the mode

--variants picks a subset (a profiler run of the warp call alone: --variants b).

One JSON line per (workload, variant): median ms per launch over every window
of every round, min, max, the windows; then one summary line per workload."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "mlx-data_amd"))

import bench  # noqa: E402

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
FILL = (124, 116, 104)


def rotate_matrix(w, h, angle):
    """Pillow's Image.rotate matrix (expand=False, centre (w / 2, h / 2))."""
    r = -math.radians(angle % 360.0)
    c, s = round(math.cos(r), 15), round(math.sin(r), 15)
    cx, cy = w / 2.0, h / 2.0
    return (c, s, c * (-cx) + s * (-cy) + 0.0 + cx, -s, c, (-s) * (-cx) + c * (-cy) + 0.0 + cy)


def run_workload(name, capi, torch, rounds, emit, only):
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
    rot = rotate_matrix(cw, ch, 30.0)
    bilinear = capi.make_warps([(capi.MXD_WARP_BILINEAR, FILL, rot)] * B)
    nearest = capi.make_warps([(capi.MXD_WARP_NEAREST, FILL, rot)] * B)
    table = capi.make_warps([(capi.MXD_WARP_NEAREST, FILL, (1.0, 0.0, 20.5, 0.0, 1.0, -12.25))] * B)
    cubic = capi.make_warps([(capi.MXD_WARP_BICUBIC, FILL, rot)] * B)
    # the same rotation in affine_grid's normalised coordinates (square images: no aspect term)
    r = math.radians(30.0)
    theta = torch.tensor([[math.cos(r), math.sin(r), 0.0], [-math.sin(r), math.cos(r), 0.0]], device="cuda:0")
    theta = theta.unsqueeze(0).expand(B, 2, 3).contiguous()
    mean_t = torch.tensor(MEAN, device="cuda:0").view(1, 3, 1, 1)
    std_t = torch.tensor(STD, device="cuda:0").view(1, 3, 1, 1)

    def call(rc):
        if rc != 0:
            raise RuntimeError(L.mxd_last_error().decode())

    def a(i):
        call(L.mxd_resize_crop_batch_fmt(arrays["chw16"][i % 2], B, ctypes.byref(fmt), dev, hs))

    def warp_call(warps, lib=L):
        def f(i):
            if lib.mxd_resize_crop_batch_warp(arrays["chw16"][i % 2], warps, None, None, B, capi.MXD_U8, ctypes.byref(fmt),
                                              dev, hs) != 0:
                raise RuntimeError(lib.mxd_last_error().decode())
        return f

    def torch_route(mode):
        def f(i):
            call(L.mxd_resize_crop_batch(arrays["u8"][i % 2], B, capi.MXD_U8, dev, hs))
            with torch.cuda.stream(ext):
                x = u8s[i % 2].permute(0, 3, 1, 2).float()
                grid = F.affine_grid(theta, (B, C, ch, cw), align_corners=False)
                y = F.grid_sample(x, grid, mode=mode, padding_mode="zeros", align_corners=False)
                ((y / 255 - mean_t) / std_t).to(torch.bfloat16)
        return f

    every = {"a": a, "b": warp_call(bilinear), "c": warp_call(nearest), "t": warp_call(table), "d": torch_route("bilinear"),
             "q": warp_call(cubic), "e": torch_route("bicubic"), "a2": a, "q2": warp_call(cubic)}
    if not only or "g" in only:
        every["g"] = warp_call(cubic, gather_lib())
    variants = {k: f for k, f in every.items() if not only or k in only}
    try:
        if "q" in variants and "g" in variants:  # both routes give the same bytes
            variants["q"](0)
            stream.synchronize()
            ref = outs[0].view(torch.int16).cpu()
            outs[0].zero_()
            variants["g"](0)
            stream.synchronize()
            assert torch.equal(outs[0].view(torch.int16).cpu(), ref), "the gather build's output differs"
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
        def ratio(x, y):
            return round(med[x] / med[y], 4) if x in med and y in med else None

        summary = {"workload": name, "summary": True}
        if "a" in med and "a2" in med:
            med["lo"] = min(med["a"], med["a2"])
            summary["a_spread"] = round(abs(med["a"] - med["a2"]) / med["lo"], 4)
        if "q" in med and "q2" in med:
            summary["q_spread"] = round(abs(med["q"] - med["q2"]) / min(med["q"], med["q2"]), 4)
        for x, y in (("b", "lo"), ("c", "lo"), ("t", "lo"), ("q", "lo"), ("b", "d"), ("c", "d"), ("d", "b"), ("d", "c"),
                     ("q", "b"), ("e", "q"), ("g", "q")):
            if ratio(x, y) is not None:
                summary[f"{x}_over_{'a' if y == 'lo' else y}"] = ratio(x, y)
        emit(summary)
    finally:
        stream.synchronize()
        for src, dst, _, _ in sets:
            src.free()
            dst.free()
        stream.close()


def gather_lib():
    """The diagnostic build beside the product library (tools/lib_ab.py's way)."""
    path = os.path.join(REPO, "tools", "libmxd_amd_var_cubic_gather.so")
    G = ctypes.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    G.mxd_last_error.restype = ctypes.c_char_p
    if G.mxd_set_device(0) != 0:
        raise RuntimeError("cubic_gather: mxd_set_device failed")
    return G


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
