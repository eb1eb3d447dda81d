"""Per-launch time of the cubic filters against the triangle filter, in one
process on one box.

  python tools/bench_filter.py [--workloads c2,c4] [--parent tools/libmxd_amd_var_parent.so]
      [--out profiles/r08/filter_ab.jsonl]

For each workload (bench.py's inputs, two alternating source/output sets
resident in HBM) three variants are timed:

  a  the triangle launch of the parent commit's library, loaded beside this
     one as tools/lib_ab.py loads its variants (--parent; skipped without it)
  b  the triangle launch of this tree
  c  the Catmull-Rom launch of this tree (the same batch with filter = 1)

by bench.py's launch_windows method -- device events around windows of >= 100
launches and >= 20 ms -- with the variants alternating window by window, nine
windows each.  b runs the kernels a runs, so its median must sit inside a's own
window range; c is reported as a ratio to a (its algorithmic bytes are a's plus
a slightly wider footprint, so the ratio says how far the S = 4 kernels are
from the pace of the S = 2 ones).  One JSON line per workload.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "mlx-data_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402

import band_sweep  # noqa: E402
import bench  # noqa: E402

WINDOWS = 9


def with_filter(capi, imgs, n, filter):
    out = (capi.MxdImage * max(1, n))()
    ctypes.memmove(out, imgs, ctypes.sizeof(capi.MxdImage) * n)
    for i in range(n):
        out[i].filter = filter
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c4")
    ap.add_argument("--parent", default="", help="the parent commit's libmxd_amd.so (variant a)")
    ap.add_argument("--filter", default="catmullrom")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    for wl in args.workloads.split(","):
        capi, L, stream, sets, mode, alg, sizes, geoms, f32 = band_sweep.setup(wl)
        fid = capi.FILTERS[args.filter]
        cubic = [with_filter(capi, s[2], s[3], fid) for s in sets]
        variants = {}
        if args.parent:
            P = ctypes.CDLL(os.path.abspath(args.parent), mode=os.RTLD_LOCAL | os.RTLD_NOW)
            P.mxd_last_error.restype = ctypes.c_char_p
            if P.mxd_set_device(0) != 0:
                raise RuntimeError("parent library: mxd_set_device failed")
            variants["a_parent_triangle"] = (P, [s[2] for s in sets])
        variants["b_triangle"] = (L, [s[2] for s in sets])
        variants["c_" + args.filter] = (L, cubic)
        hs = ctypes.c_void_p(stream.handle)
        e0, e1 = capi.Event(), capi.Event()

        def launch(name, i):
            lib, imgs = variants[name]
            rc = lib.mxd_resize_crop_batch(imgs[i % 2], sets[i % 2][3], mode, 0, hs)
            if rc != 0:
                raise RuntimeError(name + ": " + lib.mxd_last_error().decode())

        def window(name, k):
            stream.synchronize()
            e0.record(stream)
            for i in range(k):
                launch(name, i)
            e1.record(stream)
            stream.synchronize()
            return e0.elapsed_ms(e1) / k

        # the triangle variants write the same bytes; the cubic one other bytes of the same shape
        outs = {}
        for name in variants:
            sets[0][1].memset(0, stream=stream)
            launch(name, 0)
            stream.synchronize()
            outs[name] = sets[0][1].download((sets[0][1].nbytes,), np.uint8, stream=stream)
        k = {}
        for name in variants:
            for i in range(20):
                launch(name, i)
            pilot = window(name, 10)
            k[name] = max(bench.MIN_WINDOW_LAUNCHES, int(bench.MIN_WINDOW_MS / max(pilot, 1e-4)) + 1)
            k[name] += k[name] % 2
        times = {name: [] for name in variants}
        for _ in range(WINDOWS):
            for name in variants:
                times[name].append(window(name, k[name]))
        rec = {"workload": wl, "filter": args.filter, "windows": WINDOWS, "alg_bytes_triangle": int(alg)}
        for name, t in times.items():
            rec[name] = {"ms_per_launch": round(statistics.median(t), 5), "min": round(min(t), 5),
                         "max": round(max(t), 5), "launches_per_window": k[name]}
        b, c = rec["b_triangle"], rec["c_" + args.filter]
        base = rec.get("a_parent_triangle", b)
        rec["cubic_over_triangle"] = round(c["ms_per_launch"] / base["ms_per_launch"], 4)
        rec["cubic_differs"] = bool(not np.array_equal(outs["b_triangle"], outs["c_" + args.filter]))
        if "a_parent_triangle" in rec:
            rec["b_equals_a_bytes"] = bool(np.array_equal(outs["a_parent_triangle"], outs["b_triangle"]))
            rec["b_inside_a_range"] = bool(base["min"] <= b["ms_per_launch"] <= base["max"])
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        for s in sets:
            s[0].free()
            s[1].free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
