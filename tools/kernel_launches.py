"""Kernel name, grid, workgroup -> dispatch count, from a rocprofv3 --kernel-trace CSV directory."""
import collections
import csv
import glob
import os
import sys

src, dst = sys.argv[1], sys.argv[2]
files = glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True)
assert files, "no kernel trace under " + src
counts = collections.Counter()
for f in files:
    with open(f, newline="") as fh:
        for row in csv.DictReader(fh):
            r = {k.lower(): v for k, v in row.items()}
            grid = "x".join(r.get("grid_size_" + a, r.get("grid_size", "?")) for a in "xyz")
            wg = "x".join(r.get("workgroup_size_" + a, r.get("workgroup_size", "?")) for a in "xyz")
            counts[(r["kernel_name"], grid, wg)] += 1
with open(dst, "w", newline="") as fh:
    w = csv.writer(fh)
    w.writerow(["kernel", "grid", "workgroup", "dispatches"])
    for (name, grid, wg), c in sorted(counts.items()):
        w.writerow([name, grid, wg, c])
print(dst, len(counts), "rows,", sum(counts.values()), "dispatches")
