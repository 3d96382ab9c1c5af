"""Developer tool: per-shape device times of the attention kernels from a rocprofv3 --kernel-trace csv.  One template serves
several shapes (self- and cross-attention), so launches are grouped by kernel name AND grid:
  rocprofv3 --kernel-trace -d DIR -o k --output-format csv -- python tools/attn_micro.py ...;  python tools/attn_kernel_times.py DIR [skip]
`skip` leading launches of each group are dropped as warm-up (default 1)."""
import csv
import glob
import os
import sys
from collections import defaultdict

path = sys.argv[1]
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 1
files = [path] if os.path.isfile(path) else glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
groups = defaultdict(list)
for f in files:
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        if "attn_" not in name:
            continue
        short = name[name.index("attn_"):].split("(")[0]
        wg = int(r["Workgroup_Size_X"])
        grid = tuple(int(r[f"Grid_Size_{a}"]) // (wg if a == "X" else 1) for a in "XYZ")
        groups[(short, grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for (short, grid), ts in sorted(groups.items()):
    ts = ts[skip:] or ts
    ts.sort()
    print(f"{short:44s} grid {str(grid):18s} n {len(ts):4d}  median {ts[len(ts) // 2]:8.1f} us  min {ts[0]:8.1f}  max {ts[-1]:8.1f}")
