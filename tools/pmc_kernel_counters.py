#!/usr/bin/env python
"""Counters of named kernels from rocprofv3 --pmc counter_collection CSVs, restricted to the WORKLOAD launches (those of the
kernel's largest grid: bench.py first runs a tiny set-up scene through the same kernels), averaged per launch and summed over
the XCDs.  Several pass directories may be given; the result is one JSON object {kernel: {counter: value, "launches": n}}.
    python tools/pmc_kernel_counters.py out.json bin_count,bin_scatter <pass dir> [<pass dir> ...]"""
import csv
import glob
import json
import sys
from collections import defaultdict

out, names, dirs = sys.argv[1], sys.argv[2].split(","), sys.argv[3:]
res = {n: {} for n in names}
for d in dirs:
    rows = defaultdict(list)        # (kernel, counter) -> [(grid, dispatch, value)]
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for n in names:
                if n in r["Kernel_Name"]:
                    rows[(n, r["Counter_Name"])].append((int(r.get("Grid_Size", 0) or 0), r.get("Dispatch_Id") or len(rows[(n, r["Counter_Name"])]),
                                                         float(r["Counter_Value"])))
    for (n, c), ls in rows.items():
        big = max(g for g, _, _ in ls)
        per = defaultdict(float)
        for g, disp, v in ls:
            if g == big:
                per[disp] += v
        res[n][c] = round(sum(per.values()) / len(per), 1)
        res[n]["launches"] = len(per)
        res[n]["grid_threads"] = big
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
