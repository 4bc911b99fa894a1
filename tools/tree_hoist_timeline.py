#!/usr/bin/env python3
"""the last steady sync in a rocprofv3 --kernel-trace of `python bench.py --steps 5 --warmup 2`, as a timeline:
python tools/tree_hoist_timeline.py <dir with *kernel_trace.csv> <tag> [out.json]
prints every kernel of that sync (start relative to its first kernel, duration, queue) and where the kernels of the
linked-octree build lie relative to the mover bins, the leaf pass and the gather of h"""
import csv
import glob
import json
import os
import re
import sys

src, tag = sys.argv[1], sys.argv[2]
path = glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True)[0]
rows = []
for r in csv.DictReader(open(path)):
    m = re.search(r"(\w+Kernel)\b", r["Kernel_Name"])
    rows.append(dict(name=m.group(1) if m else r["Kernel_Name"][:40], t0=int(r["Start_Timestamp"]),
                     t1=int(r["End_Timestamp"]), queue=r.get("Queue_Id", "?")))
rows.sort(key=lambda r: r["t0"])


def last(name, before=None):
    return max(i for i, r in enumerate(rows) if r["name"] == name and (before is None or i < before))


end = last("gatherHaloRadiiKernel")
begin = last("leafStartWordsKernel", end)
# (the node ops of a hoisted sync start on the tree stream before the leaf-table prepare: take them in)
OPS = ("focusOpsKernel", "protectAncestorsKernel", "leafOpsKernel", "blockSumKernel", "blockScanKernel", "scanSumsKernel",
       "smallCopyKernel")
while begin > 0 and rows[begin - 1]["name"] in OPS and rows[begin]["t0"] - rows[begin - 1]["t0"] < 200_000:
    begin -= 1
stop = end
while stop + 1 < len(rows) and rows[stop + 1]["t0"] - rows[end]["t1"] < 1_500_000 and rows[stop + 1]["name"] != "fillCompactLeavesKernel":
    stop += 1
sync = rows[begin:stop + 1]
origin = sync[0]["t0"]
for r in sync:
    print(f"{(r['t0'] - origin) / 1e3:9.1f} us  +{(r['t1'] - r['t0']) / 1e3:8.1f} us  q{r['queue']:>3}  {r['name']}")


def span(name, which):
    hits = [r for r in sync if r["name"] == name]
    return None if not hits else (min(r["t0"] for r in hits) if which == "start" else max(r["t1"] for r in hits)) - origin


link = [r for r in sync if r["name"] in ("unsortedLayoutKernel", "invertOrderKernel", "linkKernel")]
summary = {
    "setting": tag,
    "bin_movers_start_us": span("binMoversKernel", "start") / 1e3,
    "leaf_pass_end_us": span("leafSortWaveKernel", "end") / 1e3,
    "link_octree_first_start_us": min(r["t0"] for r in link) / 1e3 - origin / 1e3 if link else None,
    "link_octree_last_end_us": max(r["t1"] for r in link) / 1e3 - origin / 1e3 if link else None,
    "rebalance_start_us": (span("rebalanceKernel", "start") or 0) / 1e3,
    "gather_h_start_us": span("gatherHaloRadiiKernel", "start") / 1e3,
    "leaf_pass_end_to_gather_h_start_us": (span("gatherHaloRadiiKernel", "start") - span("leafSortWaveKernel", "end")) / 1e3,
    "sync_kernels": len(sync),
    "first_to_last_kernel_us": (max(r["t1"] for r in sync) - origin) / 1e3,
}
print(json.dumps(summary))
if len(sys.argv) > 3:
    json.dump(summary, open(sys.argv[3], "w"), indent=1)
