#!/usr/bin/env python3
"""Where the kernels of one steady re-sorted sync lie, from a rocprofv3 --kernel-trace of `python bench.py --steps 5
--warmup 2`, and what the mover bins move, from --pmc FETCH_SIZE / --pmc WRITE_SIZE passes over the same command:

python tools/resort_timeline.py <tag> <trace dir> [<FETCH_SIZE dir> <WRITE_SIZE dir>] [out.json]

The sync is the last one of the trace whose gather of h is in it, taken from the first of the library's kernels behind the
caller's own (torch's) kernels to the last one before them.  Times are relative to the sync's first kernel."""
import csv
import glob
import json
import os
import re
import sys
from statistics import median

tag, trace_dir = sys.argv[1], sys.argv[2]
rest = sys.argv[3:]
out_path = rest.pop() if rest and rest[-1].endswith(".json") else None
OURS = re.compile(r"\b([A-Za-z]\w*Kernel)\b")


def short(name):
    """the library's kernels by their short names; None for the caller's (torch's) kernels between two syncs"""
    if "at::" in name or "c10::" in name:
        return None
    m = OURS.search(name)
    return m.group(1) if m else name[:40]


def find(d, what):
    hits = glob.glob(os.path.join(d, "**", f"*{what}.csv"), recursive=True)
    if not hits:
        raise SystemExit(f"no *{what}.csv under {d}")
    return hits[0]


rows = []
for r in csv.DictReader(open(find(trace_dir, "kernel_trace"))):
    rows.append(dict(name=short(r["Kernel_Name"]), t0=int(r["Start_Timestamp"]), t1=int(r["End_Timestamp"]),
                     queue=r.get("Queue_Id", "?")))
rows.sort(key=lambda r: r["t0"])
enc = [i for i, r in enumerate(rows) if r["name"] == "encodeResortKernel"]
gath = [i for i, r in enumerate(rows) if r["name"] == "gatherHaloRadiiKernel"]
e = max(i for i in enc if any(g > i for g in gath))
begin = e
while begin > 0 and rows[begin - 1]["name"]:
    begin -= 1
stop = e
while stop + 1 < len(rows) and rows[stop + 1]["name"]:
    stop += 1
sync = rows[begin:stop + 1]
origin = sync[0]["t0"]
for r in sync:
    print(f"{(r['t0'] - origin) / 1e3:9.1f} us  +{(r['t1'] - r['t0']) / 1e3:8.1f} us  q{r['queue']:>3}  {r['name']}")


def at(names, which):
    hits = [r for r in sync if r["name"] in names]
    if not hits:
        return None
    return ((min(r["t0"] for r in hits) if which == "start" else max(r["t1"] for r in hits)) - origin) / 1e3


LEAF = ("leafSortWaveKernel", "leafSortKernel")
TABLE = ("leafStartWordsKernel", "fillCompactLeavesKernel", "coarseLeafTableKernel")
PLACE = ("placeMoversKernel",)
summary = {
    "setting": tag,
    "encode_start_us": at(("encodeResortKernel",), "start"),
    "bin_movers_start_us": at(("binMoversKernel",), "start"),
    "place_movers_start_us": at(PLACE, "start"),
    "leaf_pass_start_us": at(LEAF, "start"),
    "leaf_pass_end_us": at(LEAF, "end"),
    "gather_h_end_us": at(("gatherHaloRadiiKernel",), "end"),
    "leaf_table_first_start_us": at(TABLE, "start"),
    "leaf_table_last_end_us": at(TABLE, "end"),
    "last_kernel_end_us": (max(r["t1"] for r in sync) - origin) / 1e3,
    "last_kernel_without_table_end_us": (max(r["t1"] for r in sync if r["name"] not in TABLE) - origin) / 1e3,
    "sync_kernels": len(sync),
}
if len(rest) >= 2:
    # bytes per mover of the two bin kernels: 2 x FETCH_SIZE (gfx950 reports half of what is read) + WRITE_SIZE, KiB units
    counters = {}
    for name, d in zip(("FETCH_SIZE", "WRITE_SIZE"), rest[:2]):
        per = {}
        for r in csv.DictReader(open(find(d, "counter_collection"))):
            k = short(r["Kernel_Name"])
            if k in ("binMoversKernel",) + PLACE and r["Counter_Name"] == name:
                per.setdefault(k, []).append(float(r["Counter_Value"]))
        counters[name] = {k: median(v[1:] or v) for k, v in per.items()}  # (not the first launch: a cold table)
    movers = float(os.environ.get("RESORT_TIMELINE_MOVERS", "0"))
    summary["movers"] = movers
    for k in counters["FETCH_SIZE"]:
        b = 2.0 * 1024 * counters["FETCH_SIZE"][k] + 1024 * counters["WRITE_SIZE"].get(k, 0.0)
        summary[f"{k}_hbm_bytes"] = b
        if movers:
            summary[f"{k}_bytes_per_mover"] = b / movers
print(json.dumps(summary))
if out_path:
    json.dump(summary, open(out_path, "w"), indent=1)
