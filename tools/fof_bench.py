#!/usr/bin/env python3
"""cstone_hip_domain_fof (friends-of-friends groups, csrc/fof.hip) against one counting walk of cstone_hip_find_neighbors
(ngmax = 0, h = b / 2) on the same synced cloud in the same process: the walk is the floor of what the link pass can cost.

Cases: a uniform cloud in a periodic box at b = 0.2 x and 0.9 x the mean separation (the second is the union-heavy one:
just above the percolation threshold, one spanning group beside a broad spectrum of smaller ones), and a Plummer sphere
at b = 0.2 x the mean separation inside its half-mass radius.  Timed, steady state (one warm-up run, then --reps runs):
  walk_ms   the counting walk: host clock around the call and a synchronise; walk_stage_ms: its stage timer (events)
  link_ms   the link pass alone (the stage timer CSTONE_STAGE_FOF around the kernel that walks and unites)
  call_ms   the whole call with labels, group sizes and the number of groups: host clock, ends in the call's own
            synchronisation
  labels_ms the call with labels only (asynchronous; a synchronise behind it)
One JSON line per case is appended to --out."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cornerstone-octree_amd"))

import torch  # noqa: E402

import cstone_amd  # noqa: E402
from cstone_amd import clouds  # noqa: E402
from cstone_amd.domain import Domain  # noqa: E402


class Raw:
    """a device pointer of the domain view where the bindings expect a tensor"""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


def timed(ctx, fn, reps, stage):
    """(last result, host ms per run, stage ms per run); the first run warms up"""
    out, host, dev = None, [], []
    for _ in range(reps + 1):
        ctx.profile_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(ctx.profile_get(stage)[0])
    return out, host[1:], dev[1:]


def run(ctx, case, n, rb, a):
    dev, rdt = "cuda", (torch.float64 if rb == 64 else torch.float32)
    if case.startswith("uniform"):
        x, y, z, h = clouds.uniform(n, dev, rdt, a.seed)
        lim, bc = [0.0, 1.0] * 3, (1, 1, 1)
        b = float(case.split("-")[1]) * n ** (-1.0 / 3.0)
    else:
        x, y, z, h, lim = clouds.make_cloud("plummer", n, n, dev, rdt, a.seed)
        bc = (0, 0, 0)
        r_half = 1.3048 * 3.0 * math.pi / 16.0  # half-mass radius of the Plummer model of scale radius 3 pi / 16
        b = 0.2 * (4.0 / 3.0 * math.pi * r_half ** 3 / (0.5 * n)) ** (1.0 / 3.0)
    dom = Domain(ctx, cstone_amd.HILBERT, 64, rb, a.bucket, a.bucket_focus, 0.5, cstone_amd.make_cbox(lim, bc))
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    scratch = [torch.empty(n, dtype=rdt, device=dev) for _ in range(3)]
    keys, x, y, z, h, _, _ = dom.sync(keys, x, y, z, h, scratch)
    ctx.sync()
    v = dom.view()
    assert (v.start_index, v.end_index) == (0, n)
    tree = dict(child_offsets=Raw(v.child_offsets), internal_to_leaf=Raw(v.internal_to_leaf))
    layout, cen, siz = Raw(v.layout), Raw(v.centers), Raw(v.sizes)
    hw = torch.full((n,), 0.5 * b, dtype=rdt, device=dev)

    ctx.profile_enable(True)
    (_, counts), t_walk, s_walk = timed(
        ctx, lambda: ctx.find_neighbors(x, y, z, hw, 0, n, v.box, tree, layout, cen, siz, 0), a.reps, "neighbors")
    (labels, sizes, ng), t_call, s_link = timed(ctx, lambda: dom.fof(x, y, z, b), a.reps, "fof")
    first = labels.clone()
    _, t_labels, _ = timed(
        ctx, lambda: ctx.friends_of_friends(x, y, z, 0, n, v.box, tree, layout, cen, siz, b, want_sizes=False,
                                            want_num_groups=False), a.reps, "fof")
    ctx.profile_enable(False)
    ctx.sync()  # raises if a union gave up or the traversal stack overflowed
    med = statistics.median
    res = dict(case=case, n=n, real_bits=rb, linking_length=b, focus_leaves=v.num_focus_leaves,
               walk_ms=med(t_walk), walk_ms_runs=t_walk, walk_stage_ms=med(s_walk),
               link_ms=med(s_link), link_ms_runs=s_link, call_ms=med(t_call), call_ms_runs=t_call,
               labels_ms=med(t_labels), labels_ms_runs=t_labels,
               mean_neighbours=counts.double().mean().item(), groups=ng, largest_group=int(sizes.max().item()),
               in_groups_of_2_or_more=int((sizes > 1).sum().item()),
               repeatable=bool(torch.equal(first, dom.fof(x, y, z, b)[0])))
    res["link_over_walk"] = res["link_ms"] / res["walk_stage_ms"]
    res["call_over_walk"] = res["call_ms"] / res["walk_ms"]
    res["labels_over_walk"] = res["labels_ms"] / res["walk_ms"]
    res["particles_per_s_call"] = n / (res["call_ms"] * 1e-3)
    res["particles_per_s_link"] = n / (res["link_ms"] * 1e-3)
    dom.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=float, default=1e7)
    p.add_argument("--cases", nargs="+", default=["uniform-0.2", "uniform-0.9", "plummer"])
    p.add_argument("--real-bits", type=int, nargs="+", default=[64])
    p.add_argument("--bucket", type=int, default=1024)
    p.add_argument("--bucket-focus", type=int, default=64)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "fof_bench.jsonl"))
    a = p.parse_args()
    ctx = cstone_amd.Context(0)
    for case in a.cases:
        for rb in a.real_bits:
            res = run(ctx, case, int(a.n), rb, a)
            line = json.dumps(res)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
