#!/usr/bin/env python3
"""cstone_hip_domain_mr_fof (friends-of-friends with global labels, csrc/domain_mr.hip) on a communicator of ONE rank
against cstone_hip_domain_fof, the single-rank call, on the same cloud in the same process.  With one rank no collective
is made and the two find the same groups, so the difference is what the multi-rank call adds on the device and the host:
the id pass, two lowering passes with their read-backs, the 64-bit copies, and -- with sizes -- the size protocol (count,
compaction, a 64-bit sort of one pair per group, two passes at the owner, the scatter).

Cases: a uniform cloud in a periodic box at b = 0.2 x and 0.9 x the mean separation, h = 0.6 b.  Timed, steady state (one
warm-up run, then --reps runs, host clock around the call and a synchronise), alternating the three calls run by run:
  single_ms     cstone_hip_domain_fof with labels, sizes and the number of groups
  mr_ms         cstone_hip_domain_mr_fof with labels, sizes, the number of groups and of rounds
  mr_labels_ms  the same without sizes
One JSON line per case is appended to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cornerstone-octree_amd"))

import torch  # noqa: E402

import cstone_amd  # noqa: E402
from cstone_amd import clouds  # noqa: E402
from cstone_amd.distributed import CommOps, NativeDistributedDomain  # noqa: E402
from cstone_amd.domain import Domain  # noqa: E402


class OneRank:
    """the transport of a communicator of one rank: no collective is ever called"""

    rank, size, error = 0, 1, None

    def __init__(self):
        self.ops = CommOps()


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def run(ctx, case, n, rb, a):
    dev, rdt = "cuda", (torch.float64 if rb == 64 else torch.float32)
    x, y, z, _ = clouds.uniform(n, dev, rdt, a.seed)
    lim, bc = [0.0, 1.0] * 3, (1, 1, 1)
    b = float(case.split("-")[1]) * n ** (-1.0 / 3.0)
    h = torch.full((n,), 0.6 * b, dtype=rdt, device=dev)

    single = Domain(ctx, cstone_amd.HILBERT, 64, rb, a.bucket, a.bucket_focus, 0.5, cstone_amd.make_cbox(lim, bc))
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    scratch = [torch.empty(n, dtype=rdt, device=dev) for _ in range(3)]
    _, sx, sy, sz, _, _, _ = single.sync(keys, x.clone(), y.clone(), z.clone(), h.clone(), scratch)
    mr = NativeDistributedDomain(ctx, cstone_amd.HILBERT, 64, rb, a.bucket, a.bucket_focus, lim, bc, coll=OneRank())
    r = mr.sync(x, y, z, h)
    ctx.sync()
    assert (r["start"], r["end"]) == (0, n) and torch.equal(r["x"], sx)

    calls = dict(single=lambda: single.fof(sx, sy, sz, b), mr=lambda: mr.fof(r["x"], r["y"], r["z"], b),
                 mr_labels=lambda: mr.fof(r["x"], r["y"], r["z"], b, want_sizes=False))
    times, last = {k: [] for k in calls}, {}
    for rep in range(a.reps + 1):  # (the first run of each warms up)
        for k, fn in calls.items():
            last[k], ms = clock(fn)
            if rep:
                times[k].append(ms)
    ctx.sync()
    l1, s1, g1 = last["single"]
    labels, sizes, groups, rounds = last["mr"]
    same = bool(torch.equal(labels, l1.long() & 0xFFFFFFFF) and torch.equal(sizes, s1.long() & 0xFFFFFFFF) and groups == g1 and
                torch.equal(labels, last["mr_labels"][0]))
    med = statistics.median
    res = dict(case=case, n=n, real_bits=rb, linking_length=b, ranks=1, rounds=rounds, groups=groups,
               largest_group=int(sizes.max().item()), same_as_single_rank=same,
               single_ms=med(times["single"]), single_ms_runs=times["single"], mr_ms=med(times["mr"]), mr_ms_runs=times["mr"],
               mr_labels_ms=med(times["mr_labels"]), mr_labels_ms_runs=times["mr_labels"])
    res["mr_over_single"] = res["mr_ms"] / res["single_ms"]
    res["mr_labels_over_single"] = res["mr_labels_ms"] / res["single_ms"]
    single.close()
    mr.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=float, default=1e7)
    p.add_argument("--cases", nargs="+", default=["uniform-0.2", "uniform-0.9"])
    p.add_argument("--real-bits", type=int, nargs="+", default=[64])
    p.add_argument("--bucket", type=int, default=1024)
    p.add_argument("--bucket-focus", type=int, default=64)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "fof_mr_bench.jsonl"))
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
