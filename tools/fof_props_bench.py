#!/usr/bin/env python3
"""cstone_hip_fof_group_properties (the group catalogue, csrc/fof_props.hip) on the clouds of tools/fof_bench.py: a uniform
cloud in a periodic box at b = 0.2 x the mean separation (hardly a link: as many groups as particles) and at 0.9 x (one
spanning group of most particles beside a broad spectrum of smaller ones), and a Plummer sphere.

Timed with events on the context's stream, medians of --reps runs after a warm-up run:
  props_ms    the property call alone, on a ready catalogue (mass, centre, velocity, radius, flags; f64 masses, velocities):
              the C entry itself on outputs allocated beforehand -- no allocation or fill lies between the two events
  catalog_ms  cstone_hip_fof_catalog through Context.fof_catalog, which allocates and zero-fills the two outputs (8 bytes per
              particle) inside the timed region; the call ends in its own synchronisation: host clock
  gather_ms   the yardstick: cstone_hip_gather_multi of x, y, z, m through `members` in the same process -- the floor for
              reading those bytes in that order (it also writes them, which the property call does not)
  mr_ms       cstone_hip_domain_mr_fof_catalog on a communicator of one rank (sort, runs, reduction, combine, finish; no
              collective), the C entry on outputs allocated beforehand, host clock; single_pair_ms = catalog_ms + props_ms
              is what it stands beside
Bytes per member of the property call: 4 (members) + 3 x 8 (x, y, z) + 8 (m) + 3 x 8 (v) = 60 gathered, plus the group's
reference and offsets (cached) and 36 + 4 bytes written per group.  One JSON line per case is appended to --out."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cornerstone-octree_amd"))

import ctypes as C  # noqa: E402

import torch  # noqa: E402

import cstone_amd  # noqa: E402
from cstone_amd import clouds  # noqa: E402
from cstone_amd.distributed import CommOps, NativeDistributedDomain  # noqa: E402
from cstone_amd.domain import Domain  # noqa: E402

PEAK_BYTES_PER_S = 8e12  # HBM3E of one MI355X


class OneRank:
    """the transport of a communicator of one rank: no collective is ever called"""

    rank, size, error = 0, 1, None

    def __init__(self):
        self.ops = CommOps()


def event_ms(fn, reps):
    """(last result, device ms per run by events on the current stream); the first run warms up"""
    out, ms = None, []
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return out, ms[1:]


def host_ms(fn, reps):
    out, ms = None, []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms[1:]


def run(ctx, case, n, a):
    dev, rdt = "cuda", torch.float64
    if case.startswith("uniform"):
        x, y, z, h = clouds.uniform(n, dev, rdt, a.seed)
        lim, bc = [0.0, 1.0] * 3, (1, 1, 1)
        b = float(case.split("-")[1]) * n ** (-1.0 / 3.0)
    else:
        x, y, z, h, lim = clouds.make_cloud("plummer", n, n, dev, rdt, a.seed)
        bc = (0, 0, 0)
        r_half = 1.3048 * 3.0 * math.pi / 16.0
        b = 0.2 * (4.0 / 3.0 * math.pi * r_half ** 3 / (0.5 * n)) ** (1.0 / 3.0)
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    m = 0.5 + torch.rand(n, dtype=rdt, device=dev, generator=gen)
    vel = [2 * torch.rand(n, dtype=rdt, device=dev, generator=gen) - 1 for _ in range(3)]
    dom = Domain(ctx, cstone_amd.HILBERT, 64, 64, a.bucket, a.bucket_focus, 0.5, cstone_amd.make_cbox(lim, bc))
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    scratch = [torch.empty(n, dtype=rdt, device=dev) for _ in range(3)]
    out = dom.sync(keys, x, y, z, h, scratch, props=[m] + vel)
    keys, x, y, z, h = out[:5]
    m, vx, vy, vz = out[-1]
    ctx.sync()
    v = dom.view()
    assert (v.start_index, v.end_index) == (0, n)
    labels, sizes, ng = dom.fof(x, y, z, b)

    (off, mem), t_cat = host_ms(lambda: ctx.fof_catalog(labels, 0, n, 1), a.reps)
    G = off.numel() - 1
    props = [torch.zeros(G, dtype=rdt, device=dev), torch.zeros((G, 3), dtype=rdt, device=dev),
             torch.zeros((G, 3), dtype=rdt, device=dev), torch.zeros(G, dtype=rdt, device=dev),
             torch.zeros(G, dtype=torch.int32, device=dev)]
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def properties():
        ctx._chk(ctx.lib.cstone_hip_fof_group_properties(
            ctx.h, 64, 64, P(x), P(y), P(z), P(m), P(vx), P(vy), P(vz), C.cast(C.byref(v.box), C.c_void_p), P(off), P(mem), G,
            *[P(t) for t in props]), "fof_group_properties")

    _, t_props = event_ms(properties, a.reps)
    ctx.sync()
    first = [t.clone() for t in props]
    for t in props:
        t.zero_()
    properties()
    ctx.sync()
    again = props
    props = first
    dst = [torch.empty(n, dtype=rdt, device=dev) for _ in range(4)]
    sp = (C.c_void_p * 4)(*[t.data_ptr() for t in (x, y, z, m)])
    dp = (C.c_void_p * 4)(*[t.data_ptr() for t in dst])

    def gather():
        ctx._chk(ctx.lib.cstone_hip_gather_multi(ctx.h, C.c_int(8), C.c_void_p(mem.data_ptr()), C.c_size_t(n), sp, dp,
                                                 C.c_int(4)), "gather_multi")

    _, t_gather = event_ms(gather, a.reps)

    # the multi-rank call on a communicator of one rank
    mr = NativeDistributedDomain(ctx, cstone_amd.HILBERT, 64, 64, a.bucket, a.bucket_focus, lim, bc, coll=OneRank())
    r = mr.sync(x.clone(), y.clone(), z.clone(), torch.full((n,), 0.6 * b, dtype=rdt, device=dev), props=[m, vx, vy, vz])
    ctx.sync()
    gl, _, _, _ = mr.fof(r["x"], r["y"], r["z"], b, want_sizes=False)
    pm, pv = r["props"][0].clone(), [p.clone() for p in r["props"][1:4]]
    table = [torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
             torch.zeros(n, dtype=rdt, device=dev), torch.zeros((n, 3), dtype=rdt, device=dev),
             torch.zeros((n, 3), dtype=rdt, device=dev), torch.zeros(n, dtype=rdt, device=dev),
             torch.zeros(n, dtype=torch.int32, device=dev)]
    listed = C.c_uint32(0)

    def catalogue():
        ctx._chk(ctx.lib.cstone_hip_domain_mr_fof_catalog(
            mr.h, P(r["x"]), P(r["y"]), P(r["z"]), P(pm), 64, P(pv[0]), P(pv[1]), P(pv[2]), P(gl), 1, n,
            *[P(t) for t in table], C.byref(listed)), "domain_mr_fof_catalog")

    _, t_mr = host_ms(catalogue, a.reps)
    ctx.sync()
    same = bool(torch.equal(r["x"], x)) and listed.value == G and all(torch.equal(table[2 + i][:G], props[i]) for i in range(5))
    mr.close()

    med = statistics.median
    res = dict(case=case, n=n, real_bits=64, mass_bits=64, linking_length=b, groups=ng, largest_group=int(sizes.max().item()),
               props_ms=med(t_props), props_ms_runs=t_props, catalog_ms=med(t_cat), catalog_ms_runs=t_cat,
               gather_ms=med(t_gather), gather_ms_runs=t_gather, mr_ms=med(t_mr), mr_ms_runs=t_mr,
               repeatable=all(torch.equal(p, q) for p, q in zip(props, again)), mr_equals_single_bits=same)
    res["props_over_gather"] = res["props_ms"] / res["gather_ms"]
    res["gathered_bytes_per_member"] = 60
    res["props_fraction_of_peak"] = 60.0 * n / (res["props_ms"] * 1e-3) / PEAK_BYTES_PER_S
    res["members_per_s"] = n / (res["props_ms"] * 1e-3)
    res["single_pair_ms"] = res["catalog_ms"] + res["props_ms"]
    res["mr_over_single_pair"] = res["mr_ms"] / res["single_pair_ms"]
    dom.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=float, default=1e7)
    p.add_argument("--cases", nargs="+", default=["uniform-0.2", "uniform-0.9", "plummer"])
    p.add_argument("--bucket", type=int, default=1024)
    p.add_argument("--bucket-focus", type=int, default=64)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "fof_props_bench.jsonl"))
    a = p.parse_args()
    ctx = cstone_amd.Context(0)
    for case in a.cases:
        res = run(ctx, case, int(a.n), a)
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
