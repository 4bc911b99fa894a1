#!/usr/bin/env python3
"""cstone_hip_knn (csrc/knn.hip) on the arrays of a synced single-rank domain: a uniform cloud in a periodic box and a
Plummer sphere, f32 coordinates, k = 32, 64 and 128.
  self      every particle asks for its k nearest others (query_self = its own index): n queries
  probes    --probes scattered points: drawn uniformly in the box, or at randomly chosen particles displaced by the local h
            (Plummer), so that they lie where the particles are

The yardstick is existing code on the same arrays: ONE counting walk of cstone_hip_find_neighbors (ngmax = 0) over all n
particles at the h that gives k neighbours on average (uniform: the sphere of k / n of the volume; Plummer: plummer_h at
ng = k).  It finds no order and no distances, and it shares one traversal among 64 targets.

Timed with events on the context's stream around the C entry alone, on outputs allocated beforehand; after one warm-up run
each, the cases ALTERNATE run by run and the median of --reps runs is reported beside every run.
  knn_ms, yardstick_ms      the calls
  ratio_per_query           (knn_ms / queries) / (yardstick_ms / n): time per query against time per target of the walk
  queries_per_s
One JSON line per cloud and k is appended to --out.  The number of particles tested per query is no output of the call;
it is not reported here."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cornerstone-octree_amd"))

import torch  # noqa: E402

import cstone_amd  # noqa: E402
from cstone_amd import clouds  # noqa: E402
from cstone_amd.domain import Domain  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def run(ctx, case, n, a):
    dev, rdt = "cuda", torch.float32
    if case == "uniform":
        x, y, z, h = clouds.uniform(n, dev, rdt, a.seed)
        lim, bc = [0.0, 1.0] * 3, (1, 1, 1)
    else:
        x, y, z, h, lim = clouds.make_cloud("plummer", n, n, dev, rdt, a.seed)
        bc = (0, 0, 0)
    dom = Domain(ctx, cstone_amd.HILBERT, 64, 32, a.bucket, a.bucket_focus, 0.5, cstone_amd.make_cbox(lim, bc))
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    scratch = [torch.empty(n, dtype=rdt, device=dev) for _ in range(3)]
    keys, x, y, z, h = dom.sync(keys, x, y, z, h, scratch)[:5]
    ctx.sync()
    v = dom.view()
    assert (v.start_index, v.end_index) == (0, n)
    gen = torch.Generator(device=dev).manual_seed(a.seed + 1)
    if case == "uniform":
        probes = torch.rand((a.probes, 3), dtype=rdt, device=dev, generator=gen)
    else:
        at = torch.randint(0, n, (a.probes,), device=dev, generator=gen)
        jitter = (torch.rand((a.probes, 3), dtype=rdt, device=dev, generator=gen) - 0.5) * h[at][:, None]
        probes = (torch.stack([x[at], y[at], z[at]], dim=1) + jitter).contiguous()
    own = torch.stack([x, y, z], dim=1).contiguous()
    me = torch.arange(n, dtype=torch.int32, device=dev)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    out = []
    for k in a.k:
        if case == "uniform":
            hk = torch.full((n,), 0.5 * (3.0 * k / (4.0 * math.pi * n)) ** (1.0 / 3.0), dtype=rdt, device=dev)  # 2h = radius
        else:
            hk = clouds.plummer_h(x, y, z, n, ng=float(k)).to(rdt)
        nb = torch.empty((n, k), dtype=torch.int32, device=dev)
        d2 = torch.empty((n, k), dtype=rdt, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        nc = torch.zeros(n, dtype=torch.int32, device=dev)

        def knn(qc, qself):
            ctx._chk(ctx.lib.cstone_hip_domain_knn(dom.h, P(x), P(y), P(z), P(qc), None, P(qself), qc.shape[0], k, P(nb), P(d2),
                                                   P(cnt)), "domain_knn")

        def walk():
            ctx._chk(ctx.lib.cstone_hip_find_neighbors(ctx.h, C.c_int(32), P(x), P(y), P(z), P(hk), C.c_uint32(0), C.c_uint32(n),
                                                       C.byref(v.box), C.c_void_p(v.child_offsets), C.c_void_p(v.internal_to_leaf),
                                                       C.c_void_p(v.layout), C.c_void_p(v.centers), C.c_void_p(v.sizes),
                                                       C.c_float(1.0), C.c_uint32(0), None, P(nc)), "find_neighbors")

        cases = dict(self=lambda: knn(own, me), probes=lambda: knn(probes, None), yardstick=walk)
        ms = {name: [] for name in cases}
        for fn in cases.values():
            fn()  # warm-up
        ctx.sync()
        for _ in range(a.reps):
            for name, fn in cases.items():  # alternating
                ms[name].append(timed(fn))
        mean_nc = float(nc.double().mean().item())
        yard = statistics.median(ms["yardstick"])
        res = dict(case=case, n=n, real_bits=32, k=k, bucket_focus=a.bucket_focus, yardstick_ms=yard, yardstick_ms_runs=ms["yardstick"],
                   yardstick_mean_neighbors=mean_nc)
        for name, queries in (("self", n), ("probes", a.probes)):
            t = statistics.median(ms[name])
            res[name] = dict(queries=queries, knn_ms=t, knn_ms_runs=ms[name], queries_per_s=queries / (t * 1e-3),
                             ratio_per_query=(t / queries) / (yard / n))
        out.append(res)
    ctx.sync()
    dom.close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=float, nargs="+", default=[1e6, 1e7])
    p.add_argument("--cases", nargs="+", default=["uniform", "plummer"])
    p.add_argument("--k", type=int, nargs="+", default=[32, 64, 128])
    p.add_argument("--probes", type=int, default=100000)
    p.add_argument("--bucket", type=int, default=1024)
    p.add_argument("--bucket-focus", type=int, default=64)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.jsonl"))
    a = p.parse_args()
    ctx = cstone_amd.Context(0)
    for n in a.n:
        for case in a.cases:
            for res in run(ctx, case, int(n), a):
                line = json.dumps(res)
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
