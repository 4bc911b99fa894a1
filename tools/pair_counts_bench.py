#!/usr/bin/env python3
"""cstone_hip_pair_counts and cstone_hip_pair_counts_cross (csrc/pair_counts.hip) on the clouds of
tools/sphere_profiles_bench.py: a uniform cloud in a periodic box and a Plummer sphere in an open one, f64 coordinates and
f64 weights.  The outer edge is chosen for about --partners partners per particle at the mean density (uniform) or at the
mean density inside the half-mass radius (Plummer); the edges are logarithmic over two decades below it.

Timed with events on the context's stream around the C entry alone, on outputs allocated beforehand.  The configurations
of one cloud -- NB = 16 and 64, with and without weights, every outer edge -- ALTERNATE run by run after one warm-up run
each, and every run is kept beside the median.
  ms                 the call
  pairs_per_s        ordered pairs binned / time
  tests_per_pair     distance tests issued / pairs binned (the call's stats, read in a run of its own that is not timed):
                     the price of sharing one traversal among 64 targets
Yardsticks, code that existed before, in the same session (--yardstick-n particles at most):
  sphere_rows        cstone_hip_domain_sphere_profiles with every particle as a query at scale 1, rows summed: the only way
                     to DD(r) before (it also counts the particle itself, at d2 = 0)
  neighbors_stats    cstone_hip_find_neighbors_stats with 2 h = the outer edge: a shared traversal that bins nothing
Cross counts: --cross-queries random points as targets -- uniform in the box, or a second realisation of the Plummer
sphere --, NB = 16, no weights.  encode_sort_ms is cstone_hip_compute_sfc_keys plus cstone_hip_sort_pairs on as many points
through the public entries (allocations of the outputs included): the share of the call's encode and sort, from above;
its split and gather kernels (two passes over the queries) are not in it.
One JSON line per cloud is appended to --out."""
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


def log_edges(nb, inner, outer):
    return [inner * (outer / inner) ** (k / nb) for k in range(nb + 1)]


def run(ctx, case, n, a):
    dev, rdt = "cuda", torch.float64
    if case == "uniform":
        x, y, z, h = clouds.uniform(n, dev, rdt, a.seed)
        lim, bc = [0.0, 1.0] * 3, (1, 1, 1)
        density = float(n)
    else:
        x, y, z, h, lim = clouds.make_cloud("plummer", n, n, dev, rdt, a.seed)
        bc = (0, 0, 0)
        r_half = 1.3048 * 3.0 * math.pi / 16.0
        density = 0.5 * n / (4.0 / 3.0 * math.pi * r_half ** 3)
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    m = 0.5 + torch.rand(n, dtype=rdt, device=dev, generator=gen)
    dom = Domain(ctx, cstone_amd.HILBERT, 64, 64, a.bucket, a.bucket_focus, 0.5, cstone_amd.make_cbox(lim, bc))
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    scratch = [torch.empty(n, dtype=rdt, device=dev) for _ in range(3)]
    out = dom.sync(keys, x, y, z, h, scratch, props=[m])
    keys, x, y, z, h = out[:5]
    (m,) = out[-1]
    ctx.sync()
    v = dom.view()
    assert (v.start_index, v.end_index) == (0, n)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def auto(w, e, nb, counts, sums, stats=None):
        ctx._chk(ctx.lib.cstone_hip_domain_pair_counts(dom.h, P(x), P(y), P(z), P(w), 64, e, nb, P(counts), P(sums), stats),
                 "domain_pair_counts")

    res = dict(case=case, n=n, real_bits=64, w_bits=64, bucket_focus=a.bucket_focus, configs=[])
    cfgs = []
    for partners in a.partners:
        outer = (partners / (4.0 / 3.0 * math.pi * density)) ** (1.0 / 3.0)
        for nb in (16, 64):
            for weighted in (False, True):
                e, _ = cstone_amd.sphere_edges(log_edges(nb, 0.01 * outer, outer))
                c = dict(partners=partners, outer=outer, nb=nb, weighted=weighted, e=e, w=m if weighted else None,
                         counts=torch.zeros(nb, dtype=torch.int64, device=dev),
                         sums=torch.zeros(nb, dtype=rdt, device=dev) if weighted else None, ms=[])
                st = (C.c_uint64 * 2)()
                auto(c["w"], e, nb, c["counts"], c["sums"], st)  # warm-up, and the stats
                c["tests"], c["binned"] = int(st[0]), int(st[1])
                cfgs.append(c)
    for _ in range(a.reps):
        for c in cfgs:  # alternating
            c["ms"].append(timed(lambda: auto(c["w"], c["e"], c["nb"], c["counts"], c["sums"])))
    for c in cfgs:
        ms = statistics.median(c["ms"])
        res["configs"].append(dict(partners=c["partners"], outer_edge=c["outer"], nb=c["nb"], weighted=c["weighted"], ms=ms,
                                   ms_runs=c["ms"], pairs_binned=c["binned"], pairs_per_s=c["binned"] / (ms * 1e-3),
                                   tests_per_pair=c["tests"] / max(c["binned"], 1),
                                   partners_found=c["binned"] / n))

    # ---- yardsticks: code that existed before, at the first outer edge, NB = 16, no weights
    if n <= a.yardstick_n:
        outer = cfgs[0]["outer"]
        e, nb = cstone_amd.sphere_edges(log_edges(16, 0.01 * outer, outer))
        qc = torch.stack([x, y, z], dim=1).contiguous()
        rows = torch.zeros((n, nb), dtype=torch.int64, device=dev)
        flags = torch.zeros(n, dtype=torch.int32, device=dev)

        def sphere_rows():
            ctx._chk(ctx.lib.cstone_hip_domain_sphere_profiles(dom.h, P(x), P(y), P(z), None, 64, P(qc), None, n, e, nb,
                                                               P(rows), None, P(flags)), "domain_sphere_profiles")
            return rows.sum(dim=0)

        sphere_rows()
        ms = [timed(sphere_rows) for _ in range(a.reps)]
        total = int(rows.sum().item())
        res["sphere_rows"] = dict(queries=n, nb=nb, outer_edge=outer, ms=statistics.median(ms), ms_runs=ms, binned=total,
                                  equals_auto_plus_selves=bool(total == cfgs[0]["binned"] or total == cfgs[0]["binned"] + n),
                                  pairs_per_s=total / (statistics.median(ms) * 1e-3))
        del rows, qc
        ngmax = 256
        hh = torch.full((n,), 0.5 * outer, dtype=rdt, device=dev)
        nidx = torch.zeros((n, ngmax), dtype=torch.int32, device=dev)
        nc = torch.zeros(n, dtype=torch.int32, device=dev)
        st = (C.c_uint64 * 4)()
        V = C.c_void_p

        def walk():
            ctx._chk(ctx.lib.cstone_hip_find_neighbors_stats(
                ctx.h, C.c_int(64), P(x), P(y), P(z), P(hh), C.c_uint32(0), C.c_uint32(n), C.byref(v.box), V(v.child_offsets),
                V(v.internal_to_leaf), V(v.layout), V(v.centers), V(v.sizes), C.c_float(1.0), C.c_uint32(ngmax), P(nidx), P(nc),
                st), "find_neighbors_stats")

        walk()
        ms = [timed(walk) for _ in range(a.reps)]
        res["neighbors_stats"] = dict(radius=outer, ngmax=ngmax, ms=statistics.median(ms), ms_runs=ms,
                                      neighbors=int(nc.to(torch.int64).sum().item()), stats=[int(s) for s in st])
        del nidx, nc, hh

    # ---- cross counts: a random catalogue as targets
    res["cross"] = []
    outer = cfgs[0]["outer"]
    e, nb = cstone_amd.sphere_edges(log_edges(16, 0.01 * outer, outer))
    for Q in a.cross_queries:
        Q = int(Q)
        if case == "uniform":
            qx, qy, qz = [torch.rand(Q, dtype=rdt, device=dev, generator=gen) for _ in range(3)]
        else:
            qx, qy, qz = clouds.make_cloud("plummer", Q, Q, dev, rdt, a.seed + 1)[:3]
        qc = torch.stack([qx, qy, qz], dim=1).contiguous()
        counts = torch.zeros(nb, dtype=torch.int64, device=dev)

        def cross(stats=None):
            ctx._chk(ctx.lib.cstone_hip_domain_pair_counts_cross(dom.h, P(x), P(y), P(z), None, 64, P(qc), None, Q, e, nb,
                                                                 P(counts), None, stats), "domain_pair_counts_cross")

        def encode_and_sort():
            k = ctx.compute_sfc_keys(cstone_amd.HILBERT, 64, qx, qy, qz, v.box)
            ctx.sort_pairs(k, torch.empty(Q, dtype=torch.int32, device=dev))

        st = (C.c_uint64 * 2)()
        cross(st)
        encode_and_sort()
        full, prep = [], []
        for _ in range(a.reps):  # alternating
            full.append(timed(cross))
            prep.append(timed(encode_and_sort))
        ms = statistics.median(full)
        res["cross"].append(dict(queries=Q, nb=nb, outer_edge=outer, ms=ms, ms_runs=full, encode_sort_ms=statistics.median(prep),
                                 encode_sort_ms_runs=prep, pairs_binned=int(st[1]), pairs_per_s=int(st[1]) / (ms * 1e-3),
                                 tests_per_pair=int(st[0]) / max(int(st[1]), 1)))
        del qc, qx, qy, qz
    ctx.sync()
    dom.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=float, nargs="+", default=[1e6, 1e7])
    p.add_argument("--cases", nargs="+", default=["uniform", "plummer"])
    p.add_argument("--partners", type=float, nargs="+", default=[100, 1000])
    p.add_argument("--cross-queries", type=float, nargs="+", default=[1e6, 1e7])
    p.add_argument("--yardstick-n", type=float, default=1e6)
    p.add_argument("--bucket", type=int, default=1024)
    p.add_argument("--bucket-focus", type=int, default=64)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_counts_bench.jsonl"))
    a = p.parse_args()
    ctx = cstone_amd.Context(0)
    for n in a.n:
        for case in a.cases:
            res = run(ctx, case, int(n), a)
            line = json.dumps(res)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
