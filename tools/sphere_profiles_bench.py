#!/usr/bin/env python3
"""cstone_hip_sphere_profiles (csrc/sphere.hip) on the clouds of tools/fof_props_bench.py: a uniform cloud in a periodic box
at b = 0.9 x the mean separation and a Plummer sphere at 0.9 x the mean separation inside its half-mass radius (at the 0.2 x
of that tool neither cloud has a group of 20 members).  The queries are the centres of the friends-of-friends catalogue
(groups of at least --min-members members, the --max-queries largest), with 16 and with 64 logarithmic bins from 0.05 to 3
group radii, f64 coordinates and f64 weights.

Timed with events on the context's stream around the C entry alone, on outputs allocated beforehand; the two bin counts
ALTERNATE run by run (16, 64, 16, 64, ...) after one warm-up run each, and every run is kept beside the median.
  kernel_ms             the call
  queries_per_s         queries / kernel time
  binned_per_s          particles counted in some bin (the sum of all counts) / kernel time
  leaf_bytes_fraction   (3 x 8 + 8) bytes per particle binned / kernel time, over READ_STREAM_BYTES_PER_S: what the binned
                        particles alone cost to read, against what read streams reach on this machine.
                        The kernel also reads the particles of opened leaves that fall outside the last edge, and a
                        particle binned by several queries is mostly served from cache: a ratio to write down, no target.
  few_large_ms          the known weakness: --few queries at the cloud's centre that hold most of the cloud, 16 bins -- one
                        wave each, the rest of the chip idle
One JSON line per case is appended to --out."""
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

READ_STREAM_BYTES_PER_S = 4.6e12  # what read streams reach on one MI355X


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
    if case.startswith("uniform"):
        x, y, z, h = clouds.uniform(n, dev, rdt, a.seed)
        lim, bc = [0.0, 1.0] * 3, (1, 1, 1)
        b = float(case.split("-")[1]) * n ** (-1.0 / 3.0)
        middle = [0.5, 0.5, 0.5]
    else:
        x, y, z, h, lim = clouds.make_cloud("plummer", n, n, dev, rdt, a.seed)
        bc = (0, 0, 0)
        r_half = 1.3048 * 3.0 * math.pi / 16.0
        b = float(case.split("-")[1]) * (4.0 / 3.0 * math.pi * r_half ** 3 / (0.5 * n)) ** (1.0 / 3.0)
        middle = [0.0, 0.0, 0.0]
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
    labels, _, _ = dom.fof(x, y, z, b, want_sizes=False)
    off, mem = ctx.fof_catalog(labels, 0, n, a.min_members)
    _, center, _, radius, _ = dom.fof_properties(x, y, z, m, off, mem)
    sizes = (off[1:] - off[:-1]).to(torch.int64)
    keep = torch.argsort(sizes, descending=True)[:a.max_queries]
    qc, qs = center[keep].contiguous(), radius[keep].contiguous()
    Q = qc.shape[0]
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def profiles(qc, qs, edges, counts, sums, flags):
        e, nb = cstone_amd.sphere_edges(edges)
        ctx._chk(ctx.lib.cstone_hip_domain_sphere_profiles(dom.h, P(x), P(y), P(z), P(m), 64, P(qc), P(qs), qc.shape[0], e,
                                                           nb, P(counts), P(sums), P(flags)), "domain_sphere_profiles")

    res = dict(case=case, n=n, real_bits=64, mass_bits=64, linking_length=b, min_members=a.min_members, queries=Q,
               largest_group=int(sizes.max().item()) if sizes.numel() else 0,
               median_radius=float(qs.median().item()) if Q else 0.0)
    if Q:
        cfg = {}
        for nb in (16, 64):
            cfg[nb] = dict(edges=log_edges(nb, 0.05, 3.0), counts=torch.zeros((Q, nb), dtype=torch.int64, device=dev),
                           sums=torch.zeros((Q, nb), dtype=rdt, device=dev),
                           flags=torch.zeros(Q, dtype=torch.int32, device=dev), ms=[])
            profiles(qc, qs, **{k: cfg[nb][k] for k in ("edges", "counts", "sums", "flags")})  # warm-up
        for _ in range(a.reps):
            for nb in (16, 64):  # alternating
                c = cfg[nb]
                c["ms"].append(timed(lambda: profiles(qc, qs, c["edges"], c["counts"], c["sums"], c["flags"])))
        for nb in (16, 64):
            c = cfg[nb]
            ms = statistics.median(c["ms"])
            binned = int(c["counts"].sum().item())
            res[f"nb{nb}"] = dict(kernel_ms=ms, kernel_ms_runs=c["ms"], queries_per_s=Q / (ms * 1e-3), binned=binned,
                                  binned_per_s=binned / (ms * 1e-3), wide=int((c["flags"] != 0).sum().item()),
                                  leaf_bytes_fraction=32.0 * binned / (ms * 1e-3) / READ_STREAM_BYTES_PER_S)
    # the known weakness: a few spheres that hold most of the cloud
    few = torch.tensor([middle] * a.few, dtype=rdt, device=dev)
    reach = 0.49 if case.startswith("uniform") else 3.0
    scale = torch.full((a.few,), reach, dtype=rdt, device=dev)
    edges = log_edges(16, 0.05, 1.0)
    counts, sums = torch.zeros((a.few, 16), dtype=torch.int64, device=dev), torch.zeros((a.few, 16), dtype=rdt, device=dev)
    flags = torch.zeros(a.few, dtype=torch.int32, device=dev)
    profiles(few, scale, edges, counts, sums, flags)
    ms = [timed(lambda: profiles(few, scale, edges, counts, sums, flags)) for _ in range(a.reps)]
    binned = int(counts.sum().item())
    res["few_large"] = dict(queries=a.few, kernel_ms=statistics.median(ms), kernel_ms_runs=ms, binned=binned,
                            binned_per_s=binned / (statistics.median(ms) * 1e-3),
                            leaf_bytes_fraction=32.0 * binned / (statistics.median(ms) * 1e-3) / READ_STREAM_BYTES_PER_S)
    ctx.sync()
    dom.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=float, nargs="+", default=[1e6, 1e7])
    p.add_argument("--cases", nargs="+", default=["uniform-0.9", "plummer-0.9"])
    p.add_argument("--bucket", type=int, default=1024)
    p.add_argument("--bucket-focus", type=int, default=64)
    p.add_argument("--min-members", type=int, default=20)
    p.add_argument("--max-queries", type=int, default=16384)
    p.add_argument("--few", type=int, default=4)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sphere_profiles_bench.jsonl"))
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
