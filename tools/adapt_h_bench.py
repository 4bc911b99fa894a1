#!/usr/bin/env python3
"""cstone_hip_domain_adapt_h against the host loop it replaces, on the arrays of a synced single-rank domain.

For every (cloud, n, real type): h0 = the h of ng0 neighbours at the local density, off by a factor U(0.8, 1.2).  Timed:
  fused      one Domain.adapt_h (one kernel: every wave repeats its walk while a lane is unconverged)
  one_walk   one cstone_hip_find_neighbors(ngmax = 0) over all particles at h0
  host_loop  the same rule as a loop of find_neighbors(ngmax = 0) over ALL particles + a torch update, until nothing is
             active (the end state is compared with the fused call's)
and from the status words the mean over waves of 64 targets of the largest number of walks in the wave: the fused call
is expected to cost about that many counting walks.  One JSON line per configuration is appended to --out."""
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

NOT_CONVERGED, CAPPED, STALLED = cstone_amd.ADAPT_H_NOT_CONVERGED, cstone_amd.ADAPT_H_CAPPED, cstone_amd.ADAPT_H_STALLED


class Raw:
    """a device pointer of the domain view where the bindings expect a tensor"""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


def timed(fn, reps):
    out, ts = None, []
    for _ in range(reps + 1):  # the first run warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts[1:]


def host_loop(ctx, x, y, z, h0, n, box, tree, layout, cen, siz, ng0, tol, max_iter, grow_limit):
    """the rule of include/cstone_hip.h with torch, one full counting walk per pass"""
    T = h0.dtype
    h = h0.clone()
    lo, hi = torch.zeros_like(h), torch.full_like(h, math.inf)
    hcap = h * grow_limit
    active = torch.ones(n, dtype=torch.bool, device=h.device)
    nn = torch.zeros(n, dtype=torch.int64, device=h.device)
    walks = torch.zeros(n, dtype=torch.int32, device=h.device)
    flags = torch.zeros(n, dtype=torch.int32, device=h.device)
    passes = 0
    for it in range(max_iter + 1):
        if not bool(active.any()):
            break
        cnt = ctx.find_neighbors(x, y, z, h, 0, n, box, tree, layout, cen, siz, 0)[1].to(torch.int64)
        passes += 1
        nn = torch.where(active, cnt, nn)
        walks += active
        a = active & ~((nn + tol >= ng0) & (nn <= ng0 + tol))
        if it == max_iter:
            flags[a] |= NOT_CONVERGED
            break
        low = nn + tol < ng0
        lo, hi = torch.where(a & low, h, lo), torch.where(a & ~low, h, hi)
        capped = a & low & (h >= hcap)
        flags[capped] |= CAPPED
        a &= ~capped
        q = (torch.tensor(float(ng0), dtype=T, device=h.device) / nn.clamp(min=1).to(T)).clamp(0.125, 8.0)
        t = (2 + q) / 3
        t = (2 * t + q / (t * t)) / 3
        hp = torch.minimum(h * t, hcap)
        hp = torch.where((hi < math.inf) & ~((lo < hp) & (hp < hi)), 0.5 * (lo + hi), hp)
        stalled = a & (hp == h)
        flags[stalled] |= STALLED
        a &= ~stalled
        h = torch.where(a, hp, h)
        active = a
    return h, nn, walks | flags, passes


def run(ctx, dist, n, rb, a):
    dev, rdt = "cuda", (torch.float64 if rb == 64 else torch.float32)
    if dist == "uniform":
        g = torch.Generator(device=dev).manual_seed(a.seed)
        x, y, z = [torch.rand(n, dtype=rdt, device=dev, generator=g) for _ in range(3)]
        h = torch.full((n,), 0.5 * (3.0 * a.ng0 / (4 * math.pi * n)) ** (1.0 / 3.0), dtype=rdt, device=dev)
        lim = [0.0, 1.0] * 3
    else:
        x, y, z, h, lim = clouds.make_cloud("plummer", n, n, dev, rdt, a.seed)
        h = clouds.plummer_h(x, y, z, n, float(a.ng0))
    g = torch.Generator(device=dev).manual_seed(a.seed + 1)
    h = (h.double() * (0.8 + 0.4 * torch.rand(n, dtype=torch.float64, device=dev, generator=g))).to(rdt)
    dom = Domain(ctx, cstone_amd.HILBERT, 64, rb, a.bucket, a.bucket_focus, 0.5, cstone_amd.make_cbox(lim))
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    scratch = [torch.empty(n, dtype=rdt, device=dev) for _ in range(3)]
    keys, x, y, z, h0, _, _ = dom.sync(keys, x, y, z, h, scratch)
    ctx.sync()
    v = dom.view()
    assert (v.start_index, v.end_index) == (0, n)
    tree = dict(child_offsets=Raw(v.child_offsets), internal_to_leaf=Raw(v.internal_to_leaf))
    layout, cen, siz = Raw(v.layout), Raw(v.centers), Raw(v.sizes)
    grow = math.inf

    def fused():
        hw = h0.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cnt, st = dom.adapt_h(x, y, z, hw, a.ng0, a.tol, a.max_iter)
        torch.cuda.synchronize()
        return hw, cnt, st, (time.perf_counter() - t0) * 1e3

    runs = [fused() for _ in range(a.reps + 1)][1:]
    hw, cnt, st = runs[-1][:3]
    t_fused = [r[3] for r in runs]
    _, t_walk = timed(lambda: ctx.find_neighbors(x, y, z, h0, 0, n, v.box, tree, layout, cen, siz, 0), a.reps)
    (hl, nl, sl, passes), t_loop = timed(
        lambda: host_loop(ctx, x, y, z, h0, n, v.box, tree, layout, cen, siz, a.ng0, a.tol, a.max_iter, grow), a.reps)
    walks = (st & 0xFF).to(torch.float64)
    pad = (-n) % 64
    per_wave = torch.cat([walks, torch.zeros(pad, dtype=walks.dtype, device=dev)]).view(-1, 64).max(1).values
    res = dict(cloud=dist, n=n, real_bits=rb, ng0=a.ng0, tol=a.tol, max_iter=a.max_iter, focus_leaves=v.num_focus_leaves,
               fused_ms=statistics.median(t_fused), fused_ms_runs=t_fused,
               one_walk_ms=statistics.median(t_walk), one_walk_ms_runs=t_walk,
               host_loop_ms=statistics.median(t_loop), host_loop_ms_runs=t_loop, host_loop_passes=passes,
               mean_walks=walks.mean().item(), mean_wave_max_walks=per_wave.mean().item(),
               max_walks=int(walks.max().item()),
               not_converged=int(((st & NOT_CONVERGED) != 0).sum()), capped=int(((st & CAPPED) != 0).sum()),
               stalled=int(((st & STALLED) != 0).sum()),
               host_loop_h_equal=int((hl.view(torch.uint8) == hw.view(torch.uint8)).view(n, -1).all(1).sum()),
               host_loop_status_equal=int((sl == st).sum()),
               mean_count=cnt.double().mean().item())
    res["fused_over_walk"] = res["fused_ms"] / res["one_walk_ms"]
    res["loop_over_fused"] = res["host_loop_ms"] / res["fused_ms"]
    dom.close()
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=float, nargs="+", default=[1e6, 1e7])
    p.add_argument("--dist", nargs="+", default=["uniform", "plummer"], choices=["uniform", "plummer"])
    p.add_argument("--real-bits", type=int, nargs="+", default=[64, 32])
    p.add_argument("--ng0", type=int, default=100)
    p.add_argument("--tol", type=int, default=10)
    p.add_argument("--max-iter", type=int, default=10)
    p.add_argument("--bucket", type=int, default=1024)
    p.add_argument("--bucket-focus", type=int, default=64)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapt_h_bench.jsonl"))
    a = p.parse_args()
    ctx = cstone_amd.Context(0)
    for dist in a.dist:
        for n in a.n:
            for rb in a.real_bits:
                res = run(ctx, dist, int(n), rb, a)
                line = json.dumps(res)
                print(line, flush=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
