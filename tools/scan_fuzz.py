#!/usr/bin/env python3
"""fuzz of the device scans (cstone_hip_exclusive_scan_u32 / _inclusive_scan_u32 / _offsets_from_counts_u32) against torch.cumsum: many sizes in a row on
ONE context, in place and out of place -- what a long-lived client does to the single-launch scan's persistent state"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cornerstone-octree_amd"))
import torch  # noqa: E402

import cstone_amd  # noqa: E402

ctx = cstone_amd.Context(0)
g = torch.Generator(device="cuda").manual_seed(5)
bad = 0
sizes = [1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 20000, 20001, 65536, 100000, 300000, 524288, 524289, 600000]
import random
random.seed(3)
M = 0xFFFFFFFF


def scan(fn, src, dst, n, *more):
    return fn(ctx.h, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.c_size_t(n), *more)


for it in range(3000):
    n = random.choice(sizes) if it % 3 else random.randint(1, 530000)
    # every seventh array over the full 32-bit range: the sums wrap modulo 2^32 (int64 -> int32 keeps the low 32 bits)
    a = torch.randint(0, 1 << 32 if it % 7 == 0 else 50, (n,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    v = a.long() & M
    want_in = torch.cumsum(v, 0)
    want_ex = want_in - v
    mode = it % 5
    if mode == 0:
        out = torch.empty_like(a)
        rc = scan(ctx.lib.cstone_hip_exclusive_scan_u32, a, out, n, C.c_uint32(7))
        want = want_ex + 7
    elif mode == 1:
        out = a.clone()
        rc = scan(ctx.lib.cstone_hip_exclusive_scan_u32, out, out, n, C.c_uint32(0))
        want = want_ex
    elif mode == 2:
        out = torch.empty_like(a)
        rc = scan(ctx.lib.cstone_hip_inclusive_scan_u32, a, out, n)
        want = want_in
    elif mode == 3:
        out = a.clone()
        rc = scan(ctx.lib.cstone_hip_inclusive_scan_u32, out, out, n)
        want = want_in
    else:  # n + 1 offsets: the exclusive scan with its total behind it
        out = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        rc = scan(ctx.lib.cstone_hip_offsets_from_counts_u32, a, out, n)
        want = torch.cat([want_ex, want_in[-1:]])
    d = ((out.long() & M) != (want & M)).nonzero()
    if rc != 0 or d.numel():
        bad += 1
        if bad < 10:
            print("MISMATCH it", it, "n", n, "mode", mode, "rc", rc, "first bad", int(d[0]) if d.numel() else None, "count", d.numel(), flush=True)
ctx.sync()
print("scan fuzz:", "OK" if bad == 0 else f"{bad} failures")
sys.exit(0 if bad == 0 else 1)
