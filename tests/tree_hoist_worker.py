"""tests/test_tree_hoist.py runs this in a fresh process per set of environment switches.

`python tree_hoist_worker.py N:BUCKET [N:BUCKET ...]`: per size the single-rank domain (64-bit Hilbert keys, f64
coordinates, open box, four scratch arrays) goes through a script of syncs that takes every branch of the focus-tree
update -- a tree that changes, a tree that does not, a re-sort that falls back inside the sync and backs off, removed
particles, a box that has to be redone -- and prints one SHA-256 over everything a client can see, and beside it the counters of the domain.

`python tree_hoist_worker.py allremoved`: a sync with every particle marked removed; prints the error code, then
whether the next sync of the same particles without the markers orders them."""
import hashlib
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cornerstone-octree_amd"))

import torch  # noqa: E402

import cstone_amd  # noqa: E402
from cstone_amd.domain import Domain  # noqa: E402

REMOVE_KEY = torch.iinfo(torch.int64).min  # bit pattern of the end of the 64-bit curve
# (four syncs of back-off follow the re-sort that fell back: the removal and the moving extreme meet re-sorted syncs again)
SCRIPT = ["first", "drift", "drift", "none", "none", "none", "drift", "jump", "drift", "drift", "drift", "drift", "drift",
          "remove", "drift", "extreme", "drift", "drift"]


class Run:
    def __init__(self, hip, n, bucket_focus, seed):
        self.hip, self.n = hip, n
        self.step = 0.02 * (bucket_focus / n) ** (1.0 / 3.0)  # a fiftieth of a full leaf: a few percent change leaves
        self.g = torch.Generator(device="cuda").manual_seed(seed)
        self.x, self.y, self.z = (self.rand(n) for _ in range(3))
        self.h = torch.full((n,), 0.6 * (300.0 / (4.0 * np.pi * n)) ** (1.0 / 3.0), dtype=torch.float64, device="cuda")
        self.keys = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.scratch = [torch.empty_like(self.x) for _ in range(4)]
        lim = [0.0, 1.0, 0.0, 1.0, 0.0, 1.0]
        self.dom = Domain(hip, cstone_amd.HILBERT, 64, 64, max(64, n // 100), bucket_focus, 0.5,
                          cstone_amd.make_cbox(lim, (0, 0, 0)))

    def rand(self, m):
        return torch.rand(m, dtype=torch.float64, device="cuda", generator=self.g)

    def some(self, one_in):
        m = self.x.numel()
        return torch.randperm(m, device="cuda", generator=self.g)[: max(1, m // one_in)]

    def move(self, kind):
        coords = (self.x, self.y, self.z)
        ext = [(float(a.min()), float(a.max())) for a in coords]  # nobody leaves the extents, but for "extreme"
        if kind == "drift":  # everybody, by a fraction of a leaf: counts cross the bucket size here and there
            for a, (lo, hi) in zip(coords, ext):
                a.add_(self.step * (2.0 * self.rand(a.numel()) - 1.0)).clamp_(lo, hi)
        elif kind == "jump":  # a fifth of the particles anywhere: too many movers, the radix path in the same sync
            sel = self.some(5)
            for a, (lo, hi) in zip(coords, ext):
                a[sel] = lo + (hi - lo) * self.rand(sel.numel())
        elif kind == "remove":  # 5 % leave
            self.keys[self.some(20)] = REMOVE_KEY
        elif kind == "extreme":  # the outermost particle in x moves out: the speculated box is wrong
            self.x[torch.argmax(self.x)] += 0.07
            self.z[torch.argmin(self.z)] -= 0.03

    def sync(self, digest):
        ident = self.x * 3.0 + self.y * 5.0 + self.z * 7.0
        self.keys, self.x, self.y, self.z, self.h, self.scratch, (ident,) = self.dom.sync(
            self.keys, self.x, self.y, self.z, self.h, self.scratch, [ident])
        self.hip.sync()
        if self.scratch[0].numel() != self.x.numel():  # particles were removed: the client shrinks its arrays
            self.keys, self.x, self.y, self.z, self.h = [t.clone() for t in (self.keys, self.x, self.y, self.z, self.h)]
            self.scratch = [torch.empty_like(self.x) for _ in range(4)]
        v = self.dom.view()
        L = v.num_focus_leaves
        leaves = self.dom.fetch(v.focus_leaves, L + 1, np.uint64)
        for t in (self.keys, self.x, self.y, self.z, self.h, ident):
            digest.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
        for a in (leaves, self.dom.fetch(v.focus_leaf_counts, L, np.uint32), self.dom.fetch(v.layout, L + 1, np.uint32),
                  self.dom.fetch(v.halo_radii, L, np.float32),
                  self.dom.fetch(v.global_leaves, v.num_global_leaves + 1, np.uint64)):
            digest.update(a.tobytes())
        digest.update(np.asarray(v.box.lim, dtype=np.float64).tobytes())
        return leaves


def script(hip, n, bucket_focus):
    run = Run(hip, n, bucket_focus, 11 + bucket_focus)
    digest = hashlib.sha256()
    before, rebuilt, kept = None, 0, 0
    for step, kind in enumerate(SCRIPT):
        run.move(kind)
        leaves = run.sync(digest)
        if step:
            same = leaves.size == before.size and np.array_equal(leaves, before)
            kept, rebuilt = kept + same, rebuilt + (not same)
        before = leaves
    st = run.dom.stats()
    os.write(1, (f"DIGEST {digest.hexdigest()} n {n} bucket {bucket_focus} resorts {st['resorts']} rebuilt {rebuilt} "
                 f"kept {kept} fallbacks {st['resort_fallbacks']} box_redos {st['box_redos']}\n").encode())


def all_removed(hip):
    run = Run(hip, 100_000, 64, 5)
    digest = hashlib.sha256()
    for kind in ("first", "drift", "drift"):
        run.move(kind)
        run.sync(digest)
    run.keys[:] = REMOVE_KEY
    try:
        run.sync(digest)
        os.write(1, b"ERROR none\n")
    except cstone_amd.CstoneError as e:
        m = re.search(r"failed \((-?\d+)\): (.*)", str(e))
        os.write(1, f"ERROR {m.group(1)} resorts {run.dom.stats()['resorts']} | {m.group(2)}\n".encode())
    # the domain goes on with the same particles once the client has taken the markers back
    run.keys[:] = 0
    run.sync(digest)
    k = run.keys.cpu().numpy().view(np.uint64)
    os.write(1, f"RECOVERED particles {k.size} sorted {bool(np.all(k[1:] >= k[:-1]) and k[-1] > k[0])}\n".encode())


if __name__ == "__main__":
    ctx = cstone_amd.Context(0)
    if sys.argv[1] == "allremoved":
        all_removed(ctx)
    else:
        for arg in sys.argv[1:]:
            size, bucket = arg.split(":")
            script(ctx, int(float(size)), int(bucket))
