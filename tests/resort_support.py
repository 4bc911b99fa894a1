"""What the tests of the re-sort's schedule share (test_resort_scenarios.py, test_encode_tile_order.py, test_resort_plan.py): a client's
time-stepping loop on device arrays, the motion of the issue's common comparison, and the bit-for-bit comparison of two
domains.  Not a test module."""
import contextlib
import os

import numpy as np


@contextlib.contextmanager
def environment(**values):
    """the given variables set (None: unset) for the block; what they were before is put back, set or not"""
    before = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def cloud(rng, n):
    """half uniform, half in five clumps, inside [0, 1)^3"""
    centers = rng.uniform(0.2, 0.8, (5, 3))
    pos = np.where(rng.uniform(size=(n, 1)) < 0.5, rng.uniform(0, 1, (n, 3)),
                   centers[rng.integers(0, 5, n)] + rng.normal(0, 0.03, (n, 3)))
    return np.clip(pos, 0.0, 1.0 - 1e-6)


def smoothing_lengths(rng, n):
    """a tenth to one times 0.27 mean particle distances (0.001 - 0.01 at 2 * 10^4 particles): a displacement of 0.1 h stays a
    small fraction of a leaf at every size, in the clumps too"""
    return rng.uniform(0.1, 1.0, n) * 0.27 * float(n) ** (-1.0 / 3.0)


class Loop:
    """a client's loop: the arrays a sync returns are moved in place and handed to the next sync (four scratch arrays, as
    bench.py hands over); ident follows its particle as a property"""

    def __init__(self, ctx, kb, rb, bucket_focus, curve, n, seed, mode=None, bc=(1, 1, 1), pos=None, h=None):
        import torch

        import cstone_amd
        from cstone_amd.domain import Domain

        rng = np.random.default_rng(seed)
        self.ctx, self.kb, self.rb = ctx, kb, rb
        self.rdt = torch.float64 if rb == 64 else torch.float32
        self.kdt = torch.int64 if kb == 64 else torch.int32
        self.dom = Domain(ctx, curve, kb, rb, max(bucket_focus, 64) * 4, bucket_focus, 0.5,
                          cstone_amd.make_cbox([0, 1, 0, 1, 0, 1], bc))
        if mode is not None:
            self.dom.set_sort_mode(mode)
        pos = cloud(rng, n) if pos is None else pos
        h = smoothing_lengths(rng, n) if h is None else h
        self.x, self.y, self.z = [torch.from_numpy(np.ascontiguousarray(pos[:, d])).to(self.rdt).cuda() for d in range(3)]
        self.h = torch.from_numpy(h).to(self.rdt).cuda()
        self.ident = torch.arange(n, dtype=self.rdt, device="cuda")
        self.keys = torch.zeros(n, dtype=self.kdt, device="cuda")
        self.scratch = [torch.empty_like(self.x) for _ in range(4)]

    def sync(self):
        self.keys, self.x, self.y, self.z, self.h, self.scratch, (self.ident,) = self.dom.sync(
            self.keys, self.x, self.y, self.z, self.h, self.scratch, [self.ident])
        self.ctx.sync()
        if self.scratch[0].numel() != self.x.numel():
            self.resize()
        return self

    def resize(self):
        """particles left: fresh arrays of the new size (every array stays 16-byte aligned)"""
        import torch

        self.keys, self.x, self.y, self.z, self.h, self.ident = [t.clone() for t in (
            self.keys, self.x, self.y, self.z, self.h, self.ident)]
        self.scratch = [torch.empty_like(self.x) for _ in range(4)]

    def arrays(self):
        return dict(keys=self.keys, x=self.x, y=self.y, z=self.z, h=self.h, ident=self.ident)


class Motion:
    """the common motion: every particle displaced by at most 0.1 h per coordinate, 2 % (one at least) jump anywhere in
    the box.  Drawn once per step on the device and applied to every loop of the comparison: the loops hold the same
    arrays in the same order, so they see the same motion.  periodic: positions wrap, else they are clamped to the extents
    the particles have (the box of an open domain then stays what it is)"""

    def __init__(self, seed, periodic=True):
        import torch

        self.gen = torch.Generator(device="cuda")
        self.gen.manual_seed(seed)
        self.periodic = periodic

    def draw(self, loop):
        import torch

        m = loop.x.numel()
        frac = [torch.rand(m, generator=self.gen, device="cuda", dtype=torch.float64) * 0.2 - 0.1 for _ in range(3)]
        jumpers = torch.randperm(m, generator=self.gen, device="cuda")[:max(1, m // 50)]
        where = [torch.rand(jumpers.numel(), generator=self.gen, device="cuda", dtype=torch.float64) for _ in range(3)]
        return frac, jumpers, where

    def apply(self, loop, drawn):
        frac, jumpers, where = drawn
        for a, f, w in zip((loop.x, loop.y, loop.z), frac, where):
            lo, hi = (0.0, 1.0) if self.periodic else (float(a.min()), float(a.max()))
            a.add_((f * loop.h.double()).to(a.dtype))
            a[jumpers] = (lo + w * (hi - lo)).to(a.dtype)
            if self.periodic:
                a.remainder_(1.0)
                a.clamp_(0.0, 1.0 - 1e-6)
            else:
                a.clamp_(lo, hi)


def assert_same(a, b, what):
    """bit for bit: keys, x, y, z, h, the carried index, layout, leaves and leaf counts of two loops"""
    import torch

    va, vb = a.dom.view(), b.dom.view()
    assert (va.end_index, va.num_focus_leaves) == (vb.end_index, vb.num_focus_leaves), what
    for (name, ta), tb in zip(a.arrays().items(), b.arrays().values()):
        assert torch.equal(ta, tb), (what, name)
    L = va.num_focus_leaves
    kdt = np.uint64 if a.kb == 64 else np.uint32
    for field, count, dt in (("layout", L + 1, np.uint32), ("focus_leaf_counts", L, np.uint32),
                             ("focus_leaves", L + 1, kdt), ("halo_radii", L, np.float32)):
        assert np.array_equal(a.dom.fetch(getattr(va, field), count, dt), b.dom.fetch(getattr(vb, field), count, dt)), (
            what, field)
