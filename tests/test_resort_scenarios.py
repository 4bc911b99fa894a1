"""Scenarios the incremental re-sort of Domain::sync (csrc/resort.hpp, csrc/domain.hip: tryResort) must survive: several
domains on one context, refused calls, removals, a change of the sort mode, arrays permuted by the caller, a moving open
box, other work on the context between two syncs, a failed sync.  Every case runs the same client loop through a domain
that sorts from scratch and through a re-sorting one, compares them bit for bit after every sync, and checks which syncs
were re-sorted."""
import numpy as np
import pytest

from resort_support import Loop, Motion, assert_same, environment

N, BUCKET = 20_000, 16


class Pair:
    """the two loops of a comparison in lockstep"""

    def __init__(self, ctx, seed, kb=64, rb=64, curve=1, bc=(1, 1, 1), n=N):
        from cstone_amd.domain import Domain

        self.ref = Loop(ctx, kb, rb, BUCKET, curve, n, seed, mode=Domain.SORT_FROM_SCRATCH, bc=bc)
        self.lp = Loop(ctx, kb, rb, BUCKET, curve, n, seed, bc=bc)
        self.motion = Motion(seed + 100, periodic=all(bc))
        self.step = 0
        self.movers = 0

    def loops(self):
        return (self.ref, self.lp)

    def sync(self, move=True):
        """one step of the client: move (not before the first sync), sync, compare"""
        if move and self.step:
            drawn = self.motion.draw(self.ref)
            for lp in self.loops():
                self.motion.apply(lp, drawn)
        for lp in self.loops():
            lp.sync()
        assert_same(self.lp, self.ref, self.step)
        self.step += 1
        self.movers += self.lp.dom.stats()["last_movers"]
        return self

    def resorts(self):
        return self.lp.dom.stats()["resorts"]


@pytest.mark.gpu
@pytest.mark.parametrize("kb,rb,curve", [(64, 64, 1), (32, 32, 0)])
def test_plain_loop(hip, kb, rb, curve):
    t = Pair(hip, 1, kb, rb, curve)
    for step in range(6):
        t.sync()
        assert t.resorts() == step  # one per steady sync
    assert t.movers > 0


@pytest.mark.gpu
def test_two_domains_on_one_context(hip):
    """the slots of the context's scalar block are shared by everything on the context: nothing of a domain's re-sort
    lives there between two of its syncs"""
    a, b = Pair(hip, 2), Pair(hip, 3, n=N + 4321)
    for step in range(5):
        a.sync()
        b.sync()
        assert a.resorts() == step and b.resorts() == step
    assert a.movers > 0 and b.movers > 0


@pytest.mark.gpu
def test_a_call_with_another_particle_count_in_between(hip):
    """a sync refuses arrays of another length than the domain holds (particles leave through remove markers only); the
    syncs behind the refused call re-sort as if it had not been made"""
    import torch

    import cstone_amd

    t = Pair(hip, 4)
    t.sync().sync().sync()
    for change in (7, -5):
        for lp in t.loops():
            m = lp.x.numel() + change
            grown = [torch.zeros(m, dtype=a.dtype, device="cuda") for a in (lp.keys, lp.x, lp.y, lp.z, lp.h)]
            for g, a in zip(grown, (lp.keys, lp.x, lp.y, lp.z, lp.h)):
                g[:min(m, a.numel())] = a[:min(m, a.numel())]
            with pytest.raises(cstone_amd.CstoneError, match="inconsistent"):
                lp.dom.sync(*grown, [torch.empty_like(grown[1]) for _ in range(4)])
        before = t.resorts()
        t.sync()
        assert t.resorts() == before + 1
        t.sync()
    assert t.movers > 0


@pytest.mark.gpu
def test_remove_markers(hip):
    import torch

    t = Pair(hip, 5)
    t.sync().sync()
    for step in range(2, 6):
        m = t.ref.x.numel()
        sel = torch.from_numpy(np.random.default_rng(step).choice(m, m // 100, replace=False)).cuda()
        for lp in t.loops():
            lp.keys[sel] = torch.iinfo(torch.int64).min  # bit pattern of endKey
        t.sync()
        assert t.ref.x.numel() == m - sel.numel()
        assert t.resorts() == step
    assert t.movers > 0


@pytest.mark.gpu
def test_a_sync_sorted_from_scratch_in_between(hip):
    t = Pair(hip, 6)
    t.sync().sync().sync()
    assert t.resorts() == 2
    t.lp.dom.set_sort_mode(t.lp.dom.SORT_ALL_DIGITS)
    t.sync()
    assert t.resorts() == 2
    t.lp.dom.set_sort_mode(t.lp.dom.SORT_INCREMENTAL)
    t.sync()
    assert t.resorts() == 3
    t.sync()
    assert t.resorts() == 4
    assert t.movers > 0


@pytest.mark.gpu
def test_arrays_permuted_by_the_caller(hip):
    """every particle is a mover then: the attempt is given up, the domain backs off, and the re-sorts come back
    afterwards"""
    import torch

    t = Pair(hip, 7)
    t.sync().sync().sync()
    perm = torch.from_numpy(np.random.default_rng(0).permutation(t.ref.x.numel())).cuda()
    for lp in t.loops():
        lp.x, lp.y, lp.z, lp.h, lp.ident = [a[perm].contiguous() for a in (lp.x, lp.y, lp.z, lp.h, lp.ident)]
    t.sync(move=False)
    assert t.resorts() == 2 and t.lp.dom.stats()["resort_fallbacks"] == 1
    for _ in range(6):
        t.sync()
    assert t.resorts() >= 3
    assert t.movers > 0


@pytest.mark.gpu
def test_open_box_whose_outermost_particle_moves(hip):
    """the encode speculates on the box of the sync before; a particle that leaves it makes the attempt fall back and the
    following syncs measure first"""
    t = Pair(hip, 8, bc=(0, 0, 0))
    t.sync().sync().sync()
    assert t.resorts() == 2
    for lp in t.loops():
        at = int(lp.x.argmax())
        lp.x[at] += 0.05
    t.sync(move=False)
    assert t.lp.dom.stats()["box_redos"] >= 1 and t.resorts() == 2
    for _ in range(4):
        t.sync()
    assert t.resorts() > 2
    assert t.movers > 0


@pytest.mark.gpu
def test_other_work_on_the_context_between_two_syncs(hip):
    """sorts, scans, tree builds and a neighbour search use the context's scalar slots and its arena between two syncs"""
    import torch

    import cstone_amd

    t = Pair(hip, 9)
    box = cstone_amd.make_cbox([0, 1, 0, 1, 0, 1], (1, 1, 1))
    for step in range(5):
        t.sync()
        assert t.resorts() == step
        x, y, z, h = [a.clone() for a in (t.ref.x, t.ref.y, t.ref.z, t.ref.h)]
        n = x.numel()
        keys = hip.compute_sfc_keys(1, 64, x, y, z, box)
        vals = torch.arange(n, dtype=torch.int32, device="cuda")
        hip.sort_pairs(keys.flip(0).contiguous(), vals)
        tree, counts, _ = hip.compute_octree(keys, 16)
        layout = torch.zeros(counts.numel() + 1, dtype=torch.int32, device="cuda")
        hip.exclusive_scan(torch.cat([counts, torch.zeros(1, dtype=torch.int32, device="cuda")]), layout)
        oc = hip.build_octree(tree)
        centers, sizes = hip.node_centers(1, oc["prefixes"], box, 64)
        hip.find_neighbors(x, y, z, h, 0, n, box, oc, layout, centers, sizes, 32)
        hip.sync()
        assert int(layout[-1]) == n
    assert t.movers > 0


@pytest.mark.gpu
def test_a_failed_sync(hip, monkeypatch):
    """with the tests' build of the library: a sync whose device-side check word is raised fails at its end, behind its
    re-sort; the following syncs re-sort from what it left"""
    import cstone_amd

    monkeypatch.setenv("CSTONE_HIP_LIB", cstone_amd.LIBPATH.replace("libcstone_hip.so", "libcstone_hip_hooks.so"))
    hooked = cstone_amd.Context(0)
    monkeypatch.delenv("CSTONE_HIP_LIB")
    assert hooked.lib.cstone_hip_test_hooks() == 1
    t = Pair(hooked, 10)
    t.sync().sync().sync()
    # the same sync for both (the trees take the same steps), on copies: a failed call leaves its arrays undefined.
    # Nothing moves before it, so the arrays of the loops stay in the order the domains hold
    for lp in t.loops():
        copies = [a.clone() for a in (lp.keys, lp.x, lp.y, lp.z, lp.h)]
        scratch, ident = [a.clone() for a in lp.scratch], lp.ident.clone()
        with environment(CSTONE_FORCE_DEVICE_ERROR=None if lp is t.ref else "1"):
            if lp is t.ref:
                lp.dom.sync(*copies, scratch, [ident])
            else:
                with pytest.raises(cstone_amd.CstoneError, match="device-side check failed"):
                    lp.dom.sync(*copies, scratch, [ident])
        hooked.sync()
    assert t.resorts() == 3
    t.sync()
    assert t.resorts() == 4
    t.sync()
    assert t.resorts() == 5
    assert t.movers > 0
