"""With CSTONE_EARLY_LEAF_TABLE=1 the leaf table of a re-sort (csrc/resort.hpp, prepareTable) is built at the END of the
sync before, behind the halo search, and the following sync uses it only if it was built for exactly the state that sync
starts from (csrc/domain.hip, queueLeafTable / tryResort).  Every case runs the same client loop through a domain that
sorts from scratch, a re-sorting domain with the early table, and a re-sorting domain without it (the default: the table
built in front of the encode), and compares them bit for bit after every sync; cstone_hip_domain_leaf_table_stats tells whether the early table
was used or had to be rejected."""
import numpy as np
import pytest

from resort_support import Loop, Motion, assert_same, environment

N, BUCKET = 20_000, 16


class Trio:
    """the three loops of a comparison in lockstep"""

    def __init__(self, ctx, monkeypatch, seed, kb=64, rb=64, curve=1, bc=(1, 1, 1), n=N):
        from cstone_amd.domain import Domain

        self.mp = monkeypatch
        self.ref = Loop(ctx, kb, rb, BUCKET, curve, n, seed, mode=Domain.SORT_FROM_SCRATCH, bc=bc)
        self.early = Loop(ctx, kb, rb, BUCKET, curve, n, seed, bc=bc)
        self.late = Loop(ctx, kb, rb, BUCKET, curve, n, seed, bc=bc)
        self.motion = Motion(seed + 100, periodic=all(bc))
        self.step = 0
        self.movers = 0

    def loops(self):
        return (self.ref, self.early, self.late)

    def switches(self, lp, **env):
        """the environment of one sync of lp: the early table on for the early loop alone, whatever the run has set"""
        on = "1" if lp is self.early else None
        return environment(CSTONE_EARLY_LEAF_TABLE=on, CSTONE_NO_EARLY_LEAF_TABLE=None, **env)

    def sync_one(self, lp):
        with self.switches(lp):
            lp.sync()

    def sync(self, move=True):
        """one step of the client: move (not before the first sync), sync, compare"""
        if move and self.step:
            drawn = self.motion.draw(self.ref)
            for lp in self.loops():
                self.motion.apply(lp, drawn)
        for lp in self.loops():
            self.sync_one(lp)
        for lp in (self.early, self.late):
            assert_same(lp, self.ref, (self.step, "late" if lp is self.late else "early"))
        self.step += 1
        self.movers += self.early.dom.stats()["last_movers"]
        return self

    def resorts(self):
        return self.early.dom.stats()["resorts"], self.late.dom.stats()["resorts"]

    def tables(self):
        """(used, rejected) of the early loop; the late loop never builds one"""
        assert self.late.dom.leaf_table_stats() == (0, 0)
        assert self.ref.dom.leaf_table_stats() == (0, 0)
        return self.early.dom.leaf_table_stats()


@pytest.mark.gpu
@pytest.mark.parametrize("kb,rb,curve", [(64, 64, 1), (32, 32, 0)])
def test_plain_loop_uses_the_table_of_the_sync_before(hip, monkeypatch, kb, rb, curve):
    t = Trio(hip, monkeypatch, 1, kb, rb, curve)
    for step in range(6):
        t.sync()
        assert t.resorts() == (step, step)  # one per steady sync
        assert t.tables() == (step, 0)      # ... each with the table the sync before left
    assert t.movers > 0


@pytest.mark.gpu
def test_two_domains_on_one_context_keep_their_own_tables(hip, monkeypatch):
    """the slots of the context's scalar block are shared by everything on the context: J of a table that waits for the next
    sync lives in the domain's own buffer"""
    a, b = Trio(hip, monkeypatch, 2), Trio(hip, monkeypatch, 3, n=N + 4321)
    for step in range(5):
        a.sync()
        b.sync()
        assert a.resorts() == (step, step) and b.resorts() == (step, step)
        assert a.tables() == (step, 0) and b.tables() == (step, 0)
    assert a.movers > 0 and b.movers > 0


@pytest.mark.gpu
def test_a_call_with_another_particle_count_spoils_the_table(hip, monkeypatch):
    """a sync refuses arrays of another length than the domain holds (particles leave through remove markers only); the
    table that waited for it is not trusted afterwards"""
    import torch

    import cstone_amd

    t = Trio(hip, monkeypatch, 4)
    t.sync().sync().sync()
    assert t.tables() == (2, 0)
    for change, rejected in ((7, 1), (-5, 2)):
        for lp in t.loops():
            m = lp.x.numel() + change
            grown = [torch.zeros(m, dtype=a.dtype, device="cuda") for a in (lp.keys, lp.x, lp.y, lp.z, lp.h)]
            for g, a in zip(grown, (lp.keys, lp.x, lp.y, lp.z, lp.h)):
                g[:min(m, a.numel())] = a[:min(m, a.numel())]
            with pytest.raises(cstone_amd.CstoneError, match="inconsistent"):
                lp.dom.sync(*grown, [torch.empty_like(grown[1]) for _ in range(4)])
        before = t.resorts()
        t.sync()
        assert t.resorts() == (before[0] + 1, before[1] + 1)
        assert t.tables() == (2 + (rejected - 1), rejected)
        t.sync()
        assert t.tables() == (2 + rejected, rejected)
    assert t.movers > 0


@pytest.mark.gpu
def test_remove_markers_shrink_the_table_with_the_particles(hip, monkeypatch):
    import torch

    t = Trio(hip, monkeypatch, 5)
    t.sync().sync()
    for step in range(2, 6):
        m = t.ref.x.numel()
        sel = torch.from_numpy(np.random.default_rng(step).choice(m, m // 100, replace=False)).cuda()
        for lp in t.loops():
            lp.keys[sel] = torch.iinfo(torch.int64).min  # bit pattern of endKey
        t.sync()
        assert t.ref.x.numel() == m - sel.numel()
        assert t.resorts() == (step, step)
        assert t.tables() == (step, 0)  # the table was built for the particles that stayed
    assert t.movers > 0


@pytest.mark.gpu
def test_a_sync_sorted_from_scratch_leaves_the_table_unused(hip, monkeypatch):
    t = Trio(hip, monkeypatch, 6)
    t.sync().sync().sync()
    assert t.tables() == (2, 0) and t.resorts() == (2, 2)
    for lp in (t.early, t.late):
        lp.dom.set_sort_mode(lp.dom.SORT_ALL_DIGITS)
    t.sync()
    assert t.tables() == (2, 1) and t.resorts() == (2, 2)  # rejected; and none is queued for a mode that never re-sorts
    for lp in (t.early, t.late):
        lp.dom.set_sort_mode(lp.dom.SORT_INCREMENTAL)
    t.sync()
    assert t.tables() == (2, 1) and t.resorts() == (3, 3)  # built in front of the encode, as without the early table
    t.sync()
    assert t.tables() == (3, 1) and t.resorts() == (4, 4)
    assert t.movers > 0


@pytest.mark.gpu
def test_arrays_permuted_by_the_caller(hip, monkeypatch):
    """every particle is a mover then: the attempt is given up behind a table that did fit, the domain backs off, and the
    re-sorts come back afterwards"""
    import torch

    t = Trio(hip, monkeypatch, 7)
    t.sync().sync().sync()
    perm = torch.from_numpy(np.random.default_rng(0).permutation(t.ref.x.numel())).cuda()
    for lp in t.loops():
        lp.x, lp.y, lp.z, lp.h, lp.ident = [a[perm].contiguous() for a in (lp.x, lp.y, lp.z, lp.h, lp.ident)]
    t.sync(move=False)
    assert t.resorts() == (2, 2) and t.early.dom.stats()["resort_fallbacks"] == 1
    assert t.tables() == (3, 0)
    for _ in range(6):
        t.sync()
    assert t.resorts()[0] == t.resorts()[1] >= 3
    used, rejected = t.tables()
    assert rejected == 0 and used > 3  # no table is queued while the domain backs off; then they are used again
    assert t.movers > 0


@pytest.mark.gpu
def test_open_box_whose_outermost_particle_moves(hip, monkeypatch):
    """the encode speculates on the box of the sync before; a particle that leaves it makes the attempt fall back and the
    following syncs measure first"""
    t = Trio(hip, monkeypatch, 8, bc=(0, 0, 0))
    t.sync().sync().sync()
    assert t.resorts() == (2, 2) and t.tables() == (2, 0)
    for lp in t.loops():
        at = int(lp.x.argmax())
        lp.x[at] += 0.05
    t.sync(move=False)
    assert t.early.dom.stats()["box_redos"] >= 1 and t.resorts() == (2, 2)
    for _ in range(4):
        t.sync()
    assert t.resorts()[0] == t.resorts()[1] > 2
    used, rejected = t.tables()
    assert used >= 3 and used + rejected <= t.step - 1
    assert t.movers > 0


@pytest.mark.gpu
def test_other_work_on_the_context_between_two_syncs(hip, monkeypatch):
    """sorts, scans, tree builds and a neighbour search use the context's scalar slots and its arena between the sync that
    built the table and the sync that reads it"""
    import torch

    import cstone_amd

    t = Trio(hip, monkeypatch, 9)
    box = cstone_amd.make_cbox([0, 1, 0, 1, 0, 1], (1, 1, 1))
    for step in range(5):
        t.sync()
        assert t.resorts() == (step, step) and t.tables() == (step, 0)
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
def test_a_failed_sync_spoils_the_table(hip, monkeypatch):
    """with the tests' build of the library: a sync whose device-side check word is raised fails at its end, behind the
    table it queued; the next sync builds its own"""
    import cstone_amd

    monkeypatch.setenv("CSTONE_HIP_LIB", cstone_amd.LIBPATH.replace("libcstone_hip.so", "libcstone_hip_hooks.so"))
    hooked = cstone_amd.Context(0)
    monkeypatch.delenv("CSTONE_HIP_LIB")
    assert hooked.lib.cstone_hip_test_hooks() == 1
    t = Trio(hooked, monkeypatch, 10)
    t.sync().sync().sync()
    assert t.tables() == (2, 0)
    # the same sync for all three (the trees take the same steps), on copies: a failed call leaves its arrays undefined.
    # Nothing moves before it, so the arrays of the loops stay in the order the domains hold
    for lp in t.loops():
        copies = [a.clone() for a in (lp.keys, lp.x, lp.y, lp.z, lp.h)]
        scratch, ident = [a.clone() for a in lp.scratch], lp.ident.clone()
        with t.switches(lp, CSTONE_FORCE_DEVICE_ERROR=None if lp is t.ref else "1"):
            if lp is t.ref:
                lp.dom.sync(*copies, scratch, [ident])
            else:
                with pytest.raises(cstone_amd.CstoneError, match="device-side check failed"):
                    lp.dom.sync(*copies, scratch, [ident])
        hooked.sync()
    assert t.tables() == (3, 0) and t.resorts() == (3, 3)
    t.sync()
    assert t.tables() == (3, 1) and t.resorts() == (4, 4)  # queued by the failed sync, not trusted
    t.sync()
    assert t.tables() == (4, 1) and t.resorts() == (5, 5)
    assert t.movers > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kb,rb,curve", [(64, 64, 1), (32, 32, 0)])
def test_movers_placed_ahead_of_the_read_back(hip, kb, rb, curve):
    """CSTONE_EARLY_PLACE=1 (csrc/resort.hpp, placeMoversEarly): the placement kernel reads the mover count and the flags
    on the device and runs while the host decides.  A steady loop, removals (the markers' bin lies behind the movers) and
    an attempt that overflows the mover list and must place nothing, against a domain that sorts from scratch"""
    import torch

    from cstone_amd.domain import Domain

    ref = Loop(hip, kb, rb, BUCKET, curve, N, 12, mode=Domain.SORT_FROM_SCRATCH)
    lp = Loop(hip, kb, rb, BUCKET, curve, N, 12)
    motion = Motion(112)
    movers = 0
    for step in range(10):
        if step:
            drawn = motion.draw(ref)
            for one in (ref, lp):
                motion.apply(one, drawn)
        if step == 3:
            m = ref.x.numel()
            sel = torch.from_numpy(np.random.default_rng(step).choice(m, m // 100, replace=False)).cuda()
            for one in (ref, lp):
                one.keys[sel] = torch.iinfo(one.kdt).min if kb == 64 else (1 << 30)  # bit pattern of endKey
        if step == 4:
            perm = torch.from_numpy(np.random.default_rng(0).permutation(ref.x.numel())).cuda()
            for one in (ref, lp):
                one.x, one.y, one.z, one.h, one.ident = [a[perm].contiguous() for a in (one.x, one.y, one.z, one.h, one.ident)]
        ref.sync()
        with environment(CSTONE_EARLY_PLACE="1", CSTONE_NO_EARLY_PLACE=None):
            lp.sync()
        assert_same(lp, ref, step)
        st = lp.dom.stats()
        if step <= 3:
            assert st["resorts"] == step, (step, st)
            movers += st["last_movers"]
        if step == 4:
            assert st["resort_fallbacks"] == 1 and st["resorts"] == 3, st
    assert lp.dom.stats()["resorts"] >= 4 and movers > 0  # the back-off of four syncs has run out
