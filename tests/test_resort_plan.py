"""The DECISIONS of the incremental re-sort of Domain::sync (csrc/resort.hpp; classify in encodeResortKernel, csrc/sfc.hip;
binMoversKernel, newLeafSizesKernel, checkTilesKernel in csrc/resort.hip; tryResort in csrc/domain.hip) against a numpy
model of them (resort_plan_support.plan).  The re-sort returns the stable sort whatever its stages decide, so the tests
that compare its RESULT with a sort from scratch (test_resort.py and its neighbours) cannot see a stayer taken for a
mover, a limit raised a slot early, or an attempt given up for nothing: those only cost time.  Here the number of movers
(cstone_hip_domain_stats: last_movers) and the fate of every attempt (resorts, resort_fallbacks, the four syncs of
back-off) are predicted from the previous sync's view and the arrays handed over, and compared with ==.  Every case also
runs a twin domain that sorts from scratch and compares everything bit for bit: a limit raised a slot LATE shows there.

Every scenario is a function of a driver: the Tracker (two domains on the GPU) or the Sim (no library: the model alone
on leaves kept on the host).  The CPU tests run the scenarios on the Sim: they check that the rule is sufficient (stayers
and arrivals ordered leaf by leaf are the stable sort) and that each scenario's plan differs from that of one wrong
restatement of the rule (plan(variant=...)), i.e. that the GPU case would notice that defect in the kernels.  Each edge
case asserts its own premise on the plan before the library runs."""
import numpy as np
import pytest

import resort_plan_support as S
from resort_support import environment

N_CLOUD = 20_000


class Make:
    """drivers for the scenarios: Trackers on a context, or Sims"""

    def __init__(self, oracle, ctx=None):
        self.oracle, self.ctx = oracle, ctx

    def __call__(self, kb, rb, bucket_focus, curve, **kw):
        if self.ctx is None:
            return S.Sim(self.oracle, kb, rb, bucket_focus, curve, **kw)
        return S.Tracker(self.ctx, self.oracle, kb, rb, bucket_focus, curve, **kw)


class Witness:
    """the inputs of one planned sync of a scenario, to be planned again under a wrong rule"""

    def __init__(self, drv, p):
        self.inputs, self.kb, self.bucket_focus, self.plan = drv.inputs, drv.kb, drv.bucket_focus, p

    def under(self, variant):
        return S.plan(*self.inputs, self.kb, self.bucket_focus, variant=variant)


# ----------------------------------------------------------------------------------------------------------------------
# scenarios
# ----------------------------------------------------------------------------------------------------------------------
def random_cloud(make, kb, rb, curve, bucket_focus, n, syncs=6):
    """the common cloud and motion; -> attempts made"""
    drv = make(kb, rb, bucket_focus, curve, n=n, seed=n + kb + bucket_focus)
    attempts = 0
    for step in range(syncs):
        if step:
            drv.move()
        attempted, _ = drv.sync(what=("cloud", n, step))
        attempts += attempted
    return drv, attempts


def start_lattice(make, kb, rb, curve, bucket_focus, per_leaf=None):
    """the lattice after its first sync, and the premise of every lattice case: 512 leaves of level 3 with 64 particles
    each (or what per_leaf keeps of them), in the order of their keys"""
    pos, h = S.lattice(make.oracle, kb, curve, per_leaf)
    drv = make(kb, rb, bucket_focus, curve, pos=pos, h=h)
    drv.sync(what="lattice, first sync")
    s = drv.state()
    want = np.full(512, 64)
    for cell, count in (per_leaf or {}).items():
        want[cell] = count
    assert np.array_equal(s.tree, np.arange(513, dtype=np.uint64) * np.uint64(S.end_key(kb) // 512))
    assert np.array_equal(s.counts, want)
    return drv, s


EDGE_LEAVES = [0, 1, 2, 31, 62, 63, 64, 65, 127, 128, 200, 255, 256, 300, 383, 447, 448, 449, 500, 509, 510, 511]


def key_edges(make, kb, rb, curve):
    """one particle of a leaf onto (a) the leaf's first key, (b) its last key, (c) the next leaf's first key, (d) the
    previous leaf's last key -- for leaves at the edges and inside of first, last and interior tiles"""
    drv, s = start_lattice(make, kb, rb, curve, 64)
    who, keys, moves = [], [], []
    for l in EDGE_LEAVES:
        lo, hi = int(s.tree[l]), int(s.tree[l + 1])
        cases = [(lo, False), (hi - 1, False)] + ([(hi, True)] if l < 511 else []) + ([(lo - 1, True)] if l > 0 else [])
        for k, (key, leaves) in enumerate(cases):
            who.append(64 * l + k), keys.append(key), moves.append(leaves)
    S.send(drv, s, who, keys)
    expect = np.zeros(s.n, dtype=bool)
    expect[who] = moves

    def premise(attempted, p):
        assert attempted
        assert np.array_equal(drv.inputs[2][who], np.array(keys, dtype=np.uint64))  # every particle has the key it is meant to
        assert np.array_equal(p.mover, expect) and p.movers == sum(moves) == 2 * len(EDGE_LEAVES) - 2
        assert p.accepted

    _, p = drv.sync(premise, "key edges")
    w = Witness(drv, p)
    drv.sync(what="key edges, quiet sync behind")
    return w


def empty_ranges(make, kb=64, rb=64, curve=1):
    """every eighth leaf emptied; once the re-sort has resumed, one particle of the leaf in front of each empty one moves
    into the empty cell: the range of a compact leaf runs over the empty leaves behind it, the particle stays"""
    drv, s = start_lattice(make, kb, rb, curve, 64)
    emptied = list(range(3, 512, 8))
    # particle k of the e-th emptied leaf goes to a leaf 4 + 8 k further on (none of the emptied ones), to the e-th of 64
    # places spread over that leaf: the leaf splits once at the next update and none of its children stays empty
    span = int(s.tree[1])
    who, keys = [], []
    for e, l in enumerate(emptied):
        for k in range(64):
            who.append(64 * l + k), keys.append(int(s.tree[(l + 4 + 8 * k) % 512]) + e * (span // 64) + 1)
    S.send(drv, s, who, keys)

    def premise_emptying(attempted, p):
        # an eighth of the particles move, which the list takes, and every tile keeps its 4096 old slots and gets 512
        # arrivals: given up
        assert attempted and p.movers == 64 * 64 == s.n // 8 and not p.leaf_flag and not p.list_flag
        assert p.tile_flag and np.all(p.slots_tile == 4096 + 512) and not p.accepted

    drv.sync(premise_emptying, "emptying")
    for k in range(S.BACKOFF_SYNCS):
        drv.sync(lambda attempted, p: _assert(not attempted), ("back-off", k))
    drv.sync(lambda attempted, p: _assert(attempted and p.movers == 0 and p.accepted), "resumed")

    s2 = drv.state()
    empty = np.nonzero(s2.counts == 0)[0]
    assert np.array_equal(s2.tree[empty], s.tree[emptied]) and np.all(s2.counts[empty - 1] > 0)
    who = [int(s2.layout[l]) - 1 for l in empty]  # the last particle of the leaf in front
    keys = [int(s2.tree[l]) for l in empty]  # the first key of the empty leaf
    S.send(drv, s2, who, keys)

    def premise(attempted, p):
        assert attempted and np.array_equal(drv.inputs[2][who], np.array(keys, dtype=np.uint64))
        assert np.array_equal(s2.leaf_of(np.array(who)), empty - 1)
        assert p.movers == 0 and not p.mover.any() and p.accepted

    _, p = drv.sync(premise, "into the empty cells")
    w = Witness(drv, p)
    drv.sync(what="into the empty cells, quiet sync behind")
    return w


def _assert(cond):
    assert cond


def back_off_then_resume(drv, what):
    """after an attempt that was given up: four syncs that do not try, the fifth tries again (nothing moves: accepted)"""
    for k in range(S.BACKOFF_SYNCS):
        before = dict(drv.schedule.expected)
        drv.sync(lambda attempted, p: _assert(not attempted), (what, "back-off", k))
        assert drv.schedule.expected == before
    before = dict(drv.schedule.expected)
    drv.sync(lambda attempted, p: _assert(attempted and p.movers == 0 and p.accepted), (what, "resumed"))
    assert drv.schedule.expected == dict(before, resorts=before["resorts"] + 1, last_movers=0)


def leaf_limit(make, bucket_focus, where, extra):
    """a leaf of 64 filled from far leaves to exactly 255 slots (accepted) or 256 (given up).  bucket_focus 64, 128, 200:
    64, 32, 16 leaves per tile; the leaf is the first or the last of the second tile.  With 64 leaves per tile a tile of
    full leaves has 4096 old slots and takes 128 arrivals only: three other leaves of that tile start with 16 particles
    instead of 64, so that the tile stays under ITS limit (4143 or 4144 slots) and the leaf's alone decides"""
    G = S.leaves_per_tile(bucket_focus)
    thinned = {70: 16, 80: 16, 90: 16} if G == 64 else None
    drv, s = start_lattice(make, 64, 64, 1, bucket_focus, thinned)
    target = G if where == "first" else 2 * G - 1
    arrivals = S.LEAF_CAP - 1 - 64 + extra
    who = S.donors(s, range(G, 2 * G), arrivals)
    S.send(drv, s, who, S.keys_inside(s, target, arrivals))

    def premise(attempted, p):
        assert attempted and p.leaves_per_tile == G and p.J == 512
        assert p.slots_leaf[target] == 255 + extra and np.all(np.delete(p.slots_leaf, target) <= 64)
        assert p.movers == arrivals and p.leaf_flag == bool(extra) and not p.tile_flag and not p.list_flag
        assert p.slots_tile.max() == p.slots_tile[1] <= S.TILE_SLOTS
        assert p.accepted == (not extra)

    _, p = drv.sync(premise, ("leaf limit", bucket_focus, where, extra))
    w = Witness(drv, p)
    if extra:
        back_off_then_resume(drv, "leaf limit")
    else:
        drv.sync(lambda attempted, p: _assert(attempted), "leaf limit, sync behind")
    return w


def tile_limit(make, bucket_focus, which, extra):
    """a tile filled from far leaves to exactly 4224 slots (accepted) or 4225 (given up), spread evenly over its leaves.
    Three cells of the lattice are empty: 509 compact leaves, so the last tile is short (61 leaves of 64, 29 of 32) and
    the compact leaves are not the leaves of the tree"""
    G = S.leaves_per_tile(bucket_focus)
    drv, s = start_lattice(make, 64, 64, 1, bucket_focus, {5: 0, 100: 0, 300: 0})
    compact = S.compact_leaves(s)
    J = compact.size
    assert J == 509 and J % G != 0
    tile = 0 if which == "first" else J // G
    targets = compact[tile * G:min(tile * G + G, J)]
    old = int(s.counts[targets].sum())
    assert old == 64 * (G if which == "first" else J % G)
    arrivals = S.TILE_SLOTS - old + extra
    per_leaf = np.bincount(np.arange(arrivals) % targets.size, minlength=targets.size)
    keys = [key for l, c in zip(targets, per_leaf) for key in S.keys_inside(s, int(l), int(c))]
    who = S.donors(s, targets, arrivals)
    S.send(drv, s, who, keys)

    def premise(attempted, p):
        assert attempted and p.leaves_per_tile == G and p.J == J
        assert p.slots_tile[tile] == S.TILE_SLOTS + extra and np.all(np.delete(p.slots_tile, tile) <= 64 * G)
        assert p.movers == arrivals <= s.n // 8 and not p.leaf_flag and not p.list_flag and p.tile_flag == bool(extra)
        assert p.accepted == (not extra)

    _, p = drv.sync(premise, ("tile limit", bucket_focus, which, extra))
    w = Witness(drv, p)
    if extra:
        back_off_then_resume(drv, "tile limit")
    else:
        drv.sync(lambda attempted, p: _assert(attempted), "tile limit, sync behind")
    return w


def _spread(s, m, G):
    """destination leaves for m arrivals that keep every tile and every leaf of the state under its limit: tiles take
    arrivals in proportion to the room they have, at most 100 per leaf (64 + 100 < 256); -> tree leaf per arrival"""
    compact = S.compact_leaves(s)
    starts = np.arange(0, compact.size, G)
    leaves_in = np.diff(np.append(starts, compact.size))
    room = np.minimum(S.TILE_SLOTS - np.add.reduceat(s.counts[compact], starts), 100 * leaves_in)
    assert s.counts.max() <= 64 and room.min() >= 0 and room.sum() >= m
    share = m * room // room.sum()
    for t in range(starts.size):  # the remainder, where there is room left
        add = min(m - int(share.sum()), int(room[t] - share[t]))
        share[t] += add
    assert share.sum() == m
    dest = [compact[starts[t] + np.arange(share[t]) % leaves_in[t]] for t in range(starts.size)]
    return np.sort(np.concatenate(dest))


def mover_share(make, extra):
    """exactly n / 8 particles leave their leaves for leaves that stay under both limits (accepted), one more (given up:
    too many), 1025 more (the list overflows: given up; the sync behind the back-off re-sorts)"""
    drv = make(64, 64, 64, 1, n=N_CLOUD, seed=3)
    drv.sync()
    drv.sync(lambda attempted, p: _assert(attempted and p.movers == 0 and p.accepted), "mover share, quiet")
    s = drv.state()
    m = s.n // 8 + extra
    who = np.sort(S.donors(s, [], m))
    dest = np.roll(_spread(s, m, 64), m // 2)
    assert np.all(s.leaf_of(who) != dest)
    order = np.argsort(dest, kind="stable")
    leaves, counts = np.unique(dest, return_counts=True)
    keys = [key for l, c in zip(leaves, counts) for key in S.keys_inside(s, int(l), int(c))]
    S.send(drv, s, who[order], keys)

    def premise(attempted, p):
        assert attempted and p.movers == m and p.markers == 0
        assert not p.leaf_flag and not p.tile_flag and p.list_flag == (extra > S.LIST_EXTRA)
        assert p.accepted == (extra == 0)

    _, p = drv.sync(premise, ("mover share", extra))
    w = Witness(drv, p)
    if extra:
        back_off_then_resume(drv, "mover share")
    else:
        drv.sync(lambda attempted, p: _assert(attempted), "mover share, sync behind")
    return w


def markers(make, kb, rb):
    """every 97th particle marked for removal next to the common motion: the markers are movers, the arrays shrink, the
    next plan is made for the shrunk arrays"""
    drv = make(kb, rb, 64, 1, n=N_CLOUD, seed=5)
    drv.sync()
    drv.move()
    drv.sync(what="markers, before")
    s = drv.state()
    marks = np.zeros(s.n, dtype=bool)
    marks[::97] = True
    drv.move()
    moved = drv.state()
    drv.put(moved.x, moved.y, moved.z, marks)

    def premise(attempted, p):
        assert attempted and p.markers == marks.sum() == 207 and np.all(p.mover[marks]) and p.movers > p.markers
        assert np.all(p.dest[marks] == p.J) and p.incoming[p.J] == 207 and p.accepted

    _, p = drv.sync(premise, "markers")
    assert drv.schedule.expected["last_movers"] == p.movers
    after = drv.state()
    assert after.n == s.n - 207 and after.layout[-1] == after.n
    drv.move()
    drv.sync(lambda attempted, p: _assert(attempted and p.markers == 0 and p.mover.size == after.n), "markers, behind")
    return drv


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the model alone
# ----------------------------------------------------------------------------------------------------------------------
CLOUD_CONFIGS = ([(kb, rb, 1, 64) for kb, rb in ((64, 64), (64, 32), (32, 32), (32, 64))]
                 + [(64, 64, 0, 64), (32, 32, 0, 64)]
                 + [(64, 64, 1, b) for b in (8, 100, 200)])
CLOUD_SIZES = [1, 3, 65, 257, 4099, N_CLOUD]


def test_leaves_per_tile_and_what_cannot_be_reached():
    assert [S.leaves_per_tile(b) for b in (1, 8, 64, 65, 128, 129, 200, 255, 256, 1000)] == [64, 64, 64, 32, 32, 16, 16, 16, 0, 0]
    # 16 leaves of fewer than 256 slots stay below the tile's limit: there is no tile-limit case for 16 leaves per tile
    assert 16 * (S.LEAF_CAP - 1) < S.TILE_SLOTS
    # ... while 32 and 64 leaves can reach it with every leaf under its own limit
    assert 32 * (S.LEAF_CAP - 1) > S.TILE_SLOTS and 64 * (S.LEAF_CAP - 1) > S.TILE_SLOTS


def test_model_on_a_table_worked_by_hand():
    """five leaves, the third empty, ten particles; 32-bit keys"""
    e = S.end_key(32)
    tree = np.array([0, e // 8, 2 * e // 8, 3 * e // 8, 4 * e // 8, e], dtype=np.uint64)
    layout = np.array([0, 3, 5, 5, 8, 10])
    keys = np.array([0, e // 8 - 1, e // 8,  # leaf 0: stays, stays (last key), leaves for compact leaf 1
                     e // 8, 3 * e // 8 - 1,  # leaf 1: stays (first key), stays (inside the empty leaf behind it)
                     3 * e // 8, 3 * e // 8 - 1, e,  # leaf 3: stays, leaves for compact leaf 1, marker
                     e - 1, 0], dtype=np.uint64)  # leaf 4: stays, leaves for compact leaf 0
    p = S.plan(tree, layout, keys, 32, 64)
    assert p.J == 4 and p.mover.tolist() == [False, False, True, False, False, False, True, True, False, True]
    assert (p.movers, p.markers) == (4, 1) and p.incoming.tolist() == [1, 2, 0, 0, 1]
    assert p.slots_leaf.tolist() == [4, 4, 3, 2] and p.slots_tile.tolist() == [13]
    assert not (p.leaf_flag or p.tile_flag or p.list_flag) and not p.accepted  # 4 movers > 10 / 8
    assert np.array_equal(S.order_from_plan(p, keys), np.argsort(keys, kind="stable"))
    assert S.plan(tree, layout, keys, 32, 64, variant="own_leaf_only_range").mover.tolist()[4]
    assert S.plan(tree, layout, keys, 32, 64, variant="lo_exclusive").mover.tolist()[3]
    assert not S.plan(tree, layout, keys, 32, 64, variant="hi_inclusive").mover.tolist()[2]


@pytest.mark.parametrize("kb,rb,curve,bucket_focus", CLOUD_CONFIGS)
def test_rule_is_sufficient_on_the_clouds(oracle, kb, rb, curve, bucket_focus):
    """(the Sim asserts it at every planned sync: order_from_plan == stable argsort)"""
    for n in CLOUD_SIZES:
        _, attempts = random_cloud(Make(oracle), kb, rb, curve, bucket_focus, n)
        assert attempts >= 2, n


def test_rule_is_sufficient_on_the_edge_cases(oracle):
    make = Make(oracle)
    key_edges(make, 32, 32, 0)
    for G_bucket in (64, 128, 200):
        leaf_limit(make, G_bucket, "last", 1)
    tile_limit(make, 128, "last", 1)
    mover_share(make, 1025)
    markers(make, 64, 64)
    markers(make, 32, 32)


# variant -> the named case of the GPU list that tells it from the true rule
TELLS = {
    "lo_exclusive": lambda make: key_edges(make, 64, 64, 1),
    "hi_inclusive": lambda make: key_edges(make, 32, 32, 1),
    "rank_of_next_word": lambda make: key_edges(make, 64, 64, 0),
    "leaf_cap_255": lambda make: leaf_limit(make, 64, "first", 0),
    "tile_4223": lambda make: tile_limit(make, 64, "last", 0),
    "accept_lt": lambda make: mover_share(make, 0),
    "own_leaf_only_range": lambda make: empty_ranges(make),
}


@pytest.mark.parametrize("variant", S.VARIANTS)
def test_premise_every_wrong_rule_is_told_apart(oracle, variant):
    w = TELLS[variant](Make(oracle))
    wrong = w.under(variant)
    assert (wrong.movers, wrong.accepted) != (w.plan.movers, w.plan.accepted), variant


def test_premise_which_cases_tell_which_wrong_rule(oracle):
    """the limits from both sides: the accepted case of a limit tells the rule that raises it a slot early, and the case
    one beyond it is given up under the true rule too (a rule a slot LATE is the twin domain's to catch)"""
    make = Make(oracle)
    for bucket_focus in (64, 128, 200):
        for where in ("first", "last"):
            w = leaf_limit(make, bucket_focus, where, 0)
            assert w.plan.accepted and not w.under("leaf_cap_255").accepted
    for bucket_focus in (64, 128):
        for which in ("first", "last"):
            w = tile_limit(make, bucket_focus, which, 0)
            assert w.plan.accepted and not w.under("tile_4223").accepted
            assert not tile_limit(make, bucket_focus, which, 1).plan.accepted
    w = key_edges(make, 32, 32, 1)
    assert w.under("lo_exclusive").movers == w.plan.movers + len(EDGE_LEAVES)  # the (a) particles
    assert w.under("hi_inclusive").movers == w.plan.movers - (len(EDGE_LEAVES) - 1)  # the (c) particles
    w = empty_ranges(make)
    assert w.under("own_leaf_only_range").movers == 64
    w = mover_share(make, 0)
    assert w.plan.accepted and not w.under("accept_lt").accepted
    assert not mover_share(make, 1).plan.accepted


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the library against the model
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", CLOUD_SIZES)
@pytest.mark.parametrize("kb,rb,curve,bucket_focus", CLOUD_CONFIGS)
def test_random_clouds(hip, oracle, kb, rb, curve, bucket_focus, n):
    """n = 1, 3: the whole cloud in the encode's scalar tail and in a partial first word of the leaf table; 4099: a tail
    behind the last full vector"""
    _, attempts = random_cloud(Make(oracle, hip), kb, rb, curve, bucket_focus, n)
    assert attempts >= 2  # (a guard against a case that compares nothing; the comparisons are the Tracker's, all ==)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["stride", "tile"])
def test_random_cloud_in_either_encode_order(hip, oracle, order):
    with environment(CSTONE_ENCODE_ORDER=order):
        _, attempts = random_cloud(Make(oracle, hip), 64, 64, 1, 64, N_CLOUD)
    assert attempts >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("kb,rb", [(64, 64), (32, 32)])
def test_key_edges(hip, oracle, kb, rb, curve):
    key_edges(Make(oracle, hip), kb, rb, curve)


@pytest.mark.gpu
def test_ranges_over_empty_leaves(hip, oracle):
    empty_ranges(Make(oracle, hip))


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1], ids=["255-accepted", "256-given-up"])
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("bucket_focus", [64, 128, 200])
def test_leaf_limit(hip, oracle, bucket_focus, where, extra):
    leaf_limit(Make(oracle, hip), bucket_focus, where, extra)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1], ids=["4224-accepted", "4225-given-up"])
@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("bucket_focus", [64, 128])
def test_tile_limit(hip, oracle, bucket_focus, which, extra):
    tile_limit(Make(oracle, hip), bucket_focus, which, extra)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1, 1025], ids=["eighth-accepted", "eighth+1-given-up", "list-overflow"])
def test_mover_share(hip, oracle, extra):
    mover_share(Make(oracle, hip), extra)


@pytest.mark.gpu
@pytest.mark.parametrize("kb,rb", [(64, 64), (32, 32)])
def test_markers(hip, oracle, kb, rb):
    drv = markers(Make(oracle, hip), kb, rb)
    assert drv.lp.dom.view().end_index == N_CLOUD - 207


@pytest.mark.gpu
def test_bucket_256_never_attempts(hip, oracle):
    drv = Make(oracle, hip)(64, 64, 256, 1, n=N_CLOUD, seed=9)
    for step in range(4):
        if step:
            drv.move()
        drv.sync(lambda attempted, p: _assert(not attempted), ("bucket 256", step))
        st = drv.lp.dom.stats()
        assert (st["resorts"], st["resort_fallbacks"], st["last_movers"]) == (0, 0, 0)


@pytest.mark.gpu
def test_unaligned_arrays_do_not_attempt(hip, oracle):
    """arrays offset by one element (test_resort.py::test_unaligned_arrays_take_the_regular_path): the vector encode does
    not take them -- no attempt, no fallback counted, no back-off started: the first aligned sync behind them re-sorts"""
    import torch

    import cstone_amd
    from cstone_amd.domain import Domain

    n = N_CLOUD + 1
    drv = Make(oracle, hip)(64, 64, 64, 1, n=n, seed=11)
    drv.sync()
    for lp, mode in zip(drv.loops(), (Domain.SORT_INCREMENTAL, Domain.SORT_FROM_SCRATCH)):
        # views shifted by one element (8 bytes): the client dropped its first particle; a new domain, since the old one
        # insists on the size of its last sync
        lp.keys, lp.x, lp.y, lp.z, lp.h, lp.ident = [t[1:] for t in (lp.keys, lp.x, lp.y, lp.z, lp.h, lp.ident)]
        lp.scratch = [torch.empty(n, dtype=lp.x.dtype, device="cuda")[1:] for _ in range(4)]
        lp.dom = Domain(hip, 1, 64, 64, 256, 64, 0.5, cstone_amd.make_cbox([0, 1, 0, 1, 0, 1], (1, 1, 1)))
        lp.dom.set_sort_mode(mode)
    drv.schedule = S.Schedule(64)
    for step in range(4):
        if step:
            drv.move()
        assert drv.lp.x.data_ptr() % 16 == 8
        drv.sync(lambda attempted, p: _assert(not attempted), ("unaligned", step))
        st = drv.lp.dom.stats()
        assert (st["resorts"], st["resort_fallbacks"], st["last_movers"]) == (0, 0, 0)
    # the client moves to aligned arrays: no back-off is pending, the next sync tries and is accepted
    for lp in drv.loops():
        lp.resize()
    drv.move()
    drv.sync(lambda attempted, p: _assert(attempted and p.accepted), "aligned again")
    assert drv.lp.dom.stats()["resorts"] == 1
