"""TEST INFRASTRUCTURE for tests/test_resort_plan.py: a numpy model of the DECISIONS of the incremental re-sort of
Domain::sync -- who is a mover, where movers go, which limit is hit, whether the attempt is accepted, which syncs attempt
at all -- a Tracker that follows a Loop of resort_support.py and compares the model with cstone_hip_domain_stats, a CPU
stand-in for that pair, and the clouds and moves that place leaves, tiles and mover counts exactly on the limits.  Not a
test module.

The model.  Written from csrc/resort.hpp (ResortArgs, the RESORT_* limits, LeafResort::leavesPerTile), the rule of
csrc/host_rules.hpp (resortAccepted, RESORT_BACKOFF_SYNCS) and DESIGN.md section 4b; all key arithmetic in uint64,
everything a searchsorted, a bincount or a reduceat.  It shares no code with the library and uses nothing of the oracle
but compute_sfc_keys (the keys of the positions a client hands to a sync).  The previous sync's view gives
focus_leaves[L + 1] and layout[L + 1]; the client hands over its arrays in array order:
  compact leaves  the J non-empty leaves.  leafLo[0] = 0, leafLo[j] = first key of the j-th non-empty leaf, leafLo[J] =
                  endKey; leafPos[j] = its first position, leafPos[J] = n.  The key range of a compact leaf runs over the
                  empty leaves behind it
  new keys        of the new positions in the sync's box; a particle whose old key is the remove marker keeps endKey
  classification  position p belongs to compact leaf j(p), the last j with leafPos[j] <= p; it is a STAYER iff
                  leafLo[j] <= key < leafLo[j + 1], a mover otherwise.  Markers are always movers
  destination     a mover goes to the last j in [0, J] with leafLo[j] <= key, markers to entry J
  leaf limit      raised if some j < J has old[j] + incoming[j] >= 256 (old: the leaf's old positions, holes included)
  tile limit      tiles are G = leavesPerTile(bucketFocus) consecutive compact leaves; raised if old + arrivals > 4224
  list limit      raised if movers > n / 8 + 1024
  accepted        no limit raised and movers <= n / 8
plan(variant=...) restates one WRONG rule at a time; the variants never judge the library, they show that the cases of
test_resort_plan.py tell every such mistake from the true rule."""
import types

import numpy as np

from resort_support import Loop, assert_same

MAX_LEVEL = {32: 10, 64: 21}
KEY_DTYPE = {32: np.uint32, 64: np.uint64}
REAL_DTYPE = {32: np.float32, 64: np.float64}

# csrc/resort.hpp, csrc/host_rules.hpp
LEAF_CAP = 256  # a leaf must hold FEWER slots
TILE_SLOTS = 4224  # a tile may hold this many
BACKOFF_SYNCS = 4
LIST_EXTRA = 1024  # the mover list holds n / 8 + this many

VARIANTS = ("lo_exclusive", "hi_inclusive", "rank_of_next_word", "leaf_cap_255", "tile_4223", "accept_lt",
            "own_leaf_only_range")

_u64 = np.uint64


def end_key(kb):
    return 1 << (3 * MAX_LEVEL[kb])


def leaves_per_tile(bucket_focus):
    """LeafResort::leavesPerTile: 0 = buckets this large are not re-sorted"""
    if bucket_focus <= 64:
        return 64
    if bucket_focus <= 128:
        return 32
    return 16 if bucket_focus < LEAF_CAP else 0


def plan(focus_leaves, layout, keys_new, kb, bucket_focus, variant=None):
    """what a re-sort attempt decides for keys_new[n] (unsigned, in array order, endKey = remove marker) on the leaves and
    the layout of the previous sync"""
    assert variant is None or variant in VARIANTS
    tree = np.asarray(focus_leaves).astype(_u64)
    layout = np.asarray(layout).astype(np.int64)
    keys = np.asarray(keys_new).astype(_u64)
    n, end = keys.size, _u64(end_key(kb))
    assert tree.size == layout.size and layout[0] == 0 and layout[-1] == n and tree[0] == 0 and tree[-1] == end

    nonempty = np.nonzero(np.diff(layout) > 0)[0]
    J = nonempty.size
    leaf_lo = np.concatenate([[_u64(0)], tree[nonempty[1:]], [end]]).astype(_u64)
    leaf_pos = np.concatenate([layout[nonempty], [n]])
    hi = tree[nonempty + 1] if variant == "own_leaf_only_range" else leaf_lo[1:]

    p = np.arange(n, dtype=np.int64)
    at = p + 64 if variant == "rank_of_next_word" else p
    own = np.minimum(np.searchsorted(leaf_pos[:J], at, side="right") - 1, J - 1)
    above = keys > leaf_lo[own] if variant == "lo_exclusive" else keys >= leaf_lo[own]
    below = keys <= hi[own] if variant == "hi_inclusive" else keys < hi[own]
    marker = keys == end
    mover = ~(above & below) | marker

    dest = np.searchsorted(leaf_lo, keys, side="right") - 1
    assert np.all(dest[marker] == J) and np.all(dest[~marker] < J)
    incoming = np.bincount(dest[mover], minlength=J + 1)
    old = np.diff(leaf_pos)
    slots_leaf = old + incoming[:J]
    G = leaves_per_tile(bucket_focus)
    slots_tile = np.add.reduceat(slots_leaf, np.arange(0, J, G)) if G else np.zeros(0, dtype=np.int64)

    movers = int(mover.sum())
    leaf_flag = bool(np.any(slots_leaf >= (LEAF_CAP - 1 if variant == "leaf_cap_255" else LEAF_CAP)))
    tile_flag = bool(np.any(slots_tile > (TILE_SLOTS - 1 if variant == "tile_4223" else TILE_SLOTS)))
    list_flag = movers > n // 8 + LIST_EXTRA
    few = movers < n // 8 if variant == "accept_lt" else movers <= n // 8
    return types.SimpleNamespace(J=J, mover=mover, movers=movers, markers=int(marker.sum()), own=own, dest=dest,
                                 incoming=incoming, slots_leaf=slots_leaf, slots_tile=slots_tile, leaves_per_tile=G,
                                 leaf_flag=leaf_flag, tile_flag=tile_flag, list_flag=list_flag,
                                 accepted=few and not (leaf_flag or tile_flag or list_flag))


def order_from_plan(p, keys_new):
    """the order the re-sort's rule produces: per compact leaf its stayers and its arrivals by (key, old index), leaf after
    leaf, the markers behind them in index order"""
    group = np.where(p.mover, p.dest, p.own)
    return np.lexsort((np.arange(keys_new.size), np.asarray(keys_new).astype(_u64), group))


# ----------------------------------------------------------------------------------------------------------------------
# drivers: a pair of loops on the GPU (Tracker), or the same bookkeeping without a library (Sim)
# ----------------------------------------------------------------------------------------------------------------------
class Schedule:
    """which syncs attempt (csrc/domain.hip, tryResort) and what an attempt does to the three counters"""

    def __init__(self, bucket_focus, incremental=True):
        self.bucket_focus, self.incremental = bucket_focus, incremental
        self.syncs, self.backoff = 0, 0
        self.expected = dict(resorts=0, resort_fallbacks=0, last_movers=0)

    def step(self, aligned, make_plan):
        """-> (attempted, plan or None); the counters and the back-off move as the library's must"""
        attempt = (self.syncs > 0 and leaves_per_tile(self.bucket_focus) > 0 and self.backoff == 0 and self.incremental)
        if self.backoff > 0:
            self.backoff -= 1
        self.syncs += 1
        if not (attempt and aligned):
            return False, None
        p = make_plan()
        if p.accepted:
            self.expected["resorts"] += 1
            self.expected["last_movers"] = p.movers
        else:
            self.expected["resort_fallbacks"] += 1
            self.backoff = BACKOFF_SYNCS
        return True, p


class State:
    """what a client holds between two syncs, on the host: its arrays in the order of the last sync, the keys that sync
    returned, and the leaves and the layout of its view"""

    def __init__(self, x, y, z, keys, tree, layout):
        self.x, self.y, self.z, self.keys, self.tree, self.layout = x, y, z, keys, tree, layout
        self.n = x.size
        self.counts = np.diff(layout)

    def leaf_of(self, index):
        return np.searchsorted(self.layout, index, side="right") - 1


def _aligned(loop):
    """the vector encode takes arrays on 16-byte boundaries, the keys on a vector of as many keys as a lane has reals"""
    vec = 16 // (loop.rb // 8)
    return (all(t.data_ptr() % 16 == 0 for t in (loop.x, loop.y, loop.z))
            and loop.keys.data_ptr() % (vec * loop.kb // 8) == 0)


class Tracker:
    """follows one Loop next to a twin that sorts from scratch.  sync(): the plan for the arrays about to be handed over
    on the previous view, the predicted counters (back-off included), the premise of the case asserted on the plan BEFORE
    the library runs, then both syncs, the counters compared with ==, the results compared bit for bit"""

    def __init__(self, ctx, oracle, kb, rb, bucket_focus, curve, n=None, seed=0, pos=None, h=None):
        from cstone_amd.domain import Domain

        n = pos.shape[0] if pos is not None else n
        self.oracle, self.kb, self.rb, self.curve, self.bucket_focus = oracle, kb, rb, curve, bucket_focus
        self.lp = Loop(ctx, kb, rb, bucket_focus, curve, n, seed, pos=pos, h=h)
        self.ref = Loop(ctx, kb, rb, bucket_focus, curve, n, seed, mode=Domain.SORT_FROM_SCRATCH, pos=pos, h=h)
        self.schedule = Schedule(bucket_focus)
        self.inputs, self.motion, self.seed = None, None, seed

    def loops(self):
        return (self.lp, self.ref)

    def _host(self, t):
        return t.cpu().numpy()

    def state(self):
        """of the re-sorting loop, after at least one sync"""
        v, dom = self.lp.dom.view(), self.lp.dom
        L = v.num_focus_leaves
        return State(self._host(self.lp.x), self._host(self.lp.y), self._host(self.lp.z),
                     self._host(self.lp.keys).view(KEY_DTYPE[self.kb]),
                     dom.fetch(v.focus_leaves, L + 1, KEY_DTYPE[self.kb]).astype(_u64),
                     dom.fetch(v.layout, L + 1, np.uint32).astype(np.int64))

    def put(self, x, y, z, marks=None):
        """the client's move: new coordinates (array order), remove markers where marks is set -- for both loops"""
        import torch

        for lp in self.loops():
            for t, a in zip((lp.x, lp.y, lp.z), (x, y, z)):
                t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=REAL_DTYPE[self.rb])))
            if marks is not None:
                # (the bit pattern of endKey in the signed type torch has)
                lp.keys[torch.from_numpy(np.nonzero(marks)[0]).cuda()] = (
                    torch.iinfo(torch.int64).min if self.kb == 64 else (1 << 30))

    def move(self):
        """the common motion (resort_support.Motion), the same draw for both loops"""
        from resort_support import Motion

        if self.motion is None:
            self.motion = Motion(self.seed + 100)
        drawn = self.motion.draw(self.lp)
        for lp in self.loops():
            self.motion.apply(lp, drawn)

    def _plan(self):
        from oracle.oracle import Box

        s, v = self.state(), self.lp.dom.view()
        new = self.oracle.compute_sfc_keys(self.curve, self.kb, s.x, s.y, s.z, Box(list(v.box.lim), (1, 1, 1))).astype(_u64)
        new[s.keys.astype(_u64) == _u64(end_key(self.kb))] = _u64(end_key(self.kb))
        self.inputs = (s.tree, s.layout, new)
        return plan(s.tree, s.layout, new, self.kb, self.bucket_focus)

    def sync(self, premise=None, what=""):
        """-> (attempted, plan or None)"""
        before = dict(self.schedule.expected)
        attempted, p = self.schedule.step(_aligned(self.lp), self._plan)
        if premise is not None:
            premise(attempted, p)
        for lp in self.loops():
            lp.sync()
        st = self.lp.dom.stats()
        got = {k: st[k] for k in self.schedule.expected}
        assert got == self.schedule.expected, (what, self.schedule.syncs, "before", before, "plan", _brief(p))
        assert self.ref.dom.stats()["resorts"] == 0
        assert_same(self.lp, self.ref, (what, self.schedule.syncs))
        return attempted, p


def _brief(p):
    return None if p is None else dict(J=p.J, movers=p.movers, markers=p.markers, leaf=p.leaf_flag, tile=p.tile_flag,
                                       list=p.list_flag, accepted=p.accepted,
                                       max_leaf=int(p.slots_leaf.max()), max_tile=int(p.slots_tile.max(initial=0)))


class Sim:
    """the Tracker's interface without a GPU: the arrays are sorted with numpy, the leaves follow the keys one update step
    per sync (oracle.compute_octree at the first sync).  Its leaves are A valid previous view, and for the lattice cases,
    whose premises pin the view, THE view the domain has"""

    def __init__(self, oracle, kb, rb, bucket_focus, curve, n=None, seed=0, pos=None, h=None):
        from resort_support import cloud, smoothing_lengths

        rng = np.random.default_rng(seed)
        pos = cloud(rng, n) if pos is None else pos
        n = pos.shape[0]
        self.h = (smoothing_lengths(rng, n) if h is None else h).astype(REAL_DTYPE[rb])
        self.oracle, self.kb, self.rb, self.curve, self.bucket_focus = oracle, kb, rb, curve, bucket_focus
        self.x, self.y, self.z = [np.ascontiguousarray(pos[:, d]).astype(REAL_DTYPE[rb]) for d in range(3)]
        self.keys = np.zeros(n, dtype=_u64)
        self.tree = self.layout = None
        self.schedule = Schedule(bucket_focus)
        self.inputs = None
        self.rng = np.random.default_rng(seed + 100)

    def move(self):
        self.put(*motion_np(self.rng, self.state(), self.h.astype(np.float64)))

    def state(self):
        return State(self.x.copy(), self.y.copy(), self.z.copy(), self.keys.copy(), self.tree, self.layout)

    def put(self, x, y, z, marks=None):
        self.x, self.y, self.z = [np.ascontiguousarray(a, dtype=REAL_DTYPE[self.rb]) for a in (x, y, z)]
        if marks is not None:
            self.keys[marks] = _u64(end_key(self.kb))

    def _new_keys(self):
        from oracle.oracle import Box

        new = self.oracle.compute_sfc_keys(self.curve, self.kb, self.x, self.y, self.z, Box([0, 1] * 3, (1, 1, 1))).astype(_u64)
        new[self.keys == _u64(end_key(self.kb))] = _u64(end_key(self.kb))
        return new

    def _plan(self):
        self.inputs = (self.tree, self.layout, self._new_keys())
        return plan(*self.inputs, self.kb, self.bucket_focus)

    def sync(self, premise=None, what=""):
        attempted, p = self.schedule.step(True, self._plan)
        if premise is not None:
            premise(attempted, p)
        new = self._new_keys()
        order = np.argsort(new, kind="stable")
        if p is not None:
            # the rule is sufficient: stayers and arrivals ordered leaf by leaf ARE the stable sort
            assert np.array_equal(order_from_plan(p, new), order), (what, self.schedule.syncs)
        order = order[:np.searchsorted(new[order], _u64(end_key(self.kb)))]
        self.x, self.y, self.z, self.h, self.keys = [a[order] for a in (self.x, self.y, self.z, self.h, new)]
        typed = self.keys.astype(KEY_DTYPE[self.kb])
        if self.tree is None:
            tree, counts = self.oracle.compute_octree(typed, self.bucket_focus)
        else:
            old = self.tree.astype(KEY_DTYPE[self.kb])
            tree, counts, _ = self.oracle.update_octree(typed, self.bucket_focus, old, self.oracle.node_counts(old, typed))
        self.tree = tree.astype(_u64)
        self.layout = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        return attempted, p


def motion_np(rng, s, h):
    """the common motion of resort_support.Motion restated on the host: at most 0.1 h per coordinate, 2 % (one at least)
    jump anywhere, positions wrap"""
    jumpers = rng.permutation(s.n)[:max(1, s.n // 50)]
    out = []
    for a in (s.x, s.y, s.z):
        a = a.astype(np.float64) + rng.uniform(-0.1, 0.1, s.n) * h
        a[jumpers] = rng.uniform(0, 1, jumpers.size)
        out.append(np.clip(np.remainder(a, 1.0), 0.0, 1.0 - 1e-6))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# clouds and moves
# ----------------------------------------------------------------------------------------------------------------------
LATTICE_SIDE = 32  # 32^3 particles at (i + 0.5) / 32: 512 cells of level 3 with 64 particles each


def lattice(oracle, kb, curve, per_leaf=None):
    """the lattice; per_leaf {cell in SFC order: particles kept of its 64}: thinned or empty cells.  A cell stays a leaf
    for every focus bucket from 64 to 255 as long as its parent keeps more particles than the bucket"""
    from oracle.oracle import Box

    g = (np.arange(LATTICE_SIDE) + 0.5) / LATTICE_SIDE
    pos = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))
    if per_leaf:
        keys = oracle.compute_sfc_keys(curve, kb, *[np.ascontiguousarray(pos[:, d]) for d in range(3)], Box([0, 1] * 3, (1, 1, 1)))
        order = np.argsort(keys, kind="stable")
        keep = np.ones(pos.shape[0], dtype=bool)
        for cell, count in per_leaf.items():
            keep[order[64 * cell + count:64 * cell + 64]] = False
        pos = pos[keep]
    h = np.full(pos.shape[0], 0.01)
    return pos, h


def position_of_key(oracle, kb, curve, key):
    """centre of the deepest-level cell with this key: exact in float32 (32-bit keys) and float64"""
    ix, iy, iz = oracle.decode(curve, kb, int(key))
    scale = float(1 << MAX_LEVEL[kb])
    return (ix + 0.5) / scale, (iy + 0.5) / scale, (iz + 0.5) / scale


def send(drv, s, who, keys):
    """particles who[i] (array positions) move to the cell of keys[i]; everybody else stays where they are"""
    x, y, z = s.x.copy(), s.y.copy(), s.z.copy()
    for i, key in zip(who, keys):
        x[i], y[i], z[i] = position_of_key(drv.oracle, drv.kb, drv.curve, key)
    drv.put(x, y, z)


def keys_inside(s, leaf, count):
    """`count` keys inside leaf `leaf` of the state's tree, ascending from its first key, spread over the leaf"""
    lo, hi = int(s.tree[leaf]), int(s.tree[leaf + 1])
    return [lo + k * max(1, (hi - lo) // (count + 1)) for k in range(count)]


def donors(s, exclude_leaves, count):
    """`count` array positions outside the given leaves, taken from the END of the other non-empty leaves in turn (the
    donor leaves keep their slots: holes count)"""
    banned = set(int(l) for l in exclude_leaves)
    leaves = [l for l in np.nonzero(s.counts > 0)[0] if int(l) not in banned]
    out, depth = [], 0
    while len(out) < count:
        took = False
        for l in leaves:
            if len(out) < count and s.counts[l] > depth + 1:  # (a donor leaf keeps one particle at least)
                out.append(int(s.layout[l + 1]) - 1 - depth)
                took = True
        assert took, "not enough donors"
        depth += 1
    return out


def compact_leaves(s):
    """tree indices of the non-empty leaves: the compact leaf j is leaf compact_leaves(s)[j]"""
    return np.nonzero(s.counts > 0)[0]
