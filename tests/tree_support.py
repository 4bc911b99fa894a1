"""TEST INFRASTRUCTURE for tests/test_tree_update.py and tests/test_scans.py: plain numpy models of the cornerstone leaf
array's update (csrc/tree.hip) and of the scans that drive it (csrc/scan.hip), the trees and key sets the tests run on,
and a thin caller of the C ABI that works on both backends of let_ops_support.

Models.  Written from the contract comments in include/cstone_hip.h and the reference lines they cite (R = the
reference's include/cstone: R/tree/csarray.hpp:94-103 counts, :270-310 decisions, :360-385 rebalance); vectorised, all
key arithmetic in uint64.  They share no code with tree.hip, scan.hip or the oracle: the sibling sums are differences of
one running sum, the rebalance expands every old node with np.repeat instead of searching the scanned ops, the counts
are np.searchsorted.  ops_model(variant=...) restates one WRONG rule at a time; the variants never judge a kernel, they
show that the decision cases below tell every such mistake from the true rule (test_premise_*)."""
import ctypes as C

import numpy as np

from helpers import OctreeMaker

MAX_LEVEL = {32: 10, 64: 21}
KEY_DTYPE = {32: np.uint32, 64: np.uint64}
U32_MAX = 0xFFFFFFFF
E_ARG, E_CAPACITY = -1, -2

_u64 = np.uint64


def end_key(kb):
    return 1 << (3 * MAX_LEVEL[kb])


def kb_of(tree):
    return tree.dtype.itemsize * 8


# ----------------------------------------------------------------------------------------------------------------------
# models
# ----------------------------------------------------------------------------------------------------------------------
def node_levels(tree):
    """level of every node of a leaf array: its span is 8^(maxLevel - level) (treeLevel, R/tree/csarray.hpp:273-274).
    frexp is exact for the powers of two that the spans are."""
    span = np.diff(tree.astype(_u64))
    _, e = np.frexp(span.astype(np.float64))
    return MAX_LEVEL[kb_of(tree)] - (e.astype(np.int64) - 1) // 3


def counts_model(tree, keys, max_count=U32_MAX):
    """calculateNodeCount (R/tree/csarray.hpp:94-103): keys in [tree[i], tree[i + 1]), at most max_count"""
    pos = np.searchsorted(keys, tree, side="left")
    return np.minimum(np.diff(pos), max_count).astype(np.uint32)


VARIANTS = ("sum32", "merge_lt", "split_ge", "guard0_loose", "guard1_loose", "guard2_loose", "guard3_loose",
            "guard0_tight", "guard1_tight", "guard2_tight", "guard3_tight", "no_sibling_test", "merge_sib0")


def ops_model(tree, counts, bucket, kb=None, variant=None):
    """calculateNodeOp for every node (R/tree/csarray.hpp:270-310) -> (ops[n + 1] with a trailing 0, converged).
    Merge (0): sibling index > 0, the eight nodes from i - sib tile one parent, their 64-bit sum <= bucket.  Split:
    4096 / 512 / 64 / 8 for c > bucket * 512 / 64 / 8 / 1 (products in 32-bit unsigned arithmetic) where the level
    leaves room: level + 3 / 2 / 1 / 0 < maxLevel.  Keep (1) otherwise."""
    kb = kb or kb_of(tree)
    assert variant is None or variant in VARIANTS
    ml = MAX_LEVEL[kb]
    t = tree.astype(_u64)
    n = t.size - 1
    c = counts.astype(_u64)
    span = np.diff(t)
    level = node_levels(tree)
    sib = ((t[:-1] >> (3 * (ml - level)).astype(_u64)) & _u64(7)).astype(np.int64)
    first = np.arange(n) - sib
    last = np.minimum(first + 8, n)
    running = np.concatenate([np.zeros(1, _u64), np.cumsum(c, dtype=_u64)])  # < 2^21 * 2^32: no wrap
    parent = running[last] - running[first]
    if variant == "sum32":
        parent = parent & _u64(U32_MAX)
    # eight nodes tile the parent: the ninth key is the first one plus the parent's span (8 x this node's)
    complete = (level > 0) & (first + 8 <= n)
    complete[complete] = t[last[complete]] == t[first[complete]] + _u64(8) * span[complete]
    if variant == "no_sibling_test":
        complete = level > 0
    may = (level > 0) if variant == "merge_sib0" else (sib > 0)
    fits = parent < _u64(bucket) if variant == "merge_lt" else parent <= _u64(bucket)
    merge = may & complete & fits

    ops = np.ones(n + 1, np.int64)
    ops[n] = 0
    room = {k: 0 for k in range(4)}
    if variant and variant.startswith("guard"):
        room[int(variant[5])] = -1 if variant.endswith("loose") else 1
    # weakest rule first, so that a stronger one overwrites it
    for k, mult in ((0, 1), (1, 8), (2, 64), (3, 512)):
        limit = _u64((bucket * mult) & U32_MAX)
        over = c >= limit if variant == "split_ge" else c > limit
        ops[:n][over & (level + k + room[k] < ml)] = 8 ** (k + 1)
    ops[:n][merge] = 0
    return ops, bool((ops[:n] == 1).all())


def scan_model(values, init=0, inclusive=False, bits=32):
    """exclusive: out[i] = init + sum(values[0..i)); inclusive: ... + values[i]; modulo 2^bits"""
    v = np.asarray(values).astype(_u64)
    run = np.cumsum(v, dtype=_u64)
    if not inclusive:
        run = np.concatenate([np.zeros(1, _u64), run[:-1]]) if v.size else run
    run = run + _u64(init)
    return (run & _u64(U32_MAX)).astype(np.uint32) if bits == 32 else run


def offsets_model(counts):
    """n + 1 outputs: the exclusive scan with its grand total behind it"""
    return scan_model(np.concatenate([np.asarray(counts, np.uint32), np.zeros(1, np.uint32)]))


_DOWN = {0: 0, 1: 0, 8: 1, 64: 2, 512: 3, 4096: 4}


def rebalance_model(tree, scanned_ops):
    """processNode for every old node (R/tree/csarray.hpp:360-385): node i becomes scanned[i + 1] - scanned[i] nodes
    from index scanned[i] on, each 8^-k of its span; the last key is carried over.  `tree` may be any run of
    consecutive leaves: nothing but tree[i], tree[i + 1] and the last key is used."""
    t = tree.astype(_u64)
    s = np.asarray(scanned_ops).astype(np.int64)
    cnt = np.diff(s)
    assert np.isin(cnt, list(_DOWN)).all()
    n = t.size - 1
    down = np.zeros(n, np.int64)
    for c, d in _DOWN.items():
        down[cnt == c] = d
    step = np.diff(t) >> (3 * down).astype(_u64)
    src = np.repeat(np.arange(n), cnt)
    j = (np.arange(int(s[-1])) - s[src]).astype(_u64)
    return np.concatenate([t[src] + j * step[src], t[-1:]]).astype(tree.dtype)


def update_model(keys, bucket, tree, counts, max_count=U32_MAX):
    """one step of updateOctree (R/tree/csarray.hpp:430-448): decisions, scan, rebalance, recount"""
    ops, converged = ops_model(tree, counts, bucket)
    new_tree = rebalance_model(tree, scan_model(ops))
    return new_tree, counts_model(new_tree, keys, max_count), converged


def octree_model(keys, bucket, max_count=U32_MAX, limit=64):
    """computeOctree (R/tree/csarray.hpp:453-466): from the root (seeded with the number of keys) until converged
    -> (tree, counts, number of updates)"""
    tree, counts = root(kb_of(keys)), np.array([keys.size], np.uint32)
    for it in range(1, limit + 1):
        tree, counts, converged = update_model(keys, bucket, tree, counts, max_count)
        if converged:
            return tree, counts, it
    raise AssertionError("octree_model: no convergence")


# ----------------------------------------------------------------------------------------------------------------------
# trees and keys
# ----------------------------------------------------------------------------------------------------------------------
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def root(kb):
    return np.array([0, end_key(kb)], KEY_DTYPE[kb])


def children(kb):
    return uniform(kb, 1)


def uniform(kb, level):
    n = 8 ** level
    return (np.arange(n + 1, dtype=_u64) * _u64(end_key(kb) // n)).astype(KEY_DTYPE[kb])


def merged_first(tree):
    """the same leaf array with its first eight leaves replaced by their parent"""
    return np.concatenate([tree[:1], tree[8:]])


def deepest_path(kb, digits=None):
    """refined along one key path down to the deepest level: 7 L + 1 leaves (as halos_support.deep_tree builds it with
    OctreeMaker; here from the keys: at every level the seven siblings of the path's node, around the eight deepest)"""
    ml = MAX_LEVEL[kb]
    digits = digits or [(3 * i + 5) % 8 for i in range(ml)]
    keys, at = {end_key(kb)}, 0
    for lvl in range(1, ml + 1):
        step = 1 << (3 * (ml - lvl))
        keys.update(at + s * step for s in range(8))
        at += digits[lvl - 1] * step
    return np.array(sorted(keys), KEY_DTYPE[kb])


def maker(kb, *paths):
    m = OctreeMaker(kb)
    for p in paths:
        m.divide(*p)
    return m.make()


def clustered_keys(kb, n, seed=1):
    """sorted Morton keys of a clustered cloud in the unit cube: Gaussian blobs of very different widths over a thin
    uniform background and a few particles in every corner, so the tree mixes deep and shallow leaves up to the last key"""
    def make():
        rng = np.random.default_rng(seed)
        nb = max(n // 10, 8)
        parts = [rng.uniform(0, 1, (nb, 3))]
        widths = [0.2, 0.05, 0.01, 0.002, 0.08, 0.0005]
        each = (n - nb - 16) // len(widths)
        for w in widths:
            parts.append(rng.normal(rng.uniform(0.1, 0.9, 3), w, (each, 3)))
        corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], float)
        parts.append(np.repeat(corners, 2, axis=0))
        pts = np.concatenate(parts)
        pts = np.concatenate([pts, rng.uniform(0, 1, (n - pts.shape[0], 3))])
        ml = MAX_LEVEL[kb]
        ijk = np.clip((pts * (1 << ml)).astype(np.int64), 0, (1 << ml) - 1).astype(_u64)
        key = np.zeros(n, _u64)
        for b in range(ml):
            for d in range(3):
                key |= ((ijk[:, d] >> _u64(b)) & _u64(1)) << _u64(3 * b + 2 - d)
        return np.sort(key).astype(KEY_DTYPE[kb])
    return cached(("keys", kb, n, seed), make)


def cloud_tree(kb, n, bucket, seed=1):
    """(keys, tree, counts) of the cornerstone tree of the clustered cloud, from the model's own loop"""
    def make():
        keys = clustered_keys(kb, n, seed)
        return (keys,) + octree_model(keys, bucket)[:2]
    return cached(("cloud", kb, n, bucket, seed), make)


BIG_CLOUD = (150000, 4)  # keys, bucket: about 10^5 leaves


def big_tree(kb):
    return cloud_tree(kb, *BIG_CLOUD)


# ----------------------------------------------------------------------------------------------------------------------
# decision cases: (name, tree, counts, bucket, {index: expected op})
# ----------------------------------------------------------------------------------------------------------------------
THRESHOLD_OPS = (1, 8, 8, 64, 64, 512, 512, 4096)


def threshold_counts(bucket):
    return (bucket, bucket + 1, 8 * bucket, 8 * bucket + 1, 64 * bucket, 64 * bucket + 1, 512 * bucket, 512 * bucket + 1)


def threshold_cases(kb):
    """a leaf of level 2 (sixth of its eight siblings; every other leaf holds exactly `bucket`, so nothing else moves)
    with a count at and just above each split threshold"""
    tree = maker(kb, (), (0,))
    out = []
    for bucket in (1, 16, 1 << 20):
        for c, op in zip(threshold_counts(bucket), THRESHOLD_OPS):
            counts = np.full(tree.size - 1, bucket, np.uint32)
            counts[5] = c
            out.append((f"threshold-b{bucket}-c{c}", tree, counts, bucket, {5: op}))
    return out


def guard_cases(kb):
    """the largest count on one leaf of level top, top - 1, .. top - 4 of the deepest-path tree, then on all five"""
    tree, bucket, ml = deepest_path(kb), 16, MAX_LEVEL[kb]
    level = node_levels(tree)
    at = [int(np.nonzero(level == ml - k)[0][-1]) for k in range(5)]  # the last leaf of each level: sibling 7 or 6
    out, every = [], np.full(tree.size - 1, bucket, np.uint32)
    for k, (i, op) in enumerate(zip(at, (1, 8, 64, 512, 4096))):
        counts = np.full(tree.size - 1, bucket, np.uint32)
        counts[i] = every[i] = U32_MAX
        out.append((f"guard-top-{k}", tree, counts, bucket, {i: op}))
    out.append(("guard-all", tree, every, bucket, dict(zip(at, (1, 8, 64, 512, 4096)))))
    return out


def merge_cases(kb):
    bucket, out = 16, []
    # children 2 of the root subdivided: leaves 2..9 are a complete group of level 2
    tree = maker(kb, (), (2,))

    def group(values, rest=bucket):
        counts = np.full(tree.size - 1, rest, np.uint32)
        counts[2:10] = values
        return counts
    keep = {i: 1 for i in range(tree.size - 1)}
    out.append(("merge-sum-eq-bucket", tree, group(2), bucket, {**keep, **{i: 0 for i in range(3, 10)}}))
    out.append(("merge-sum-bucket-plus-1", tree, group([3, 2, 2, 2, 2, 2, 2, 2]), bucket, keep))
    big = 1 << 20
    out.append(("merge-sum-passes-2^32", tree, group(1 << 31, big), big, {**keep, **{i: 4096 for i in range(2, 10)}}))
    # the third sibling of that group subdivided once more: 2 + 2 + 8 + 5 + 5 leaves
    deep = maker(kb, (), (2,), (2, 2))
    expect = {i: 1 for i in range(deep.size - 1)}
    expect.update({i: 0 for i in range(5, 12)})
    out.append(("merge-incomplete-group", deep, np.zeros(deep.size - 1, np.uint32), bucket, expect))
    out.append(("merge-root-children", children(kb), np.zeros(8, np.uint32), bucket, {0: 1, **{i: 0 for i in range(1, 8)}}))
    tail = maker(kb, (), (7,))
    counts = np.full(15, bucket, np.uint32)
    counts[7:] = 0
    out.append(("merge-last-eight", tail, counts, bucket, {**{i: 1 for i in range(8)}, **{i: 0 for i in range(8, 15)}}))
    # uniform level 2: groups that merge and groups that split by one, two and three levels side by side
    u2 = uniform(kb, 2)
    counts, expect = np.zeros(64, np.uint32), {}
    for g, (c, op) in enumerate(((0, 0), (bucket + 1, 8), (0, 0), (8 * bucket + 1, 64), (bucket, 1), (0, 0),
                                 (64 * bucket + 1, 512), (0, 0))):
        counts[8 * g:8 * g + 8] = c
        expect.update({8 * g + s: (1 if op == 0 and s == 0 else op) for s in range(8)})
    out.append(("merge-next-to-splits", u2, counts, bucket, expect))
    return out


def decision_cases(kb):
    return threshold_cases(kb) + guard_cases(kb) + merge_cases(kb)


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI on either backend of let_ops_support (cpu: the oracle behind the ABI on host memory; hip: the kernels)
# ----------------------------------------------------------------------------------------------------------------------
class Api:
    def __init__(self, be, kb):
        self.be, self.lib, self.ctx, self.kb = be, be.lib, be.ctx, kb

    def node_ops(self, tree, counts, bucket, ops=None):
        """-> (scanned ops[n + 1], new_num_nodes, converged); tree, counts: host arrays or device buffers; ops: a
        device buffer made beforehand, for a caller that wants nothing but the ABI call to happen here"""
        be, n = self.be, self._len(tree) - 1
        dt, dc = self._dev(tree), self._dev(counts)
        ops = ops if ops is not None else be.filled(n + 1, np.uint32, 0xDEADBEEF)
        new_n, conv = C.c_int(-1), C.c_int(-1)
        be.chk(self.lib.cstone_hip_compute_node_ops(self.ctx, C.c_int(self.kb), be.ptr(dt), C.c_int(n), be.ptr(dc),
                                                    C.c_uint32(bucket), be.ptr(ops), C.byref(new_n), C.byref(conv)),
               "compute_node_ops")
        return ops, new_n.value, conv.value

    def rebalance(self, tree, scanned, new_n):
        """-> the new_n + 1 new keys; the two sentinel keys behind them must survive"""
        be, n = self.be, self._len(tree) - 1
        kdt = KEY_DTYPE[self.kb]
        sentinel = kdt(0x5A5A5A5A)
        out = be.filled(new_n + 3, kdt, sentinel)
        dt, ds = self._dev(tree), self._dev(scanned)  # (named: the buffers must outlive the call)
        be.chk(self.lib.cstone_hip_rebalance_tree(self.ctx, C.c_int(self.kb), be.ptr(dt), C.c_int(n), C.c_int(new_n),
                                                  be.ptr(ds), be.ptr(out)), "rebalance_tree")
        got = be.to_host(out, kdt)
        assert got[new_n + 1] == sentinel and got[new_n + 2] == sentinel, "rebalance_tree wrote behind the new tree"
        return got[:new_n + 1]

    def counts(self, tree, keys, max_count=U32_MAX, guess=None):
        be, n = self.be, self._len(tree) - 1
        dt, dk = self._dev(tree), self._dev(keys)
        out = be.filled(n + 2, np.uint32, 0xDEADBEEF)
        args = (self.ctx, C.c_int(self.kb), be.ptr(dt), be.ptr(out), C.c_int(n), be.ptr(dk),
                C.c_size_t(self._len(keys)), C.c_uint32(max_count))
        if guess is None:
            be.chk(self.lib.cstone_hip_compute_node_counts(*args), "compute_node_counts")
        else:
            dg = self._dev(guess)
            be.chk(self.lib.cstone_hip_compute_node_counts_guided(*args, be.ptr(dg)), "compute_node_counts_guided")
        got = be.to_host(out, np.uint32)
        assert got[n] == 0xDEADBEEF and got[n + 1] == 0xDEADBEEF, "compute_node_counts wrote behind the counts"
        return got[:n]

    def buffers(self, tree, counts, cap):
        """device tree and counts with room for cap leaves, marked behind the payload"""
        kdt = KEY_DTYPE[self.kb]
        t = np.full(cap + 1, 0x5A5A5A5A, kdt)
        c = np.full(cap, 0xDEADBEEF, np.uint32)
        t[:tree.size], c[:counts.size] = tree, counts
        return self.be.to_dev(t), self.be.to_dev(c)

    def update(self, keys, bucket, tbuf, cbuf, nl, cap, max_count=U32_MAX):
        """one update on capacity buffers -> (rc, leaf count as reported, converged)"""
        be = self.be
        num, conv, dk = C.c_int(nl), C.c_int(-1), self._dev(keys)
        rc = self.lib.cstone_hip_update_octree(self.ctx, C.c_int(self.kb), be.ptr(dk),
                                               C.c_size_t(self._len(keys)), C.c_uint32(bucket), be.ptr(tbuf),
                                               be.ptr(cbuf), C.byref(num), C.c_int(cap), C.c_uint32(max_count),
                                               C.byref(conv))
        return rc, num.value, conv.value

    def compute(self, keys, bucket, cap, max_count=U32_MAX):
        """-> (tree, counts, number of updates)"""
        be, kdt = self.be, KEY_DTYPE[self.kb]
        tbuf, cbuf = be.filled(cap + 1, kdt, 0x5A5A5A5A), be.filled(cap, np.uint32, 0xDEADBEEF)
        num, iters, dk = C.c_int(-1), C.c_int(-1), self._dev(keys)
        be.chk(self.lib.cstone_hip_compute_octree(self.ctx, C.c_int(self.kb), be.ptr(dk),
                                                  C.c_size_t(self._len(keys)), C.c_uint32(bucket), be.ptr(tbuf),
                                                  be.ptr(cbuf), C.byref(num), C.c_int(cap), C.c_uint32(max_count),
                                                  C.byref(iters)), "compute_octree")
        return be.to_host(tbuf, kdt)[:num.value + 1], be.to_host(cbuf, np.uint32)[:num.value], iters.value

    def fetch(self, tbuf, cbuf, nl):
        return self.be.to_host(tbuf, KEY_DTYPE[self.kb])[:nl + 1], self.be.to_host(cbuf, np.uint32)[:nl]

    def dev(self, a):
        """upload once what several calls use"""
        buf = self.be.to_dev(a)
        buf.count = a.size
        return buf

    def _dev(self, a):
        return a if hasattr(a, "raw") else self.be.to_dev(a)

    @staticmethod
    def _len(a):
        return a.count if hasattr(a, "raw") else a.size
