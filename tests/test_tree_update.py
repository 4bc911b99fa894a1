"""The kernels that maintain the cornerstone leaf array (csrc/tree.hip: boundaryPositionsKernel, countsFromPositionsKernel,
nodeOpsKernel, rebalanceKernel, the host sequences updateOctree / cstone_hip_compute_octree), each called through the C
ABI and compared with `==` against the numpy models of tests/tree_support.py -- above all where a tree SHRINKS and where
a count sits exactly on a threshold, which the refining builds of test_gpu_parity.py never see.

Every body runs on two backends (let_ops_support): `cpu` (no marker) serves the ABI from the project's CPU restatement
(oracle/cabi_on_oracle.cpp on cstone_oracle.hpp), so there the MODEL is compared with the oracle on every shape; `hip`
(@gpu) lets the model judge the kernels.  Where the oracle's Python front end offers the call (node_counts, node_ops,
update_octree, compute_octree), its answer is compared with the model's on both legs as well.  All cases run for 32-bit
keys (10 levels) and 64-bit keys (21 levels)."""
import numpy as np
import pytest

import let_ops_support as S
import tree_support as T

gpu = pytest.mark.gpu
KB = pytest.mark.parametrize("kb", [32, 64])


@pytest.fixture(params=["cpu", pytest.param("hip", marks=gpu)])
def be(request):
    if request.param == "cpu":
        return S.cpu_backend()
    return S.HipBackend(request.getfixturevalue("hip"))


def check_ops(api, oracle, tree, counts, bucket, name="", dtree=None):
    """compute_node_ops against the model (scanned ops, new leaf count, flag) -> (the model's ops, the device's scan)"""
    want, want_conv = T.ops_model(tree, counts, bucket)
    scan = T.scan_model(want)
    dtree = dtree if dtree is not None else api.dev(tree)
    got, new_n, conv = api.node_ops(dtree, counts, bucket)
    assert (new_n, conv) == (int(scan[-1]), int(want_conv)), name
    assert np.array_equal(api.be.to_host(got, np.uint32), scan), name
    if oracle is not None:
        ref, ref_conv = oracle.node_ops(tree, counts, bucket)
        assert np.array_equal(ref, want[:-1]) and ref_conv == want_conv, name
    return want, got


# ----------------------------------------------------------------------------------------------------------------------
# decisions
# ----------------------------------------------------------------------------------------------------------------------
@KB
def test_decisions_at_thresholds_guards_and_merges(be, oracle, kb):
    api = T.Api(be, kb)
    for name, tree, counts, bucket, expect in T.decision_cases(kb):
        want, _ = check_ops(api, oracle, tree, counts, bucket, name)
        for i, op in expect.items():  # the model itself against the values the case was built for
            assert want[i] == op, (name, i)


@KB
def test_merge_cascade_over_two_steps(be, kb):
    """all counts 0: the subdivided third sibling's children merge first, the group it then completes merges next"""
    api = T.Api(be, kb)
    tree = T.maker(kb, (), (2,), (2, 2))
    keys = np.zeros(0, T.KEY_DTYPE[kb])
    counts = np.zeros(tree.size - 1, np.uint32)
    tbuf, cbuf = api.buffers(tree, counts, 64)
    nl = tree.size - 1
    for want_tree in (T.maker(kb, (), (2,)), T.children(kb), T.root(kb)):
        tree, counts, conv = T.update_model(keys, 16, tree, counts)
        assert np.array_equal(tree, want_tree) and not conv
        rc, nl, got_conv = api.update(keys, 16, tbuf, cbuf, nl, 64)
        assert (rc, nl, got_conv) == (0, tree.size - 1, 0)
        got_tree, got_counts = api.fetch(tbuf, cbuf, nl)
        assert np.array_equal(got_tree, tree) and np.array_equal(got_counts, counts)


def flag_trees(kb):
    return {"uniform3": T.uniform(kb, 3), "cloud": T.big_tree(kb)[1]}


def complete_group_ends(tree):
    """index of the last sibling of every complete group of eight leaves"""
    ops, _ = T.ops_model(tree, np.zeros(tree.size - 1, np.uint32), 1)  # all counts 0: every complete group merges
    return np.nonzero((ops[:-1] == 0) & (np.append(ops[1:-1], 1) != 0))[0]


def merge_group_ends(tree, which):
    """last sibling of three mergeable groups: in the last lane of a wave, in the last lane of a workgroup, and the last
    complete group of the array.  The uniform tree has them at 63, 255 and n - 1; the cloud tree where its groups fall."""
    ends = complete_group_ends(tree)
    if which == "uniform3":
        picks = (63, 255, tree.size - 2)
    else:
        picks = (int(ends[(ends % 64 == 63) & (ends % 256 != 255)][0]), int(ends[ends % 256 == 255][0]), int(ends[-1]))
    assert all(p in ends for p in picks) and picks[0] % 64 == 63 and picks[1] % 256 == 255
    return picks


@KB
@pytest.mark.parametrize("which", ["uniform3", "cloud"])
def test_converged_flag_from_one_node_anywhere(be, oracle, kb, which):
    """nodeOpsKernel raises the flag from lane 0 of a wave on behalf of the other 63: one node that splits at the start
    and end of a wave, of a workgroup and of the last, partly filled wave; then one group that merges (seven nodes with
    op 0) whose last sibling sits in the last lane of a wave, in the last lane of a workgroup, and the last complete
    group of the array"""
    api = T.Api(be, kb)
    tree, bucket = flag_trees(kb)[which], 16
    n = tree.size - 1
    dtree = api.dev(tree)
    calm = np.full(n, bucket, np.uint32)
    want, got = check_ops(api, oracle, tree, calm, bucket, "calm", dtree)
    assert (want[:-1] == 1).all() and np.array_equal(be.to_host(got, np.uint32), np.arange(n + 1, dtype=np.uint32))
    level = T.node_levels(tree)
    for i in (0, 63, 64, 255, 256, n - 1):
        counts = calm.copy()
        counts[i] = bucket + 1
        want, _ = check_ops(api, oracle, tree, counts, bucket, f"split at {i}", dtree)
        assert level[i] < T.MAX_LEVEL[kb] and want[i] == 8 and np.count_nonzero(want[:-1] != 1) == 1
    for last in merge_group_ends(tree, which):
        counts = calm.copy()
        counts[last - 7:last + 1] = 0
        want, _ = check_ops(api, oracle, tree, counts, bucket, f"merge ending at {last}", dtree)
        assert (want[last - 6:last + 1] == 0).all() and np.count_nonzero(want[:-1] != 1) == 7


def level7(kb, shape):
    return T.cached(("level7", kb, shape),
                    lambda: T.uniform(kb, 7) if shape == "full" else T.merged_first(T.uniform(kb, 7)))


@KB
@pytest.mark.parametrize("fill", ["merge-all", "split-all", "merge-a-third"])
@pytest.mark.parametrize("shape", ["full", "first-merged"])
def test_two_million_leaves_either_side_of_the_scan_switch(be, kb, shape, fill):
    """uniform level 7: 2 097 152 leaves, 2 097 153 ops: the first size scanned with three launches; with the first
    group merged (2 097 145 leaves) the last with two.  In place, the total in a device scalar."""
    api = T.Api(be, kb)
    tree, bucket = level7(kb, shape), 16
    n = tree.size - 1
    lead = 1 if shape == "first-merged" else 0  # leaves in front of the first group of level 7
    groups = (n - lead) // 8
    if fill == "merge-all":
        counts = np.zeros(n, np.uint32)
    elif fill == "split-all":
        counts = np.full(n, bucket + 1, np.uint32)
    else:
        third = np.random.default_rng(7).random(groups) < 1 / 3
        counts = np.full(n, bucket, np.uint32)
        counts[lead:] = np.repeat(np.where(third, 0, bucket), 8)
    dtree = api.dev(tree)
    want, scanned = check_ops(api, None, tree, counts, bucket, dtree=dtree)
    new_n = int(want.sum())
    if fill == "merge-all":
        assert new_n == lead + groups
    if fill == "split-all":
        assert new_n == 8 * n
    if new_n < n:  # the shrinking rebalance: 2 097 152 -> 262 144 leaves, binary search over runs of equal values
        got = api.rebalance(dtree, scanned, new_n)
        assert np.array_equal(got, T.rebalance_model(tree, T.scan_model(want)))
        if fill == "merge-all" and shape == "full":
            assert np.array_equal(got, T.uniform(kb, 6))


# ----------------------------------------------------------------------------------------------------------------------
# rebalance
# ----------------------------------------------------------------------------------------------------------------------
def check_rebalance(api, tree, ops):
    scan = T.scan_model(ops)
    want = T.rebalance_model(tree, scan)
    got = api.rebalance(tree, scan.astype(np.uint32), int(scan[-1]))
    assert np.array_equal(got, want) and got[-1] == tree[-1]
    return want


@KB
def test_rebalance_every_kind_of_op(be, kb):
    api = T.Api(be, kb)
    # uniform level 2, bucket 1: the first group merges, then leaves that keep and split by one to four levels
    tree = T.uniform(kb, 2)
    counts = np.ones(64, np.uint32)
    counts[:8] = 0
    counts[[9, 20, 21, 40, 63]] = [2, 9, 65, 513, 513]
    counts[48:56] = 0
    ops, _ = T.ops_model(tree, counts, 1)
    assert set(ops.tolist()) == {0, 1, 8, 64, 512, 4096}
    new = check_rebalance(api, tree, ops)
    assert new.size - 1 == 64 - 14 + 7 + 63 + 511 + 2 * 4095 and np.all(np.diff(new.astype(np.uint64)) > 0)


@KB
@pytest.mark.parametrize("new_n", [255, 256, 257])
def test_rebalance_around_one_workgroup(be, kb, new_n):
    """whole trees have 7 k + 1 leaves; a run of consecutive leaves is all the contract needs (tree[i], tree[i + 1],
    the last key): new_n - 7 leaves of the uniform level-3 tree, the first one split"""
    api = T.Api(be, kb)
    tree = T.uniform(kb, 3)[100:100 + new_n - 7 + 1]
    ops = np.ones(tree.size, np.int64)
    ops[0], ops[-1] = 8, 0
    assert check_rebalance(api, tree, ops).size == new_n + 1


@KB
def test_rebalance_to_a_million_leaves(be, kb):
    api = T.Api(be, kb)
    tree = T.big_tree(kb)[1]
    n, bucket = tree.size - 1, 16
    rng = np.random.default_rng(3)
    counts = rng.choice(np.array([0, bucket, bucket + 1, 8 * bucket + 1], np.uint32), n, p=[0.3, 0.3, 0.25, 0.15])
    for last in complete_group_ends(tree)[::5]:  # every fifth complete group of eight merges
        counts[last - 7:last + 1] = 0
    ops, _ = T.ops_model(tree, counts, bucket)
    assert {0, 1, 8, 64} <= set(ops.tolist()) and 7e5 < ops.sum() < 2e6
    check_rebalance(api, tree, ops)


# ----------------------------------------------------------------------------------------------------------------------
# counts
# ----------------------------------------------------------------------------------------------------------------------
COUNT_TREES = ("root", "uniform2", "deepest", "cloud")


def count_tree(kb, name):
    return {"root": lambda: T.root(kb), "uniform2": lambda: T.uniform(kb, 2), "deepest": lambda: T.deepest_path(kb),
            "cloud": lambda: T.big_tree(kb)[1]}[name]()


def background(kb, name):
    """keys all over the tree: the cloud the tree was built on, or 777 random keys (no power of two)"""
    if name == "cloud":
        return T.big_tree(kb)[0]
    return np.sort(np.random.default_rng(9).integers(0, T.end_key(kb), 777, dtype=np.uint64)).astype(T.KEY_DTYPE[kb])


def key_sets(kb, name):
    tree, kdt, end = count_tree(kb, name), T.KEY_DTYPE[kb], T.end_key(kb)
    back = background(kb, name)
    edge = int(tree[(tree.size - 1) // 2])  # a leaf boundary in the middle (the root has none: its start key)
    below = edge - 1 if edge > 0 else end - 1
    out = [("background", back)]
    for run in (1, 2, 63, 64, 65, 1000):
        out.append((f"run{run}", np.sort(np.concatenate([back, np.full(run, edge, kdt), np.full(run, below, kdt)]))))
    out.append(("all-equal", np.full(300, edge, kdt)))
    out.append(("first-leaf", np.full(5, int(tree[0]), kdt)))
    out.append(("last-leaf", np.full(5, end - 1, kdt)))
    out.append(("none", np.zeros(0, kdt)))
    out.append(("one", np.full(1, below, kdt)))
    return tree, out


@KB
@pytest.mark.parametrize("name", COUNT_TREES)
def test_counts_with_runs_of_equal_keys_on_leaf_boundaries(be, oracle, kb, name):
    api = T.Api(be, kb)
    tree, sets = key_sets(kb, name)
    dtree = api.dev(tree)
    for label, keys in sets:
        full = T.counts_model(tree, keys)
        assert int(full.sum()) == keys.size
        assert np.array_equal(oracle.node_counts(tree, keys), full), label
        dkeys = api.dev(keys)
        largest = int(full.max())
        for max_count in (T.U32_MAX, largest, max(largest - 1, 0), 1):
            got = api.counts(dtree, dkeys, max_count)
            assert np.array_equal(got, np.minimum(full, max_count)), (label, max_count)


def guesses(rng, exact, n):
    """the boundary positions themselves, off by one and by every power of two up to n (so that every gallop length
    occurs, in both directions and into both ends of the keys), constants, and random ones"""
    e = exact.astype(np.int64)
    out = [("exact", e), ("exact-1", e - 1), ("exact+1", e + 1)]
    k = 1
    while (1 << k) <= max(2 * n, 2):
        out += [(f"exact-2^{k}", e - (1 << k)), (f"exact+2^{k}", e + (1 << k))]
        k += 1
    out = [(label, np.clip(g, 0, n)) for label, g in out]
    out += [("zeros", np.zeros_like(e)), ("n", np.full_like(e, n)), ("n-1", np.full_like(e, max(n - 1, 0))),
            ("u32-max", np.full_like(e, T.U32_MAX)), ("random", rng.integers(0, n + 1, e.size))]
    return [(label, g.astype(np.uint32)) for label, g in out]


@KB
@pytest.mark.parametrize("name", COUNT_TREES)
def test_guided_counts_do_not_depend_on_the_guess(be, kb, name):
    """the guesses judge the KERNEL (hip leg).  The CPU restatement of the entry searches the whole array and never reads
    the guess, so the cpu leg only repeats model == oracle and shows that every guess array is well formed."""
    api = T.Api(be, kb)
    tree, sets = key_sets(kb, name)
    dtree = api.dev(tree)
    rng = np.random.default_rng(13)
    sets = dict(sets)
    # (the sets left out differ from run65 in the run length only; with all keys in the first or in the last leaf a
    #  wrong guess makes the search gallop to an end of the key array)
    for label in ("background", "run65", "all-equal", "first-leaf", "last-leaf", "none", "one"):
        keys = sets[label]
        want = T.counts_model(tree, keys, 100)
        dkeys = api.dev(keys)
        exact = np.searchsorted(keys, tree, side="left")
        for kind, guess in guesses(rng, exact, keys.size):
            assert np.array_equal(api.counts(dtree, dkeys, 100, guess), want), (label, kind)


# ----------------------------------------------------------------------------------------------------------------------
# whole updates
# ----------------------------------------------------------------------------------------------------------------------
def step_until_converged(api, oracle, keys, bucket, tree, counts, tbuf, cbuf, cap, max_count=T.U32_MAX):
    """update_octree against update_model (and the model against the oracle's update_octree), step for step
    -> (tree, counts, number of steps)"""
    nl, dkeys = tree.size - 1, api.dev(keys)
    for step in range(1, 65):
        ref_tree, ref_counts, ref_conv = oracle.update_octree(keys, bucket, tree, counts, max_count)
        tree, counts, conv = T.update_model(keys, bucket, tree, counts, max_count)
        assert np.array_equal(ref_tree, tree) and np.array_equal(ref_counts, counts) and ref_conv == conv, step
        rc, nl, got_conv = api.update(dkeys, bucket, tbuf, cbuf, nl, cap, max_count)
        assert (rc, nl, got_conv) == (0, tree.size - 1, int(conv)), step
        got_tree, got_counts = api.fetch(tbuf, cbuf, nl)
        assert np.array_equal(got_tree, tree) and np.array_equal(got_counts, counts), step
        if conv:
            return tree, counts, step
    raise AssertionError("no convergence")


@KB
def test_shrink_to_an_eighth_of_the_keys_and_grow_back(be, oracle, kb):
    api = T.Api(be, kb)
    bucket = 16
    keys, full_tree, full_counts = T.cloud_tree(kb, 40000, bucket)
    cap = 8 * full_tree.size
    got_tree, got_counts, iters = api.compute(keys, bucket, cap)
    assert np.array_equal(got_tree, full_tree) and np.array_equal(got_counts, full_counts)
    assert iters == T.octree_model(keys, bucket)[2]

    few = np.ascontiguousarray(keys[::8])
    counts = api.counts(full_tree, few)
    assert np.array_equal(counts, T.counts_model(full_tree, few))
    tbuf, cbuf = api.buffers(full_tree, counts, cap)
    small_tree, small_counts, steps = step_until_converged(api, oracle, few, bucket, full_tree, counts, tbuf, cbuf, cap)
    assert steps > 2 and small_tree.size < full_tree.size // 4
    # the same tree by the other route: from the root on the reduced keys
    direct_tree, direct_counts, _ = api.compute(few, bucket, cap)
    assert np.array_equal(direct_tree, small_tree) and np.array_equal(direct_counts, small_counts)
    ref_tree, ref_counts = oracle.compute_octree(few, bucket)
    assert np.array_equal(ref_tree, small_tree) and np.array_equal(ref_counts, small_counts)

    counts = api.counts(small_tree, keys)
    tbuf, cbuf = api.buffers(small_tree, counts, cap)
    tree, counts, _ = step_until_converged(api, oracle, keys, bucket, small_tree, counts, tbuf, cbuf, cap)
    assert np.array_equal(tree, full_tree) and np.array_equal(counts, full_counts)


@KB
@pytest.mark.parametrize("places", [1, 2])
def test_coincident_particles_end_at_the_deepest_level(be, oracle, kb, places):
    """1000 copies of one key (or of two keys that differ in the last octal digit) at bucket 16: refined down to the
    deepest level, converged there with leaf counts above the bucket"""
    api = T.Api(be, kb)
    ml, kdt = T.MAX_LEVEL[kb], T.KEY_DTYPE[kb]
    digits = [(5 * i + 3) % 8 for i in range(ml - 1)] + [2]
    key = sum(d << (3 * (ml - 1 - i)) for i, d in enumerate(digits))
    keys = np.full(1000, key, kdt)
    if places == 2:
        keys[500:] = key + 3
    tree, counts, iters = api.compute(keys, 16, 4096)
    want_tree, want_counts, want_iters = T.octree_model(keys, 16)
    assert np.array_equal(tree, want_tree) and np.array_equal(counts, want_counts) and iters == want_iters < 64
    assert np.array_equal(tree, T.deepest_path(kb, digits))
    ref_tree, ref_counts = oracle.compute_octree(keys, 16)
    assert np.array_equal(ref_tree, tree) and np.array_equal(ref_counts, counts)
    assert sorted(counts[counts > 0].tolist()) == ([1000] if places == 1 else [500, 500])
    assert (T.node_levels(tree)[counts > 0] == ml).all()


@KB
def test_clamped_counts_steer_the_next_step(be, oracle, kb):
    """max_count 100 at bucket 64: from the second step on every count is at most 100, so leaves split by one level only"""
    api = T.Api(be, kb)
    keys = T.clustered_keys(kb, 40000)
    want_tree, want_counts, want_iters = T.octree_model(keys, 64, 100)
    cap = want_tree.size + 4096
    tree, counts = T.root(kb), np.array([keys.size], np.uint32)
    tbuf, cbuf = api.buffers(tree, counts, cap)
    tree, counts, steps = step_until_converged(api, oracle, keys, 64, tree, counts, tbuf, cbuf, cap, 100)
    assert steps == want_iters > 4
    assert np.array_equal(tree, want_tree) and np.array_equal(counts, want_counts)
    got_tree, got_counts, iters = api.compute(keys, 64, cap, 100)
    assert iters == want_iters and np.array_equal(got_tree, want_tree) and np.array_equal(got_counts, want_counts)


@KB
def test_capacity_on_a_step_with_merges_and_splits(be, kb):
    api = T.Api(be, kb)
    bucket = 16
    _, tree, _ = T.cloud_tree(kb, 40000, bucket)
    other = T.clustered_keys(kb, 60000, seed=2)
    counts = T.counts_model(tree, other)
    ops, _ = T.ops_model(tree, counts, bucket)
    want_tree, want_counts, _ = T.update_model(other, bucket, tree, counts)
    nl, m = tree.size - 1, want_tree.size - 1
    assert (ops == 0).any() and (ops > 1).any() and m - 1 >= nl  # (a smaller capacity than nl is a bad argument)
    dkeys = api.dev(other)

    tbuf, cbuf = api.buffers(tree, counts, m)
    assert api.update(dkeys, bucket, tbuf, cbuf, nl, m) == (0, m, 0)
    got_tree, got_counts = api.fetch(tbuf, cbuf, m)
    assert np.array_equal(got_tree, want_tree) and np.array_equal(got_counts, want_counts)

    tbuf, cbuf = api.buffers(tree, counts, m - 1)
    before = be.to_host(tbuf, T.KEY_DTYPE[kb]), be.to_host(cbuf, np.uint32)
    rc, needed, _ = api.update(dkeys, bucket, tbuf, cbuf, nl, m - 1)
    assert (rc, needed) == (T.E_CAPACITY, m)
    assert np.array_equal(be.to_host(tbuf, T.KEY_DTYPE[kb]), before[0])
    assert np.array_equal(be.to_host(cbuf, np.uint32), before[1])


# ----------------------------------------------------------------------------------------------------------------------
# premises: what the cases above can and cannot tell apart
# ----------------------------------------------------------------------------------------------------------------------
@KB
@pytest.mark.parametrize("variant", T.VARIANTS)
def test_premise_every_wrong_rule_is_told_apart(kb, variant):
    told = [name for name, tree, counts, bucket, _ in T.decision_cases(kb)
            if not np.array_equal(T.ops_model(tree, counts, bucket, variant=variant)[0],
                                  T.ops_model(tree, counts, bucket)[0])]
    assert told, f"no decision case tells {variant} from the true rule"


@KB
def test_premise_trees(oracle, kb):
    """the builders against OctreeMaker / halos_support and the oracle's own loop; the sizes the cases rely on"""
    import halos_support as H

    ml = T.MAX_LEVEL[kb]
    assert np.array_equal(T.deepest_path(kb), H.deep_tree(oracle, kb, 0, "mixed").leaves)
    assert T.deepest_path(kb).size - 1 == 7 * ml + 1
    m = T.maker(kb, ())
    assert np.array_equal(T.children(kb), m) and np.array_equal(T.uniform(kb, 0), T.root(kb))
    keys, tree, counts = T.big_tree(kb)
    assert 5e4 < tree.size < 2e5
    ref_tree, ref_counts = oracle.compute_octree(keys, T.BIG_CLOUD[1])
    assert np.array_equal(ref_tree, tree) and np.array_equal(ref_counts, counts)
    assert T.uniform(kb, 7).size == 1024 * 2048 + 1  # 2 097 153 ops: one more than 1024 scan tiles
