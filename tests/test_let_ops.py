"""The device operations behind the host state machine of the locally essential tree (csrc/let.hpp), each called ON ITS
OWN through the C ABI of include/cstone_hip.h and compared with `==` against a numpy model written from the contract
comment in that header and the reference lines it cites (the models: tests/let_ops_support.py).

Covered here: halo_requests, halo_request_rows, peer_range_counts, add_macs, adjacent_difference_u32 (the first three
tests, GPU only, as before) and keys_missing, partition_keys, zero_ops_at_keys, locate_nodes, node_layout,
ranges_from_keys, gather_ranges_rows, scatter_rows, gather_tables_u32, focus_update_ops, find_peers_mac,
build_octree_bounded, upsweep_sum_bounded and upload.  Every test of the second group runs on two backends with the same
body: `cpu` (no marker: host memory, the ABI served by the project's CPU restatement, oracle/libcstone_cabi_oracle.so)
checks the MODEL where no GPU is needed; `hip` (@gpu: torch tensors, libcstone_hip.so) lets the model judge the kernels.
Sizes: 0 / 1 elements, 255 / 256 / 257 (253 / 260 leaves for trees, whose leaf counts are 1 mod 7), 10^4..10^5 and about
10^6 (multi-block scans, thousands of workgroups); leaf arrays are cornerstone trees of a clustered cloud, resolved up to
the end key (2^30 / 2^63).  The end-to-end runs of the same operations: tests/test_let.py, tests/test_distributed.py."""
import ctypes as C

import numpy as np
import pytest

import let_ops_support as S
from oracle import oracle as orc

gpu = pytest.mark.gpu


def _torch():
    import torch

    return torch


def dev(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.uint8): np.uint8}.get(a.dtype)
    if view is not None and a.dtype != np.uint8:
        a = a.view(view)
    return torch.from_numpy(a.copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def requests_model(leaves, flags, first, last, ranges):
    """extractMarkedElements per peer (R/domain/layout.hpp:104-139): runs of flagged leaves inside each peer's range as
    (first key, key behind the last) pairs; flagged leaves outside every range and outside [first, last) are unmatched"""
    pairs, counts = [], []
    owned = np.zeros(len(flags), bool)
    for a, b in ranges:
        c = 0
        while a != b:
            while a < b and flags[a] == 0:
                owned[a] = True
                a += 1
            if a != b:
                pairs.append(leaves[a])
                while a < b and flags[a] == 1:
                    owned[a] = True
                    a += 1
                pairs.append(leaves[a])
                c += 1
        counts.append(c)
    outside = np.ones(len(flags), bool)
    outside[first:last] = False
    return np.array(pairs, leaves.dtype), counts, int(np.count_nonzero((flags != 0) & ~owned & outside))


@gpu
@pytest.mark.parametrize("kb", [32, 64])
def test_halo_request_rows_equal_the_host_variant_and_the_model(hip, kb):
    torch = _torch()
    rng = np.random.default_rng(5)
    kdt = np.uint32 if kb == 32 else np.uint64
    for L, P, fail in ((5000, 4, 0), (70000, 7, 0), (300, 3, 1), (4096, 2, 0)):
        top = (1 << (30 if kb == 32 else 63)) - 1
        leaves = np.sort(rng.choice(top, L + 1, replace=False).astype(kdt))
        cuts = np.sort(rng.choice(np.arange(1, L), P - 1, replace=False))
        bounds = np.concatenate([[0], cuts, [L]])
        me = int(rng.integers(0, P))
        first, last = int(bounds[me]), int(bounds[me + 1])
        flags = (rng.random(L) < 0.3).astype(np.int32)
        flags[first:last] = 0
        # the peers: every rank but me and (if there are more than two) one other, whose flagged leaves are unmatched
        skip = (me + 1) % P if P > 2 else -1
        ranges = np.zeros((P, 2), np.int32)
        for r in range(P):
            if r != me and r != skip:
                ranges[r] = bounds[r], bounds[r + 1]
        want_pairs, want_counts, want_bad = requests_model(leaves, flags, first, last, [tuple(r) for r in ranges])

        dl, df = dev(leaves), dev(flags)
        pairs_a = torch.zeros(L + 2, dtype=dl.dtype, device="cuda")
        counts = (C.c_uint32 * P)()
        bad = C.c_uint32(77)
        rr = (C.c_int32 * (2 * P))(*[int(v) for v in ranges.ravel()])
        hip._chk(hip.lib.cstone_hip_halo_requests(hip.h, C.c_int(kb), ptr(dl), ptr(df), C.c_int(L), C.c_int(first),
                                                  C.c_int(last), rr, C.c_int(P), ptr(pairs_a), counts, C.byref(bad)),
                 "halo_requests")
        assert list(counts) == want_counts and bad.value == want_bad
        assert np.array_equal(host(pairs_a, kdt)[:want_pairs.size], want_pairs)

        pairs_b = torch.zeros(L + 2, dtype=dl.dtype, device="cuda")
        row = torch.full((P + 1,), -1, dtype=torch.int64, device="cuda")
        hip._chk(hip.lib.cstone_hip_halo_request_rows(hip.h, C.c_int(kb), ptr(dl), ptr(df), C.c_int(L), C.c_int(first),
                                                      C.c_int(last), rr, C.c_int(P), ptr(pairs_b), ptr(row), C.c_int(fail)),
                 "halo_request_rows")
        hip.sync()
        got = host(row, np.uint64)
        assert [int(v) for v in got[:P]] == [2 * c for c in want_counts]  # keys, i.e. two per pair
        assert int(got[P]) == (2 if fail else (1 if want_bad else 0))
        assert np.array_equal(host(pairs_b, kdt)[:want_pairs.size], want_pairs)


@gpu
def test_peer_range_counts(hip):
    """the treelet sizes of syncTreelets from the search results of translateAssignment (exchange_focus.hpp:61-96):
    row[p] = leaves over rank p's range + 1 for a peer, 0 otherwise"""
    torch = _torch()
    rng = np.random.default_rng(6)
    for P in (1, 2, 5, 64, 300):
        above = np.sort(rng.integers(0, 10**6, P + 1)).astype(np.uint64)          # findNodeAbove(assignment[r])
        below_plus = above + rng.integers(0, 3, P + 1).astype(np.uint64)           # first leaf >= assignment[r] + 1
        bounds = np.concatenate([above, below_plus])
        peer = (rng.random(P) < 0.5).astype(np.uint8)
        want = []
        for p in range(P):
            s, e = int(above[p]), int(below_plus[p + 1]) - 1
            e = max(e, s)
            want.append((e - s) + 1 if peer[p] else 0)
        row = torch.full((P,), -1, dtype=torch.int64, device="cuda")
        db = dev(bounds)
        hip._chk(hip.lib.cstone_hip_peer_range_counts(hip.h, ptr(db), (C.c_uint8 * P)(*peer.tolist()), C.c_int(P),
                                                      ptr(row)), "peer_range_counts")
        hip.sync()
        assert [int(v) for v in host(row, np.uint64)] == want


@gpu
def test_add_macs_and_adjacent_difference(hip):
    torch = _torch()
    rng = np.random.default_rng(8)
    for L in (1, 63, 1000, 123457):
        M = L + (L - 1) // 7
        macs = (rng.random(M) < 0.2).astype(np.int8)
        lti = rng.permutation(M)[:L].astype(np.int32)  # node of every leaf
        flags = (rng.random(L) < 0.1).astype(np.int32)
        df, dm, dl = dev(flags), torch.from_numpy(macs).cuda(), dev(lti)  # (named: a temporary's block would be reused)
        hip._chk(hip.lib.cstone_hip_add_macs(hip.h, ptr(dm), ptr(dl), C.c_int(L), ptr(df)), "add_macs")
        want = np.where(macs[lti] != 0, 1, flags)  # FocusedOctree::addMacs: marked leaves become halo candidates
        assert np.array_equal(df.cpu().numpy(), want)
        offs = np.concatenate([[0], np.cumsum(rng.integers(0, 50, L))]).astype(np.uint32)
        out = torch.zeros(L, dtype=torch.int32, device="cuda")
        do = dev(offs)
        hip._chk(hip.lib.cstone_hip_adjacent_difference_u32(hip.h, ptr(do), C.c_size_t(L), ptr(out)),
                 "adjacent_difference")
        assert np.array_equal(host(out, np.uint32), np.diff(offs))


# ----------------------------------------------------------------------------------------------------------------------
# every further operation on two backends: the CPU restatement behind the ABI (checks the model) and the HIP library
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["cpu", pytest.param("hip", marks=gpu)])
def be(request):
    if request.param == "cpu":
        return S.cpu_backend()
    return S.HipBackend(request.getfixturevalue("hip"))


KB = pytest.mark.parametrize("kb", [32, 64])
SIZES = (0, 1, 255, 256, 257, 30011, 1000003)
BIG_CLOUD = {32: 1000000, 64: 600000}  # particles for about 10^6 leaves with bucket size 2


def trees(oracle, kb):
    """(name, particle keys, leaves, counts): a few thousand, about 10^5 and about 10^6 leaves"""
    return [(name,) + S.cloud_tree(oracle, kb, n, 2) for name, n in
            (("small", 3000), ("mid", 60000), ("big", BIG_CLOUD[kb]))]


def tree_for(oracle, kb, n):
    """the tree an array operation of n elements works against: the 10^6-leaf tree for the largest size"""
    return S.cloud_tree(oracle, kb, BIG_CLOUD[kb] if n > 100000 else 60000, 2)


@KB
def test_keys_missing(be, oracle, kb):
    rng = np.random.default_rng(11)
    root = np.array([0, orc.end_key(kb)], orc.key_dtype(kb))
    for n in SIZES:
        for leaves in (tree_for(oracle, kb, n)[1], root):
            keys = S.sample_keys(rng, leaves, n)
            dl, dk = be.to_dev(leaves), be.to_dev(keys)
            out = be.filled(n, np.uint32, 77)
            be.chk(be.lib.cstone_hip_keys_missing(be.ctx, C.c_int(kb), be.ptr(dl), C.c_int(leaves.size - 1), be.ptr(dk),
                                                  C.c_size_t(n), be.ptr(out)), "keys_missing")
            got, want = be.to_host(out, np.uint32), S.keys_missing_model(leaves, keys)
            assert np.array_equal(want, (~np.isin(keys, leaves)).astype(np.uint32))
            assert np.array_equal(got, want), (n, leaves.size)
            if n > 1000 and leaves.size > 2:  # the inputs held both answers, the end key and the first key among them
                assert 0 < int(want.sum()) < n and want[keys == leaves[-1]].size and not want[keys == leaves[-1]].any()
                assert not want[keys == leaves[0]].any()


@KB
def test_partition_keys(be, oracle, kb):
    rng = np.random.default_rng(12)
    kdt = orc.key_dtype(kb)
    sentinel = kdt(0x2BADBADB)
    for n in SIZES:
        keys = S.sample_keys(rng, tree_for(oracle, kb, n)[1], n)
        for density in (0.3, 0.0, 1.0):
            flags = (rng.random(n) < density).astype(np.uint32)
            df, dk = be.to_dev(flags), be.to_dev(keys)
            scan = be.filled(n, np.uint32, 99)
            # the scan the state machine uses: the project's own exclusive scan of the flags
            be.chk(be.lib.cstone_hip_exclusive_scan_u32(be.ctx, be.ptr(df), be.ptr(scan), C.c_size_t(n), C.c_uint32(0)),
                   "exclusive_scan")
            want_set, want_unset = S.partition_keys_model(keys, flags)
            for use_set, use_unset in ((True, True), (True, False), (False, True)):
                so = be.filled(n, kdt, sentinel) if use_set else None
                uo = be.filled(n, kdt, sentinel) if use_unset else None
                be.chk(be.lib.cstone_hip_partition_keys(be.ctx, C.c_int(kb), be.ptr(dk), be.ptr(df), be.ptr(scan),
                                                        C.c_size_t(n), be.ptr(so), be.ptr(uo)), "partition_keys")
                for buf, want in ((so, want_set), (uo, want_unset)):
                    if buf is not None:  # the keys in input order, nothing behind them
                        got = be.to_host(buf, kdt)
                        assert np.array_equal(got[:want.size], want) and (got[want.size:] == sentinel).all(), (n, density)


@KB
def test_zero_ops_at_keys(be, oracle, kb):
    rng = np.random.default_rng(13)
    for n in SIZES:
        leaves = tree_for(oracle, kb, n)[1]
        nl = leaves.size - 1
        keys = S.sample_keys(rng, leaves, n)            # boundaries, keys inside leaves, the end key, duplicates
        if n == 257:
            keys[:] = leaves[nl // 2] + 1               # all on one entry: idempotent stores
        if n == 256:
            keys[:] = leaves[rng.integers(0, nl + 1, n)]  # boundaries only
        ops = (np.arange(nl + 1, dtype=np.int32) * 7 + 3)
        dl, dk, do = be.to_dev(leaves), be.to_dev(keys), be.to_dev(ops)
        be.chk(be.lib.cstone_hip_zero_ops_at_keys(be.ctx, C.c_int(kb), be.ptr(dl), C.c_int(nl), be.ptr(dk),
                                                  C.c_size_t(n), be.ptr(do)), "zero_ops_at_keys")
        want = S.zero_ops_model(leaves, keys, ops)
        assert np.array_equal(be.to_host(do, np.int32), want), n
        if n == 257:
            assert np.count_nonzero(want == 0) == 1 and want[nl // 2 + 1] == 0  # the NEXT boundary
        if n > 1000:
            assert want[nl] == 0 and 0 < np.count_nonzero(want == 0) < nl     # the end key was among them


def node_keys(octree, kb):
    """start and end key of every node of the linked tree from its prefix (placeholder bit above 3 * level key bits)"""
    ml = orc.max_level(kb)
    pre = octree["prefixes"].astype(np.uint64)
    level = (S.bit_length(pre) - 1) // 3
    shift = (3 * (ml - level)).astype(np.uint64)
    start = (pre ^ (np.uint64(1) << (3 * level).astype(np.uint64))) << shift
    return start, start + (np.uint64(1) << shift), level


@KB
def test_locate_nodes(be, oracle, kb):
    rng = np.random.default_rng(14)
    kdt, end = orc.key_dtype(kb), orc.end_key(kb)
    for name, _, leaves, _ in trees(oracle, kb):
        o = S.linked(oracle, leaves)
        nn = o["num_nodes"]
        start, stop, level = node_keys(o, kb)
        order = rng.permutation(nn)
        cases = {
            # consecutive leaf keys: every pair is a leaf node
            "leaves": leaves,
            # (start, end) of every node, leaf and internal, in random order: the pairs at even positions are nodes, the
            # pairs in between run backwards, span several nodes or are no cell at all
            "nodes": np.stack([start[order], stop[order]], axis=1).reshape(-1),
            "root": np.array([0, end]),
            # num_keys - 1 = 255, 256, 257 pairs: one workgroup either side
            "256 keys": leaves[-256:], "257 keys": leaves[-257:], "258 keys": leaves[-258:],
            "256 node keys": np.stack([start[order], stop[order]], axis=1).reshape(-1)[:256],
            "257 node keys": np.stack([start[order], stop[order]], axis=1).reshape(-1)[:257],
            "258 node keys": np.stack([start[order], stop[order]], axis=1).reshape(-1)[:258],
            "one key": np.array([7]),
            "none": np.zeros(0),
        }
        # valid cells that this tree does not hold: the first child of a leaf, and the cell one level above a node whose
        # parent it is not (shifted by one cell of that size)
        li = o["leaf_to_internal"][o["num_internal"]:]
        can = (stop[li] - start[li]) >= 8
        child = np.stack([start[li][can], start[li][can] + (stop[li][can] - start[li][can]) // np.uint64(8)], axis=1)
        cases["absent children"] = child.reshape(-1)
        # ranges of 2 .. 9 smallest cells, misaligned starts, sorted random keys, equal neighbours
        r = np.sort(rng.integers(0, end, 4000, dtype=np.uint64))
        cases["random"] = np.concatenate([r, r[:50] + np.uint64(5), r[50:100], r[50:100]])
        base = start[rng.integers(0, nn, 3000)]
        cases["short"] = np.stack([base, np.minimum(base + rng.integers(0, 10, 3000).astype(np.uint64), np.uint64(end))],
                                  axis=1).reshape(-1)
        found_levels = set()
        for what, keys in cases.items():
            keys = np.ascontiguousarray(keys).astype(kdt)
            n = keys.size
            dk, dp, dr = be.to_dev(keys), be.to_dev(o["prefixes"]), be.to_dev(o["level_range"])
            out = be.filled(max(n - 1, 0) + 2, np.int32, -5)
            be.chk(be.lib.cstone_hip_locate_nodes(be.ctx, C.c_int(kb), be.ptr(dk), C.c_size_t(n), be.ptr(dp), be.ptr(dr),
                                                  be.ptr(out)), "locate_nodes")
            got = be.to_host(out, np.int32)
            assert (got[max(n - 1, 0):] == -5).all(), (name, what)  # nothing written behind the num_keys - 1 results
            got = got[:max(n - 1, 0)]
            if n < 2:
                continue
            want = S.locate_nodes_model(keys, o["prefixes"], o["level_range"])
            assert np.array_equal(got, want), (name, what)
            if what == "leaves":
                assert np.array_equal(want, li)
            if what.endswith(" keys") and "node" not in what:
                assert np.array_equal(want, li[-want.size:])
            if what == "nodes":
                assert np.array_equal(want[0::2], order)
                found_levels |= set(level[want[0::2]].tolist())
            if what == "root":
                assert want[0] == 0
            if what == "absent children":
                assert (want[0::2] == nn).all()
        assert found_levels == set(np.unique(level).tolist())


def test_node_layout(be):
    rng = np.random.default_rng(15)
    for n in SIZES:
        for big in (False, True):
            counts = rng.integers(0, 1 << 31 if big else 64, n).astype(np.uint32)  # big: the sum passes 2^31 and 2^32
            flags = (rng.random(n) < 0.3).astype(np.int32)
            a, b = sorted(int(v) for v in rng.integers(0, n + 1, 2))
            for first, last in ((a, b), (a, a), (0, n)):
                dc, df = be.to_dev(counts), be.to_dev(flags)
                out = be.filled(n + 1, np.uint32, 0xDEAD)
                be.chk(be.lib.cstone_hip_node_layout(be.ctx, be.ptr(dc) if n else None, be.ptr(df) if n else None,
                                                     C.c_int(first), C.c_int(last), C.c_int(n), be.ptr(out)), "node_layout")
                want = S.node_layout_model(counts, flags, first, last)
                assert np.array_equal(be.to_host(out, np.uint32), want), (n, big, first, last)
                if (first, last) == (0, n):
                    assert int(want[-1]) == int(counts.astype(np.uint64).sum() & 0xFFFFFFFF)
            if n > 1000 and not big:  # flags inside the own range change nothing: the entry with and without them
                assert flags[a:b].any()
                cleared = flags.copy()
                cleared[a:b] = 0
                got = []
                for f in (flags, cleared):
                    dc, df = be.to_dev(counts), be.to_dev(f)
                    out = be.filled(n + 1, np.uint32, 0xDEAD)
                    be.chk(be.lib.cstone_hip_node_layout(be.ctx, be.ptr(dc), be.ptr(df), C.c_int(a), C.c_int(b), C.c_int(n),
                                                         be.ptr(out)), "node_layout")
                    got.append(be.to_host(out, np.uint32))
                assert np.array_equal(got[0], got[1])


def call_ranges_from_keys(be, kb, leaves, layout, pairs):
    npairs = pairs.size // 2
    dl, dy, dp = be.to_dev(leaves), be.to_dev(layout), be.to_dev(pairs)
    off, scan = be.filled(npairs, np.uint32, 0xABCD), be.filled(npairs + 1, np.uint32, 0xABCD)
    be.chk(be.lib.cstone_hip_ranges_from_keys(be.ctx, C.c_int(kb), be.ptr(dl), C.c_int(leaves.size - 1), be.ptr(dy),
                                              be.ptr(dp) if npairs else None, C.c_size_t(npairs),
                                              be.ptr(off) if npairs else None, be.ptr(scan)), "ranges_from_keys")
    return be.to_host(off, np.uint32), be.to_host(scan, np.uint32), off, scan


@KB
def test_ranges_from_keys(be, oracle, kb):
    rng = np.random.default_rng(16)
    kdt = orc.key_dtype(kb)
    for n in SIZES:
        pkeys, leaves, counts = tree_for(oracle, kb, n)
        layout = np.searchsorted(pkeys, leaves).astype(np.uint32)  # every leaf present: index of its first particle
        # disjoint ascending pairs: leaf keys, keys inside leaves (round up), equal keys (empty), the end key last
        k = np.sort(S.sample_keys(rng, leaves, 2 * n))
        if n:
            k[-1] = leaves[-1]
        if n > 2:
            k[2] = k[3]
        off, scan, _, _ = call_ranges_from_keys(be, kb, leaves, layout, k.astype(kdt))
        want_off, want_scan = S.ranges_from_keys_model(leaves, layout, k.astype(kdt))
        assert np.array_equal(off, want_off) and np.array_equal(scan, want_scan), n
        assert scan[0] == 0
        if n > 1000:
            inside = ~np.isin(k[0::2], leaves)
            assert inside.any() and (np.diff(scan) == 0).any() and int(want_off[-1] + np.diff(scan)[-1]) == pkeys.size


@KB
def test_ranges_from_keys_serve_halo_requests(be, oracle, kb):
    """requested runs (halo_requests on a coarse tree's flags) -> served ranges on the owner's finer tree -> gather_ranges
    hands out exactly the particles of the flagged leaves"""
    rng = np.random.default_rng(17)
    kdt = orc.key_dtype(kb)
    for n_particles in (3000, 60000):
        pkeys, fine, _ = S.cloud_tree(oracle, kb, n_particles, 2)
        coarse, _ = oracle.compute_octree(pkeys, 64)  # every key of it is a boundary of the finer tree
        assert np.isin(coarse, fine).all()
        nl = coarse.size - 1
        first, last = nl // 3, 2 * nl // 3
        flags = (rng.random(nl) < 0.4).astype(np.int32)
        flags[first:last] = 0
        flags[0] = flags[nl - 1] = 1
        ranges = (C.c_int32 * 6)(0, first, 0, 0, last, nl)
        dl, df = be.to_dev(coarse), be.to_dev(flags)
        pairs = be.filled(2 * nl + 2, kdt, 0)
        pair_counts, bad = (C.c_uint32 * 3)(), C.c_uint32(9)
        be.chk(be.lib.cstone_hip_halo_requests(be.ctx, C.c_int(kb), be.ptr(dl), be.ptr(df), C.c_int(nl), C.c_int(first),
                                               C.c_int(last), ranges, C.c_int(3), be.ptr(pairs), pair_counts,
                                               C.byref(bad)), "halo_requests")
        npairs = sum(pair_counts)
        assert bad.value == 0 and pair_counts[1] == 0 and npairs > 10
        req = be.to_host(pairs, kdt)[:2 * npairs]
        layout = np.searchsorted(pkeys, fine).astype(np.uint32)
        off, scan, doff, dscan = call_ranges_from_keys(be, kb, fine, layout, req)
        want_off, want_scan = S.ranges_from_keys_model(fine, layout, req)
        assert np.array_equal(off, want_off) and np.array_equal(scan, want_scan)
        total = int(scan[-1])
        src, out = be.to_dev(pkeys), be.filled(total, kdt, 0)
        be.chk(be.lib.cstone_hip_gather_ranges(be.ctx, C.c_int(pkeys.itemsize), C.c_int(32), be.ptr(dscan), be.ptr(doff),
                                               C.c_int(npairs), be.ptr(src), be.ptr(out), C.c_size_t(total)),
               "gather_ranges")
        lo, hi = np.searchsorted(pkeys, coarse[:-1]), np.searchsorted(pkeys, coarse[1:])
        want = np.concatenate([pkeys[a:b] for a, b, f in zip(lo, hi, flags) if f])
        assert np.array_equal(be.to_host(out, kdt), want)
    # a pair whose keys are no leaf keys of the serving tree rounds up to the next boundary on both sides
    q = np.array([fine[5] + 1, fine[9] - 1, fine[-2] + 1, fine[-1]], kdt)
    off, scan, _, _ = call_ranges_from_keys(be, kb, fine, layout, q)
    assert list(off) == [layout[6], layout[-1]] and list(scan) == [0, layout[9] - layout[6], layout[9] - layout[6]]


def bit_patterns(rng, n, dtype):
    """distinct bit patterns: random bits (among them NaNs with payloads), -0.0, infinities and a quiet NaN"""
    bits = dtype(0).itemsize * 8
    a = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    a = (a ^ (a << np.uint64(1))).astype(dtype)
    special = [1 << (bits - 1), (0xFF8 if bits == 32 else 0xFFF) << (bits - 12), (0x7FC if bits == 32 else 0x7FF8) << (bits - 16),
               (0x7F8 if bits == 32 else 0x7FF) << (bits - 12 if bits == 64 else 20)]
    for i, v in enumerate(special[:n]):
        a[(i * 13) % n] = dtype(v & ((1 << bits) - 1))
    return a


@pytest.mark.parametrize("elem_bytes", [4, 8])
def test_gather_ranges_rows_and_scatter_rows(be, elem_bytes):
    rng = np.random.default_rng(18)
    edt = np.uint32 if elem_bytes == 4 else np.uint64
    nsrc = 1200000
    sources = [bit_patterns(rng, nsrc, edt) for _ in range(4)]
    dsrc = [be.to_dev(a) for a in sources]
    for num_rows in SIZES:
        for na in ((1, 2, 3, 4) if num_rows in (257, 30011) else (1 + num_rows % 4,)):
            # ranges with empty ones in between, in no particular order in the source
            nr = min(num_rows, 40) + 3
            cuts = np.sort(rng.integers(0, num_rows + 1, nr - 1))
            scan = np.concatenate([[0], cuts, [num_rows]]).astype(np.uint32)
            scan[2] = scan[1]
            scan.sort()
            lengths = np.diff(scan.astype(np.int64))
            off = np.array([rng.integers(0, nsrc - l + 1) for l in lengths], np.uint32)
            dscan, doff = be.to_dev(scan), be.to_dev(off)
            rows = be.filled(num_rows * na + 3, edt, 0x5A5A5A5A)
            be.chk(be.lib.cstone_hip_gather_ranges_rows(be.ctx, C.c_int(elem_bytes), C.c_int(na), be.ptr(dscan),
                                                        be.ptr(doff), C.c_int(nr), be.ptrs(dsrc[:na]), be.ptr(rows),
                                                        C.c_size_t(num_rows)), "gather_ranges_rows")
            got = be.to_host(rows, edt)
            want = S.gather_rows_model(off, scan, sources[:na]) if num_rows else np.zeros(0, edt)
            assert np.array_equal(got[:num_rows * na], want) and (got[num_rows * na:] == 0x5A5A5A5A).all(), (num_rows, na)
            # the receiving side, behind an offset, into arrays whose other elements must stay
            dst_offset = 11
            dst = [bit_patterns(rng, num_rows + 30, edt) for _ in range(na)]
            ddst = [be.to_dev(a) for a in dst]
            be.chk(be.lib.cstone_hip_scatter_rows(be.ctx, C.c_int(elem_bytes), C.c_int(na), be.ptr(rows),
                                                  C.c_size_t(num_rows), be.ptrs(ddst), C.c_size_t(dst_offset)),
                   "scatter_rows")
            want_dst = S.scatter_rows_model(want, na, dst, dst_offset)
            for a in range(na):
                got_a = be.to_host(ddst[a], edt)
                assert np.array_equal(got_a, want_dst[a]), (num_rows, na, a)
                # ... which is what one gather_ranges per array delivers
                one = be.filled(num_rows, edt, 0)
                be.chk(be.lib.cstone_hip_gather_ranges(be.ctx, C.c_int(elem_bytes), C.c_int(32), be.ptr(dscan),
                                                       be.ptr(doff), C.c_int(nr), be.ptr(dsrc[a]), be.ptr(one),
                                                       C.c_size_t(num_rows)), "gather_ranges")
                assert np.array_equal(got_a[dst_offset:dst_offset + num_rows], be.to_host(one, edt))
                if num_rows > 256 and a:
                    assert not np.array_equal(want_dst[a][dst_offset:dst_offset + num_rows],
                                              want_dst[0][dst_offset:dst_offset + num_rows])  # the columns differ


def test_gather_tables_u32(be):
    rng = np.random.default_rng(19)
    table = 5000
    a, b = [rng.integers(0, 1 << 32, table, dtype=np.uint64).astype(np.uint32) for _ in range(2)]
    da, db = be.to_dev(a), be.to_dev(b)
    for n_a, n_b, n_c in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (255, 256, 257), (300, 0, 23), (0, 300, 23),
                          (40000, 30011, 23), (500000, 500003, 1000)):
        c = rng.integers(0, 1 << 32, n_c + 1, dtype=np.uint64).astype(np.uint32)
        dc = be.to_dev(c)
        map_ = rng.integers(0, table, n_a + n_b).astype(np.uint32)  # repeated and out-of-order indices
        if map_.size > 4:
            map_[:4] = [table - 1, 0, table - 1, 0]
        dm = be.to_dev(map_)
        for null_a, null_c in ((False, False), (True, False), (False, True)):
            nc = 0 if null_c else n_c
            out = be.filled(n_a + n_b + nc + 2, np.uint32, 0x77)
            be.chk(be.lib.cstone_hip_gather_tables_u32(be.ctx, be.ptr(dm) if map_.size else None,
                                                       None if null_a else be.ptr(da), C.c_size_t(n_a),
                                                       be.ptr(db) if n_b else None, C.c_size_t(n_b),
                                                       None if null_c else be.ptr(dc), C.c_size_t(nc), be.ptr(out)),
                   "gather_tables_u32")
            want = S.gather_tables_model(map_, None if null_a else a, n_a, b, n_b, c, nc)
            got = be.to_host(out, np.uint32)
            assert np.array_equal(got[:want.size], want) and (got[want.size:] == 0x77).all(), (n_a, n_b, n_c, null_a, null_c)


def forced_keys(rng, leaves, counts_are_zero, m):
    """m mandatory keys: leaf boundaries (with 0 and the end key), keys one level below a leaf (a split is needed), keys
    two levels below"""
    out = []
    nl = leaves.size - 1
    for _ in range(m):
        i = int(rng.integers(0, nl))
        a, span = int(leaves[i]), int(leaves[i + 1]) - int(leaves[i])
        kind = int(rng.integers(0, 3))
        if kind == 0 or span < 64:
            out.append(a)
        elif kind == 1:
            out.append(a + int(rng.integers(1, 8)) * (span // 8))
        else:
            out.append(a + int(rng.integers(1, 64)) * (span // 64))
    return np.array(out, leaves.dtype)


def call_focus_update(be, kb, o, nl, counts, macs, fs, fe, bucket, forced):
    nn = o["num_nodes"]
    l2i = np.ascontiguousarray(o["leaf_to_internal"][o["num_internal"]:])
    dev = {k: be.to_dev(v) for k, v in (("pre", o["prefixes"]), ("co", o["child_offsets"]), ("pa", o["parents"]),
                                        ("cnt", counts), ("mac", macs), ("fk", forced), ("l2i", l2i))}
    ops, leaf_ops = be.filled(nn, np.int32, -7), be.filled(nl + 1, np.int32, -7)
    res = (C.c_int * 4)(-1, -1, -1, -1)
    be.chk(be.lib.cstone_hip_focus_update_ops(
        be.ctx, C.c_int(kb), be.ptr(dev["pre"]), be.ptr(dev["co"]), be.ptr(dev["pa"]) if nn > 1 else None,
        be.ptr(dev["cnt"]), be.ptr(dev["mac"]), C.c_uint64(fs), C.c_uint64(fe), C.c_uint32(bucket),
        be.ptr(dev["fk"]) if forced.size else None, C.c_int(forced.size), be.ptr(dev["l2i"]), C.c_int(nl), C.c_int(nn),
        be.ptr(ops), be.ptr(leaf_ops), res), "focus_update_ops")
    # the three single entries one after the other
    ops3 = be.filled(nn, np.int32, -9)
    be.chk(be.lib.cstone_hip_rebalance_decision_essential(
        be.ctx, C.c_int(kb), be.ptr(dev["pre"]), be.ptr(dev["co"]), be.ptr(dev["pa"]) if nn > 1 else None,
        be.ptr(dev["cnt"]), be.ptr(dev["mac"]), C.c_uint64(fs), C.c_uint64(fe), C.c_uint32(bucket), be.ptr(ops3),
        C.c_int(nn)), "rebalance_decision_essential")
    status, conv = C.c_int(-1), C.c_int(-1)
    be.chk(be.lib.cstone_hip_enforce_keys(be.ctx, C.c_int(kb), be.ptr(dev["fk"]) if forced.size else None,
                                          C.c_int(forced.size), be.ptr(dev["pre"]), be.ptr(dev["co"]),
                                          be.ptr(dev["pa"]) if nn > 1 else None, be.ptr(ops3), C.byref(status)),
           "enforce_keys")
    be.chk(be.lib.cstone_hip_protect_ancestors(be.ctx, C.c_int(kb), be.ptr(dev["pre"]),
                                               be.ptr(dev["pa"]) if nn > 1 else None, be.ptr(ops3), C.c_int(nn),
                                               C.byref(conv)), "protect_ancestors")
    return be.to_host(ops, np.int32), be.to_host(leaf_ops, np.int32), list(res), be.to_host(ops3, np.int32), status.value


@KB
def test_focus_update_ops(be, oracle, kb):
    rng = np.random.default_rng(20)
    end = orc.end_key(kb)
    root = np.array([0, end], orc.key_dtype(kb))
    inputs = [("root", root, np.array([5], np.uint32)), ("253", S.split_tree(kb, 36, 3), None),
              ("260", S.split_tree(kb, 37, 4), None)]
    inputs += [(name, leaves, counts) for name, _, leaves, counts in trees(oracle, kb)]
    seen = set()

    def run_case(tag, o, nl, counts, macs, fs, fe, bucket, fk):
        want_ops, want_scan, want_res = S.focus_update_model(oracle, o, counts, macs, fs, fe, bucket, fk)
        ops, leaf_ops, res, ops3, status3 = call_focus_update(be, kb, o, nl, counts, macs, fs, fe, bucket, fk)
        assert res == want_res, (tag, res, want_res)
        assert np.array_equal(ops, want_ops), tag
        assert np.array_equal(leaf_ops, want_scan), tag
        assert np.array_equal(ops, ops3) and status3 == res[0], tag  # the fusion == its three parts
        seen.add((min(res[0], 2), res[1]))
        return res

    for name, leaves, leaf_counts in inputs:
        nl = leaves.size - 1
        o = S.linked(oracle, leaves) if nl > 300 else oracle.build_octree(leaves)
        nn = o["num_nodes"]
        if leaf_counts is None:
            leaf_counts = rng.integers(0, 5, nl).astype(np.uint32)
        variants = [
            # the tree's own counts, everything in focus, boundaries enforced: nothing to do
            ("own", leaf_counts, np.zeros(nn, np.int8), 0, end, 2 if nl > 300 else 1 << 20, 0),
            # random counts and MAC flags, a focus in the middle
            ("random", rng.integers(0, 4, nl).astype(np.uint32), (rng.random(nn) < 0.4).astype(np.int8),
             int(leaves[nl // 3]), int(leaves[max(2 * nl // 3, 1)]), 2, None),
            # an empty, MAC-free exterior that wants to merge
            ("empty", np.zeros(nl, np.uint32), np.zeros(nn, np.int8), int(leaves[nl // 2]), int(leaves[nl // 2 + 1]),
             16, None),
        ]
        for vname, lc, macs, fs, fe, bucket, _ in variants:
            counts = oracle.upsweep_counts(o, lc)
            key_sets = [np.zeros(0, leaves.dtype), leaves[[nl // 2]], leaves[rng.integers(0, nl + 1, 40)],
                        forced_keys(rng, leaves, False, 1), forced_keys(rng, leaves, False, 60)]
            for fk in key_sets:
                if name == "big" and fk.size not in (0, 60):
                    continue
                run_case((name, vname, fk.size), o, nl, counts, macs, fs, fe, bucket, fk)
    # status 1 with nothing left to do: two levels below the root, an empty exterior that wants to merge both, and one
    # enforced boundary among the deepest leaves, which cancels every merge above it
    leaves = S.split_tree(kb, 2, 5, deep=True)
    nl = leaves.size - 1
    o = oracle.build_octree(leaves)
    small = int(np.argmin(np.diff(leaves.astype(np.uint64))))
    res = run_case("cancelled merges", o, nl, np.zeros(o["num_nodes"], np.uint32), np.zeros(o["num_nodes"], np.int8), 0, 0,
                   16, leaves[[small + 3]])
    assert res == [1, 1, 1, nl]
    # status 1 where the two verdicts DIFFER: the first two children of the root resolved to level 3, the others to
    # level 2, one particle per leaf, nothing in focus, MAC flags everywhere but on those two children.  Their level-2
    # nodes (internal) want to merge, every leaf keeps.  The enforced boundary, the 4th level-2 node under the first
    # child, cancels the merges of that child's group only: protectAncestors still sees the zeros under the second
    # child (its verdict: not converged), but with cancelMerge updateFocus asks the LEAVES (R/focus/octree_focus.hpp:
    # 114-117) -> converged
    end8 = end // 8
    keys = [c * end8 + g * (end8 // 64) for c in (0, 1) for g in range(64)] + \
           [c * end8 + g * (end8 // 8) for c in range(2, 8) for g in range(8)] + [end]
    leaves = np.array(keys, orc.key_dtype(kb))
    nl = leaves.size - 1
    o = oracle.build_octree(leaves)
    start, _, level = node_keys(o, kb)
    macs = np.ones(o["num_nodes"], np.int8)
    macs[(level == 1) & (start < 2 * end8)] = 0
    counts = oracle.upsweep_counts(o, np.ones(nl, np.uint32))
    fk = np.array([3 * (end8 // 8)], leaves.dtype)
    ops = oracle.essential_ops(o, counts, macs, 0, 0, 4)
    ops, status = oracle.enforce_keys(fk, o, ops)
    ops, protect_verdict = oracle.protect_ancestors(o, ops)
    assert status == 1 and not protect_verdict and (ops[o["leaf_to_internal"][o["num_internal"]:]] == 1).all()
    res = run_case("verdicts differ", o, nl, counts, macs, 0, 0, 4, fk)
    assert res == [1, 1, 1, nl]
    # each of the three rules for `converged` decided cases: status 0 (protectAncestors' verdict) and status 1 (every
    # leaf keeps) both ways, status >= 2 (never)
    assert {(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)} == seen, seen


@pytest.mark.parametrize("kb,curve", [(32, orc.HILBERT), (64, orc.HILBERT), (64, orc.MORTON)])
def test_find_peers_mac(be, oracle, kb, curve):
    rng = np.random.default_rng(21 + kb + curve)
    cpu = S.cpu_backend()
    boxes = [orc.Box([0, 1], (0, 0, 0)), orc.Box([-1.0, 1.0, 0.0, 0.5, 2.0, 5.0], (1, 1, 1)),
             orc.Box([0.0, 3.0, -1.0, 1.0, 0.0, 1.0], (0, 1, 0))]
    import cstone_amd

    checked = 0
    for n_particles, bucket in ((1500, 2), (4000, 4)):
        _, leaves, _ = S.cloud_tree(oracle, kb, n_particles, bucket, seed=5, curve=curve)
        nl = leaves.size - 1
        o = S.linked(oracle, leaves) if nl > 300 else oracle.build_octree(leaves)
        dp, dc, dr = be.to_dev(o["prefixes"]), be.to_dev(o["child_offsets"]), be.to_dev(o["level_range"])
        for bi, box in enumerate(boxes):
            center, size = S.leaf_boxes(oracle, curve, leaves, box)
            cbox = cstone_amd.make_cbox(box.lim, box.bc)
            for num_ranks in ((2, 5, 33, 300) if n_particles == 1500 else (5, 300)):  # (the model costs ranks x leaves^2)
                # cuts at random leaf boundaries, with repeats: ranks with an empty range
                cuts = np.sort(rng.integers(0, nl + 1, num_ranks - 1))
                if num_ranks > 4:
                    cuts[1] = cuts[0]
                assignment = np.concatenate([[0], leaves[cuts].astype(np.uint64), [orc.end_key(kb)]]).astype(np.uint64)
                base = [1 / 0.57 + 0.5, 1 / 0.83 + 0.5, 1 / 0.41][(bi + num_ranks) % 3]
                for my_rank in sorted({0, num_ranks // 2, num_ranks - 1}):
                    # no leaf pair within a relative 1e-9 (double) resp. 1e-6 (float) of a MAC threshold: a condition
                    # on the INPUTS, met by moving the opening parameter a little until the model reports none.  (The
                    # float margin covers the rounding of the MAC products and sums; the cell centres are sums of a
                    # few dyadic multiples of the box lengths and lose little.  Should a compiler change ever flip a
                    # float verdict with no fault in the kernel, the inputs are to be changed, not the comparison.)
                    for k in range(8):
                        inv_theta = float(np.float32(base * (1 + 0.003 * k)))
                        want, near = S.peers_model(leaves, center, size, box, assignment, my_rank, inv_theta)
                        if near == [0, 0]:
                            break
                    assert near == [0, 0], "input too close to a MAC threshold: choose another seed"
                    flags = {}
                    for rb, backend in ((64, be), (32, be)) + (((32, cpu),) if be is not cpu else ()):
                        p = ((dp, dc, dr) if backend is be else
                             tuple(cpu.to_dev(o[k]) for k in ("prefixes", "child_offsets", "level_range")))
                        out = (C.c_int32 * num_ranks)(*([-1] * num_ranks))
                        backend.chk(backend.lib.cstone_hip_find_peers_mac(
                            backend.ctx, C.c_int(curve), C.c_int(kb), C.c_int(rb), backend.ptr(p[0]), backend.ptr(p[1]),
                            backend.ptr(p[2]), assignment.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_int(num_ranks),
                            C.c_int(my_rank), C.byref(cbox), C.c_float(inv_theta), out), "find_peers_mac")
                        flags[(rb, backend.name)] = np.array(list(out), np.int32)
                    assert np.array_equal(flags[(64, be.name)], want), (n_particles, bi, num_ranks, my_rank)
                    if be is not cpu:  # float: against the CPU restatement evaluated in float
                        assert np.array_equal(flags[(32, be.name)], flags[(32, "cpu")]), (n_particles, bi, num_ranks, my_rank)
                    else:  # the float restatement itself: with the float margin kept, the verdicts of the double model
                        assert np.array_equal(flags[(32, "cpu")], want), (n_particles, bi, num_ranks, my_rank)
                    assert want[my_rank] == 0
                    checked += int(want.sum())
    assert checked > 100


def deep_branch_tree(kb):
    return S.split_tree(kb, orc.max_level(kb), 9, deep=True)


@KB
def test_build_octree_bounded_and_upsweep_sum_bounded(be, oracle, kb):
    rng = np.random.default_rng(22)
    ml = orc.max_level(kb)
    root = np.array([0, orc.end_key(kb)], orc.key_dtype(kb))
    inputs = [("root", root), ("eight", S.split_tree(kb, 1, 1)), ("deep branch", deep_branch_tree(kb)),
              ("253", S.split_tree(kb, 36, 3)), ("260", S.split_tree(kb, 37, 4))]
    inputs += [(name, leaves) for name, _, leaves, _ in trees(oracle, kb)]
    names = ("prefixes", "child_offsets", "parents", "level_range", "internal_to_leaf", "leaf_to_internal")
    for name, leaves in inputs:
        nl = leaves.size - 1
        want = oracle.build_octree(leaves)
        nn = want["num_nodes"]
        deepest = int(S.leaf_levels(leaves).max())
        if name == "deep branch":
            assert deepest == ml and nl == 7 * ml + 1
        dl = be.to_dev(leaves)
        sizes = dict(prefixes=(nn, leaves.dtype), child_offsets=(nn + 1, np.int32), parents=(max(1, (nn - 1) // 8), np.int32),
                     level_range=(ml + 2, np.int32), internal_to_leaf=(nn, np.int32), leaf_to_internal=(nn, np.int32))
        leaf_counts = [rng.integers(0, 100, nl).astype(np.uint32), np.full(nl, 1 << 31, np.uint32),
                       np.where(rng.random(nl) < 0.5, 0xFFFFFFFF, 0).astype(np.uint32)]
        results = {}
        for bound in sorted({deepest, min(deepest + 1, ml), ml}) + [None]:
            bufs = {k: be.filled(n, dt, 0) for k, (n, dt) in sizes.items()}
            args = [be.ctx, C.c_int(kb), be.ptr(dl), C.c_int(nl)] + [be.ptr(bufs[k]) for k in names]
            if bound is None:
                be.chk(be.lib.cstone_hip_build_octree(*args), "build_octree")
            else:
                be.chk(be.lib.cstone_hip_build_octree_bounded(*args, C.c_int(bound)), "build_octree_bounded")
            got = {k: be.to_host(bufs[k], sizes[k][1]) for k in names}
            for k in names:
                n = (nn - 1) // 8 if k == "parents" else (nn if k == "child_offsets" else sizes[k][0])
                assert np.array_equal(got[k][:n], want[k][:n]), (name, bound, k)
            for ci, lc in enumerate(leaf_counts):
                q = np.zeros(nn, np.uint32)
                q[want["leaf_to_internal"][want["num_internal"]:]] = lc
                dq = be.to_dev(q)
                if bound is None:
                    be.chk(be.lib.cstone_hip_upsweep_sum(be.ctx, C.c_int(ml + 2), be.ptr(bufs["level_range"]),
                                                         be.ptr(bufs["child_offsets"]), be.ptr(dq)), "upsweep_sum")
                else:
                    be.chk(be.lib.cstone_hip_upsweep_sum_bounded(be.ctx, C.c_int(ml + 2), be.ptr(bufs["level_range"]),
                                                                 be.ptr(bufs["child_offsets"]), be.ptr(dq), C.c_int(bound)),
                           "upsweep_sum_bounded")
                results[(bound, ci)] = be.to_host(dq, np.uint32)
                assert np.array_equal(results[(bound, ci)], oracle.upsweep_counts(want, lc)), (name, bound, ci)
        if nl > 8:  # the saturating sum was reached, and not everywhere
            sat = results[(None, 1)]
            assert sat[0] == 0xFFFFFFFF and (sat == 1 << 31).any()


def test_upload(be):
    rng = np.random.default_rng(23)
    ring = 1 << 20  # bytes of the pinned staging ring (csrc/ctx.hip); a quarter of it is the largest staged upload
    sizes = [0, 1, 4, 255, 64 << 10, ring // 4, ring // 4 + 1, 1 << 20]
    sizes += [int(v) for v in rng.integers(1, 4096, 3000)]  # about 6 MiB in small pieces: several times round the ring
    starts = np.concatenate([[0], np.cumsum([(s + 7) // 8 * 8 + 8 for s in sizes])])
    total = int(starts[-1])
    dst = be.filled(total, np.uint8, 0xCC)
    want = np.full(total, 0xCC, np.uint8)
    src = np.zeros(max(sizes) + 8, np.uint8)
    for s, at in zip(sizes, starts[:-1]):
        at = int(at) + (1 if s % 3 == 1 else 0)  # some destinations off the 4-byte grid
        payload = rng.integers(0, 256, s, dtype=np.uint8)
        src[:s] = payload
        want[at:at + s] = payload
        be.chk(be.lib.cstone_hip_upload(be.ctx, be.ptr(dst, at), C.c_void_p(src.ctypes.data), C.c_size_t(s)), "upload")
        src[:] = 0xEE  # the contract: the source may be reused as soon as the call returns
    be.sync()
    got = be.to_host(dst, np.uint8)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


@gpu
def test_bad_arguments_are_refused_on_the_host(hip):
    """one call per entry with a null required pointer or bad key_bits: CSTONE_E_ARG, last_error set, nothing launched"""
    be = S.HipBackend(hip)
    lib, ctx = be.lib, be.ctx
    good = be.filled(64, np.uint64, 0)  # a valid allocation wherever a pointer is not the one under test
    g, null = be.ptr(good), None
    res, st = (C.c_int * 4)(), (C.c_int32 * 4)()
    box = C.create_string_buffer(64)
    one = C.c_uint64 * 2
    calls = {
        "keys_missing": lambda: lib.cstone_hip_keys_missing(ctx, 48, g, 1, g, C.c_size_t(1), g),
        "partition_keys": lambda: lib.cstone_hip_partition_keys(ctx, 32, g, null, g, C.c_size_t(1), g, g),
        "zero_ops_at_keys": lambda: lib.cstone_hip_zero_ops_at_keys(ctx, 64, g, 1, g, C.c_size_t(1), null),
        "locate_nodes": lambda: lib.cstone_hip_locate_nodes(ctx, 64, g, C.c_size_t(2), null, g, g),
        "node_layout": lambda: lib.cstone_hip_node_layout(ctx, g, g, 0, 1, 1, null),
        "ranges_from_keys": lambda: lib.cstone_hip_ranges_from_keys(ctx, 16, g, 1, g, g, C.c_size_t(1), g, g),
        "gather_ranges_rows": lambda: lib.cstone_hip_gather_ranges_rows(ctx, 4, 5, g, g, 1, be.ptrs([good]), g, C.c_size_t(1)),
        "scatter_rows": lambda: lib.cstone_hip_scatter_rows(ctx, 8, 1, null, C.c_size_t(1), be.ptrs([good]), C.c_size_t(0)),
        "gather_tables": lambda: lib.cstone_hip_gather_tables_u32(ctx, null, g, C.c_size_t(1), g, C.c_size_t(0), g,
                                                                   C.c_size_t(0), g),
        "focus_update_ops": lambda: lib.cstone_hip_focus_update_ops(ctx, 64, g, g, g, g, g, C.c_uint64(0), C.c_uint64(8),
                                                                    C.c_uint32(1), null, 0, g, 1, 1, g, null, res),
        "find_peers_mac": lambda: lib.cstone_hip_find_peers_mac(ctx, 1, 64, 16, g, g, g, one(0, 8), 1, 0, box,
                                                                C.c_float(1.0), st),
        "build_octree_bounded": lambda: lib.cstone_hip_build_octree_bounded(ctx, 64, g, 1, g, g, g, g, g, null, 3),
        "upsweep_sum_bounded": lambda: lib.cstone_hip_upsweep_sum_bounded(ctx, 23, g, g, null, 3),
        "upload": lambda: lib.cstone_hip_upload(ctx, g, null, C.c_size_t(8)),
    }
    for name, call in calls.items():
        lib.cstone_hip_raise(ctx, 0, b"marker")
        assert call() == S.E_ARG, name
        assert name in be.last_error(), (name, be.last_error())
    be.sync()
    assert (be.to_host(good, np.uint64) == 0).all()
