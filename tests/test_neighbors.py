"""The neighbour search (csrc/neighbors.hip, cstone_hip::traverseNeighbors) on the boxes and trees the other suites
never show it: anisotropic boxes under every mix of open, periodic and fixed faces, leaves of more than 64 particles,
a tree that is one leaf, the deepest walk a 64-bit Morton tree allows, the edges of the radius, ext != 1.

Three references.  The oracle (oracle.find_neighbors) is the reference for list ORDER at every shape; the CPU tests
first establish that it may serve: it equals the reference's own CPU code, its stored entries equal a numpy brute force
as sets, its lists equal a restatement of the depth-first walk in plain Python (tests/neighbors_support.py).  A
disagreement between brute force and oracle on a borderline pair would be a node pruned by rounding: it is not
tolerated away, the seeds used here are ones for which the two agree exactly.  The GPU tests then compare all four entry
points with the oracle, entry for entry, on lists pre-filled with a sentinel, and the four counters of
cstone_hip_find_neighbors_stats with the restated walk of a wave.

Every shape asserts the premise that makes it exercise its branch (the periodic surplus, the leaf beyond 128, the
restated depth >= 140, the single node), so a shape that silently stops doing so fails."""
import ctypes as C

import numpy as np
import pytest

import neighbors_support as ns
from helpers import Box, real_dtype
from neighbors_support import SENT

RBS = [32, 64]


def full_lists(case, impl, first, last, ext=1.0):
    """every neighbour of every target: lists wide enough for the largest count"""
    _, cnt = case.find(impl, first, last, 1, ext)
    return case.find(impl, first, last, max(1, int(cnt.max())), ext)


def stored_mask(counts, ngmax):
    return np.arange(ngmax)[None, :] < np.minimum(counts, ngmax)[:, None]


_totals = {}


def total_neighbours(oracle, bc, bucket, rb):
    key = (bc, bucket, rb)
    if key not in _totals:
        s = ns.spec(oracle, f"aniso-{bc}-b{bucket}", rb)
        _totals[key] = int(s.case.find(oracle, 0, s.case.n, 1)[1].sum())
    return _totals[key]


def check_premise(oracle, name, rb):
    """what makes the shape exercise the code it is here for"""
    s = ns.spec(oracle, name, rb)
    case, kind = s.case, name.split("-")[0]
    if kind == "aniso":
        # the fold matters: the same cloud has at least 10 % more neighbours in the periodic box than in the open one,
        # and the box that is periodic along x only lies strictly between the two
        b = case.bucket
        per, mixed, opn = (total_neighbours(oracle, bc, b, rb) for bc in ("111", "102", "000"))
        assert per >= 1.1 * opn and opn < mixed < per, (per, mixed, opn)
        assert (2 * case.h > 0.5 * 0.7).any()  # 2h beyond half the y length
        f, l = s.ranges[0]
        cnt = case.find(oracle, f, l, 1)[1]
        assert cnt.min() < s.ngmax < cnt.max()  # stored and overflowing lists
    elif kind == "clustered":
        assert case.leaf_counts.max() > 128     # three chunks of 64, the last one ragged
        assert case.leaf_counts.max() % 64 != 0
    elif kind == "clump300":
        assert case.leaf_counts.max() in range(300, 320)  # five chunks: the clump cannot be split
    elif kind == "single":
        assert case.o["num_nodes"] == 1 and case.o["child_offsets"][0] == 0
    elif kind == "deep":
        assert case.n == 14 * ns.DEEP_LEVELS and case.leaf_counts.max() == 2
        if rb == 64:
            assert case.o["num_leaves"] == 10438


# ---- CPU: the shapes are valid and the oracle may serve as the reference there ---------------------------------------

@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", ns.NAMES)
def test_oracle_equals_reference(oracle, reference, name, rb):
    """counts and lists, exactly.  The reference's own walk keeps a stack of 128 entries behind an assert
    (R/traversal/traversal.hpp:81,102), so it cannot run the deepest walk (142): there the same construction is cut at
    the deepest level its stack still holds, and the full chain rests on the brute force and the restated walk."""
    if name == "deep":
        levels = 18
        case = ns.deep_case(oracle, rb, levels)
        depth = ns.wave_stats(case, 0, case.n)[2]
        assert 120 <= depth <= 128, depth
        specs = [(case, (0, case.n), case.n, 1.0)]
    else:
        check_premise(oracle, name, rb)
        s = ns.spec(oracle, name, rb)
        specs = [(s.case, r, s.ngmax, ext) for r in s.ranges for ext in s.exts]
    for case, (f, l), ngmax, ext in specs:
        lo, co = case.find(oracle, f, l, ngmax, ext)
        lr, cr = case.find(reference, f, l, ngmax, ext)
        assert np.array_equal(co, cr) and np.array_equal(lo, lr), (name, f, l, ext)


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", ns.NAMES)
def test_oracle_sets_equal_brute_force(oracle, name, rb):
    check_premise(oracle, name, rb)
    s = ns.spec(oracle, name, rb)
    case = s.case
    nb = case.pair_table()
    for f, l in s.ranges:
        for ext in s.exts:
            lists, cnt = full_lists(case, oracle, f, l, ext)
            got = np.zeros((l - f, case.n), dtype=bool)
            m = stored_mask(cnt, lists.shape[1])
            got[np.nonzero(m)[0], lists[m]] = True
            assert np.array_equal(got.sum(1), cnt)  # no entry twice
            assert np.array_equal(got, nb[f:l]), (name, f, l, ext)


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", ns.NAMES)
def test_oracle_lists_equal_restated_walk(oracle, name, rb):
    check_premise(oracle, name, rb)
    s = ns.spec(oracle, name, rb)
    case = s.case
    for f, l in s.ranges:
        for ext in s.exts:
            lists, cnt = full_lists(case, oracle, f, l, ext)
            walk, depth = ns.walk_lists(case, f, l, ext)
            assert [len(w) for w in walk] == cnt.tolist()
            assert all(w == lists[t, :len(w)].tolist() for t, w in enumerate(walk)), (name, f, l, ext)
            if name == "deep":
                assert depth >= 140 and depth == ns.wave_stats(case, f, l, ext)[2]
                assert (cnt == case.n - 1).all()


@pytest.mark.parametrize("rb", RBS)
def test_ext_widens_the_walk_not_the_lists(oracle, rb):
    for b in (16, 200):
        s = ns.spec(oracle, f"aniso-111-b{b}", rb)
        f, l = s.ranges[0]
        l1, c1 = s.case.find(oracle, f, l, s.ngmax, 1.0)
        l2, c2 = s.case.find(oracle, f, l, s.ngmax, 1.5)
        assert np.array_equal(c1, c2) and np.array_equal(l1, l2)
        assert ns.wave_stats(s.case, f, l, 1.5)[0] > ns.wave_stats(s.case, f, l, 1.0)[0]


# ---- the edges of the radius -----------------------------------------------------------------------------------------

def edge_case(oracle, rb, kind, bucket, bump):
    """exact binary fractions in a unit box.  direct: x_i = 0.25, x_j = 0.5, h = 0.125, so d^2 = 4 h^2 exactly;
    fold: periodic, x_i = 0.0625, x_j = 0.9375, h = 0.0625, the same through the fold.  bump: h one ulp larger.
    coincident: five coincident particles with h = 0 and seven with h > 0.  Two more particles lie far from the pair"""
    T = real_dtype(rb)
    if kind == "coincident":
        pts = [(0.375, 0.375, 0.375)] * 5 + [(0.625, 0.125, 0.875)] * 7
        h = np.array([0.0] * 5 + [0.015625] * 7, dtype=T)
        box = Box([0, 1], (1, 1, 1))
    else:
        xi, xj, hh = (0.25, 0.5, 0.125) if kind == "direct" else (0.0625, 0.9375, 0.0625)
        pts = [(xi, 0.5, 0.5), (xj, 0.5, 0.5), (0.5, 0.125, 0.875), (0.5, 0.875, 0.125)]
        h = np.array([hh, hh, 0.015625, 0.015625], dtype=T)
        if bump:
            h[:2] = np.nextafter(h[:2], T(1))
        box = Box([0, 1], (0, 0, 0) if kind == "direct" else (1, 1, 1))
    pts = np.array(pts)
    x, y, z = [np.ascontiguousarray(pts[:, d]).astype(T) for d in range(3)]
    return ns.Case(oracle, x, y, z, h, box, bucket)


def edge_expected(case, kind, bump):
    """the counts the construction demands, in SFC order"""
    if kind == "coincident":
        return np.where(case.h == 0, 0, 6)
    pair = (case.y == 0.5) & (case.z == 0.5)
    return np.where(pair, 1 if bump else 0, 0)


EDGES = [(k, b, u) for k in ("direct", "fold") for b in (1, 64) for u in (False, True)] + \
        [("coincident", b, False) for b in (1, 64)]


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("kind,bucket,bump", EDGES)
def test_radius_edges_on_the_cpu(oracle, reference, rb, kind, bucket, bump):
    """the strict < at distance exactly 2h, directly and through the fold; h = 0; coincident particles"""
    case = edge_case(oracle, rb, kind, bucket, bump)
    assert (case.o["num_nodes"] == 1) == (bucket == 64)
    want = edge_expected(case, kind, bump)
    lo, co = case.find(oracle, 0, case.n, 8)
    lr, cr = case.find(reference, 0, case.n, 8)
    assert np.array_equal(co, want) and np.array_equal(cr, want)
    assert np.array_equal(lo, lr)
    assert np.array_equal(case.pair_table().sum(1), want)
    walk, _ = ns.walk_lists(case, 0, case.n)
    assert all(w == lo[t, :len(w)].tolist() and len(w) == want[t] for t, w in enumerate(walk))


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


class DevCase:
    def __init__(self, hip, case):
        import cstone_amd

        self.hip, self.case = hip, case
        self.x, self.y, self.z, self.h = (_dev(a) for a in (case.x, case.y, case.z, case.h))
        self.co, self.i2l = _dev(case.o["child_offsets"]), _dev(case.o["internal_to_leaf"])
        self.layout, self.cen, self.siz = _dev(case.layout), _dev(case.cen), _dev(case.siz)
        self.cbox = cstone_amd.make_cbox(case.box.lim, case.box.bc)

    def run(self, entry, first, last, ngmax, ext=1.0, groups=None, null_list=False, rows=None):
        """one call of cstone_hip_find_neighbors[_<entry>] on lists and counts pre-filled with the sentinel:
        (lists [rows, ngmax] row-major whatever the entry's layout, counts [rows], the four counters or None)"""
        import torch

        hip, P = self.hip, lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        nt = last - first if rows is None else rows
        blocks = (nt + 63) // 64
        size = blocks * 64 * ngmax if entry == "interleaved" else nt * ngmax
        lst = torch.full((max(size, 1),), -1, dtype=torch.int32, device="cuda")
        cnt = torch.full((max(nt, 1),), -1, dtype=torch.int32, device="cuda")
        head = [hip.h, C.c_int(self.case.rb), P(self.x), P(self.y), P(self.z), P(self.h), C.c_uint32(first),
                C.c_uint32(last)]
        tail = [C.byref(self.cbox), P(self.co), P(self.i2l), P(self.layout), P(self.cen), P(self.siz), C.c_float(ext),
                C.c_uint32(ngmax), None if null_list else P(lst), P(cnt)]
        stats, keep = None, None
        if entry == "groups":
            keep = (_dev(groups[0]), _dev(groups[1]))
            head += [P(keep[0]), P(keep[1]), C.c_uint32(groups[0].size)]
        if entry == "stats":
            stats = (C.c_uint64 * 4)()
            tail.append(stats)
        fn = getattr(hip.lib, "cstone_hip_find_neighbors" + ("" if entry == "plain" else "_" + entry))
        hip._chk(fn(*head, *tail), "find_neighbors " + entry)
        hip.sync()  # raises if the sticky device-side error word is set (a traversal stack overflow sets it)
        lst = lst.cpu().numpy().view(np.uint32)[:size]
        if entry == "interleaved":
            lst = lst.reshape(blocks, ngmax, 64).transpose(0, 2, 1).reshape(blocks * 64, ngmax)
            assert (lst[nt:] == SENT).all()  # the lanes behind the last target of the last block
            lst = lst[:nt]
        else:
            lst = lst.reshape(nt, ngmax)
        return lst, cnt.cpu().numpy().view(np.uint32)[:nt], (None if stats is None else [int(v) for v in stats])


def assert_same(got, ref_lists, ref_counts, ngmax, covered=None, what=""):
    """counts exactly; entries k < min(count, ngmax) exactly and in order; every other entry still the sentinel;
    targets outside `covered` untouched altogether"""
    lists, counts, _ = got
    covered = np.ones(counts.size, dtype=bool) if covered is None else covered
    assert np.array_equal(counts[covered], ref_counts[covered]), what
    assert (counts[~covered] == SENT).all(), what
    m = stored_mask(ref_counts, ngmax) & covered[:, None]
    bad = np.flatnonzero(((lists != ref_lists) & m).any(1))
    assert bad.size == 0, (what, "rows", bad[:8].tolist(), lists[bad[:3]].tolist(), ref_lists[bad[:3]].tolist())
    bad = np.flatnonzero(((lists != SENT) & ~m).any(1))
    assert bad.size == 0, (what, "written beyond the count, rows", bad[:8].tolist(), lists[bad[:3]].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", ns.NAMES)
def test_hip_equals_oracle_and_restated_counters(hip, oracle, name, rb):
    """all four entry points against the oracle, entry for entry and sentinel for sentinel; the counters of _stats
    against the restated walk of a wave"""
    check_premise(oracle, name, rb)
    s = ns.spec(oracle, name, rb)
    case, ngmax = s.case, s.ngmax
    d = DevCase(hip, case)
    big = case.n >= 2000
    for f, l in s.ranges:
        sum_p2p = []
        for ext in s.exts:
            ref_l, ref_c = case.find(oracle, f, l, ngmax, ext)
            want = ns.wave_stats(case, f, l, ext)
            assert_same(d.run("plain", f, l, ngmax, ext), ref_l, ref_c, ngmax, what=("plain", f, l, ext))
            assert_same(d.run("interleaved", f, l, ngmax, ext), ref_l, ref_c, ngmax, what=("interleaved", f, l, ext))
            got = d.run("stats", f, l, ngmax, ext)
            assert_same(got, ref_l, ref_c, ngmax, what=("stats", f, l, ext))
            assert got[2] == want, (f, l, ext)
            sum_p2p.append(got[2][0])
            gs, ge, covered = ns.make_groups(f, l, case.n)
            if big:  # every feature of the cut is there
                assert gs[0] < f and ge[-1] > l and (gs == ge).any() and not covered.all()
                assert {1, 63, 64, 65, 130} <= set((ge - gs).tolist())
            assert_same(d.run("groups", f, l, ngmax, ext, groups=(gs, ge)), ref_l, ref_c, ngmax, covered,
                        what=("groups", f, l, ext))
            if name == "deep":
                assert want[2] >= 140 and got[2][2] == want[2]  # and the sync in run() found the error word clear
                assert (ref_c == case.n - 1).all()
        if len(s.exts) > 1:  # the oracle's lists do not depend on ext (test_ext_widens_the_walk_not_the_lists)
            assert sum_p2p[1] > sum_p2p[0]


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
def test_hip_idle_lanes_of_a_partial_wave_stay_idle(hip, oracle, rb):
    """regression: the lanes of a wave without a target are parked on the wave's last target and must never become
    interested in a node.  The mask popped from the stack used to be rebuilt from two signed 32-bit halves, so bit 31 of
    the low half smeared over lanes 32..63: with 33..63 targets in a wave (lane 31 busy, the last target on another
    lane) the idle lanes followed lane 31 and overwrote the head of the last target's list.  63 targets per wave, as
    ranges of the plain entries and as groups"""
    s = ns.spec(oracle, "aniso-111-b16", rb)
    case, ngmax = s.case, s.ngmax
    d = DevCase(hip, case)
    for f in range(5, case.n - 63, 211):
        ref_l, ref_c = case.find(oracle, f, f + 63, ngmax)
        for entry in ("plain", "interleaved", "stats"):
            assert_same(d.run(entry, f, f + 63, ngmax), ref_l, ref_c, ngmax, what=(entry, f))
    f, l = s.ranges[0]
    ref_l, ref_c = case.find(oracle, f, l, ngmax)
    for size in (33, 47, 63):
        gs = np.arange(f, l, size, dtype=np.uint32)
        ge = np.minimum(gs + size, l).astype(np.uint32)
        assert_same(d.run("groups", f, l, ngmax, groups=(gs, ge)), ref_l, ref_c, ngmax, what=("groups", size))


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
def test_hip_ext_does_not_change_the_lists(hip, oracle, rb):
    for b in (16, 200):
        s = ns.spec(oracle, f"aniso-111-b{b}", rb)
        d = DevCase(hip, s.case)
        f, l = s.ranges[0]
        a, b15 = d.run("plain", f, l, s.ngmax, 1.0), d.run("plain", f, l, s.ngmax, 1.5)
        assert np.array_equal(a[0], b15[0]) and np.array_equal(a[1], b15[1])


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("kind,bucket,bump", EDGES)
def test_hip_radius_edges(hip, oracle, rb, kind, bucket, bump):
    case = edge_case(oracle, rb, kind, bucket, bump)
    want = edge_expected(case, kind, bump)
    ref_l, ref_c = case.find(oracle, 0, case.n, 8)
    assert np.array_equal(ref_c, want)
    d = DevCase(hip, case)
    gs, ge = np.array([0], dtype=np.uint32), np.array([case.n], dtype=np.uint32)
    for entry in ("plain", "interleaved", "stats", "groups"):
        assert_same(d.run(entry, 0, case.n, 8, groups=(gs, ge)), ref_l, ref_c, 8, what=entry)


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", ["aniso-111-b16", "clump300", "single-n65-pbc"])
def test_hip_ngmax_zero_one_and_empty_range(hip, oracle, name, rb):
    """ngmax = 0 with a null list gives the counts; ngmax = 1 stores the first neighbour of the oracle's order;
    first == last returns 0 and leaves counts and lists as they were"""
    s = ns.spec(oracle, name, rb)
    case = s.case
    d = DevCase(hip, case)
    f, l = s.ranges[0]
    ref_l, ref_c = case.find(oracle, f, l, 1)
    assert (ref_c > 1).any()
    gs, ge, covered = ns.make_groups(f, l, case.n)
    for entry in ("plain", "interleaved", "stats", "groups"):
        cov = covered if entry == "groups" else None
        lists, counts, _ = d.run(entry, f, l, 0, groups=(gs, ge), null_list=True)
        assert_same((lists, counts, None), ref_l[:, :0], ref_c, 0, cov, what=(entry, "ngmax 0"))
        assert_same(d.run(entry, f, l, 1, groups=(gs, ge)), ref_l, ref_c, 1, cov, what=(entry, "ngmax 1"))
        mid = (f + l) // 2
        lists, counts, _ = d.run(entry, mid, mid, 4, groups=(gs, ge), rows=70)
        assert (lists == SENT).all() and (counts == SENT).all(), (entry, "empty range")
