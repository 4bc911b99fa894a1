"""Halo discovery (csrc/halos.hip) on the boxes, trees, radii and range lengths the other suites never show it: the wave
walk findHalosKernel in its four modes (find_halos, halo_boxes, halo_boxes_foreign, find_overlaps) and haloRadiiKernel.

Once a radius has become a cell count everything here is integer geometry, so every comparison is exact, against a brute
force over all (target, leaf) pairs that shares no code with the walk (tests/halos_support.py).  The CPU tests establish
that the oracle agrees with that brute force and with the reference's own CPU code on every shape; the GPU tests compare
the five entry points with both.

Shapes: the anisotropic box under six boundary mixes with radii of 0, a fraction of a cell, a box that ends exactly on a
face, 0.4 of the y length, 1 x and 4 x the longest length (clamped at 2^L - 1: the box sticks out on both sides); the
tree that is one leaf; the root's eight children; a tree refined along one key path to the deepest level; a uniform
tree whose front outgrows 128 stack entries.  Ranges of 1, 63, 64, 65, 255, 256 and 257 leaves at the start, in the
middle and at the end of the tree.  Every shape asserts the premise that makes it reach its branch.

The reference's own walk keeps a stack of 128 entries behind an assert (R/traversal/traversal.hpp:81,102).  No shape here
has to be cut for it: the one-thread walk holds at most 1 + 7 entries per level, the restated walk (dfs_peak) gives the
height for the deepest tree, and both are asserted before the reference is called.  The uniform tree has five levels,
not four: the wave's front on four levels peaks at 56 + 64 = 120 entries, on five at 176.

The reference has halo discovery for the Hilbert curve only (its findHalos goes through sfcIBox / sfcKey, which are
Hilbert by definition), and nothing of it is restated here to make a Morton one: on Hilbert trees the oracle is
compared with the reference's own code and with the brute force, on Morton trees the brute force alone is the arbiter."""
import ctypes as C

import numpy as np
import pytest

import halos_support as hs
from helpers import Box, max_level, real_dtype
from oracle.oracle import HILBERT, MORTON

KBS, RBS, CURVES = [32, 64], [32, 64], [MORTON, HILBERT]
SMALL = ["single", "eight", "deep-corner", "deep-mixed", "wide"]
E_ARG = -1  # CSTONE_E_ARG


# ---- problems: (what, Halo, ranges) ----------------------------------------------------------------------------------

def aniso_problems(oracle, bc, kb, rb, curve):
    tree = hs.aniso_tree(oracle, kb, curve)
    assert 1000 <= tree.nl <= 1500, tree.nl
    box = Box(hs.ANISO, hs.BCS[bc])
    out = []
    for kind in ("mix", "small"):
        radii, cls = hs.aniso_radii(tree, box, kind)
        out.append((kind, hs.Halo(tree, radii, box, rb), hs.ranges_of(tree.nl)))
    return out


def check_aniso_premises(oracle, bc, kb, rb, curve):
    tree = hs.aniso_tree(oracle, kb, curve)
    box = Box(hs.ANISO, hs.BCS[bc])
    radii, cls = hs.aniso_radii(tree, box, "mix")
    assert set(cls.tolist()) == set(range(len(hs.RADIUS_CLASSES)))
    raw = hs.raw_delta(radii, box, rb, tree.L)
    assert (raw >= tree.R).any() and (raw[cls == 4] >= tree.R - 1).all()  # the clamp fired
    assert ((raw[cls == 1] == 1).all() and (raw[cls == 0] == 0).all())    # a fraction of a cell is one cell
    lo, hi = hs.dilated_boxes(tree, radii, box, rb)
    per = np.array(hs.BCS[bc]) == 1
    if per.any():
        assert ((lo[:, per] < 0) & (hi[:, per] > tree.R)).any()           # out on both sides of a periodic axis
        face = cls == 2                                                   # ... and ending exactly on a face, unclamped
        assert (lo[face][:, per] == 0).any() and (hi[face][:, per] == tree.R).any()
    assert (lo[:, ~per] >= 0).all() and (hi[:, ~per] <= tree.R).all()
    delta = np.minimum(raw, tree.R - 1)  # a and b before the clamp of the open axes: the face class alone ends on a face
    a, b = tree.corner - delta, tree.corner + tree.edge[:, None] + delta
    assert (a[cls == 2] == 0).any(0).all() and (b[cls == 2] == tree.R).any(0).all()
    y04 = raw[cls == 3, 1]
    assert (2 * y04 > tree.R // 2).all() and (y04 < tree.R // 2).all()   # beyond half the periodic length, not all of it


def small_problems(oracle, name, kb, rb, curve):
    L = max_level(kb)
    out = []
    if name in ("single", "eight"):
        tree = (hs.single_tree if name == "single" else hs.eight_tree)(oracle, kb, curve)
        assert tree.nl == (1 if name == "single" else 8)
        assert (tree.child[0] == 0) == (name == "single")
        for bc in ("111", "000", "012"):
            box = Box(hs.ANISO, hs.BCS[bc])
            cell = 0.7 / tree.R
            for vals in ([0.0], [0.3 * cell], [0.28], [48.0], [0.0, 0.3 * cell, 0.28, 12.0, 0.1, 48.0, 0.0, 1.0]):
                radii = np.resize(np.array(vals, dtype=np.float32), tree.nl)
                out.append(((bc, vals[0], len(vals)), hs.Halo(tree, radii, box, rb), hs.ranges_of(tree.nl)))
    elif name.startswith("deep"):
        tree = hs.deep_tree(oracle, kb, curve, name.split("-")[1])
        assert tree.nl == 7 * L + 1
        fine = np.flatnonzero(tree.edge == 1)
        assert fine.size == 8 and (np.diff(fine) == 1).all()              # the targets are leaves of edge 1
        i0 = int(fine[0])
        ranges = [(i0, i0 + 8), (i0, i0 + 1), (i0 + 7, i0 + 8), (i0 + 2, i0 + 5)] + hs.ranges_of(tree.nl)
        for bc in ("111", "000"):
            for r in (0.0, 2.0 ** -L):
                halo = hs.Halo(tree, np.full(tree.nl, r, dtype=np.float32), Box([0, 1], hs.BCS[bc]), rb)
                delta = hs.raw_delta(halo.radii, halo.box, rb, L)
                assert (delta == (0 if r == 0 else 1)).all()               # 0 and exactly one finest cell
                out.append(((bc, r), halo, ranges))
    elif name == "wide":
        tree = hs.wide_tree(oracle, kb, curve)
        assert tree.nl == 8 ** hs.WIDE_LEVEL
        box = Box([0, 1], (1, 1, 1))
        for t in (0, tree.nl // 2 + 5):
            radii = np.zeros(tree.nl, dtype=np.float32)
            radii[t] = 1.0  # the whole box length
            halo = hs.Halo(tree, radii, box, rb, targets=(t, t + 1))
            assert (hs.raw_delta(radii[t:t + 1], box, rb, L) >= tree.R).all()        # the clamp fired
            assert (halo.lo[t] < 0).all() and (halo.hi[t] > tree.R).all()            # out on both sides
            peak = hs.wave_peak(tree, hs.node_interest(tree, halo.lo[t], halo.hi[t], t, t + 1, False))
            assert 128 < peak < 1024, peak
            out.append((t, halo, [(t, t + 1)]))
    return out


def dfs_fits_reference(halo, ranges):
    """the reference's 128-entry stack holds every walk of these ranges"""
    tree = halo.tree
    if 1 + 7 * int(tree.level.max()) < 128:
        return True
    for f, l in ranges:
        for t in range(f, l):
            go = hs.node_interest(tree, halo.lo[t], halo.hi[t], f, l, False)
            if hs.dfs_peak(tree, go) >= 128:
                return False
    return True


def check_cpu(oracle, problems):
    """the oracle against the brute force"""
    for what, halo, ranges in problems:
        tree = halo.tree
        for f, l in ranges:
            want = halo.brute_find_halos(f, l)
            got = oracle.find_halos(tree.curve, tree.o, tree.leaves, halo.radii, halo.box, f, l, halo.rb)
            assert got is not None and np.array_equal(got, want), (what, f, l)
            plain, _ = halo.brute_boxes(f, l)
            got = oracle.halo_boxes(tree.curve, tree.leaves, halo.radii, halo.box, f, l, halo.rb)
            assert np.array_equal(got, plain), (what, f, l, "boxes")


def check_reference(oracle, reference, problems):
    """the oracle against the reference's own code, which has halo discovery for the Hilbert curve only.  A missing
    answer (None) is a failure"""
    for what, halo, ranges in problems:
        tree = halo.tree
        assert tree.curve == HILBERT and dfs_fits_reference(halo, ranges)
        for f, l in ranges:
            got = oracle.find_halos(tree.curve, tree.o, tree.leaves, halo.radii, halo.box, f, l, halo.rb)
            ref = reference.find_halos(tree.curve, tree.o, tree.leaves, halo.radii, halo.box, f, l, halo.rb)
            assert got is not None and ref is not None and np.array_equal(got, ref), (what, f, l)


# ---- CPU: the oracle equals the brute force and the reference's own code on every shape ------------------------------

@pytest.mark.parametrize("kb", KBS)
@pytest.mark.parametrize("curve", CURVES)
def test_decoder_round_trips_on_random_keys(oracle, kb, curve):
    L = max_level(kb)
    keys = np.random.default_rng(kb + curve).integers(0, 1 << (3 * L), 5000, dtype=np.uint64)
    for level in (0, 1, L // 2, L - 1, L):
        span = np.uint64(1) << np.uint64(3 * (L - level))
        hs.check_decoder(oracle, keys & ~(span - np.uint64(1)), np.full(keys.size, level), curve, kb)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("kb", KBS)
@pytest.mark.parametrize("bc", list(hs.BCS))
def test_cpu_aniso(oracle, bc, kb, rb, curve):
    check_aniso_premises(oracle, bc, kb, rb, curve)
    check_cpu(oracle, aniso_problems(oracle, bc, kb, rb, curve))


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("kb", KBS)
@pytest.mark.parametrize("bc", list(hs.BCS))
def test_cpu_aniso_equals_reference(oracle, reference, bc, kb, rb):
    check_reference(oracle, reference, aniso_problems(oracle, bc, kb, rb, HILBERT))


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("kb", KBS)
@pytest.mark.parametrize("name", SMALL)
def test_cpu_small_trees(oracle, name, kb, rb, curve):
    check_cpu(oracle, small_problems(oracle, name, kb, rb, curve))


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("kb", KBS)
@pytest.mark.parametrize("name", SMALL)
def test_cpu_small_trees_equal_reference(oracle, reference, name, kb, rb):
    check_reference(oracle, reference, small_problems(oracle, name, kb, rb, HILBERT))


def flagged(halo, ranges):
    return sum(int(halo.brute_find_halos(f, l).sum()) for f, l in ranges)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kb", KBS)
def test_periodic_faces_matter_on_the_aniso_tree(oracle, kb, curve):
    """the same tree, radii and ranges flag at least 10 % more leaves in the periodic box than in the open one; a box
    that is periodic along one axis lies in between"""
    tree = hs.aniso_tree(oracle, kb, curve)
    radii, _ = hs.aniso_radii(tree, Box(hs.ANISO), "small")
    ranges = hs.ranges_of(tree.nl)
    per, mixed, opn = (flagged(hs.Halo(tree, radii, Box(hs.ANISO, hs.BCS[bc]), 64), ranges) for bc in ("111", "010", "000"))
    assert per >= 1.1 * opn and opn < mixed < per, (per, mixed, opn)


def foreign_ranges(nl):
    """ranges of more than a workgroup: their boundary leaves, the ones with foreign boxes, sit at lanes on both sides
    of lane 32 and in the waves 1..3 of a workgroup, whatever the curve does in between"""
    return [(0, nl // 2), (nl // 2 - 100, nl // 2 + 157), (nl // 3, min(nl // 3 + 700, nl - 50)), (nl - 300, nl)]


def check_foreign_premise(pairs):
    """over the ranges of a case together: the proven rule exports something, and less than the enclosing-node rule;
    its boxes sit at lanes on both sides of lane 32 and in the waves 1..3 of a workgroup"""
    s_f = sum(int(foreign[:, 6].sum()) for _, foreign in pairs)
    s_p = sum(int(plain[:, 6].sum()) for plain, _ in pairs)
    assert 0 < s_f < s_p, (s_f, s_p)
    lanes = np.concatenate([np.flatnonzero(foreign[:, 6]) % 256 for _, foreign in pairs])
    assert ((lanes % 64) < 32).any() and ((lanes % 64) > 32).any() and {1, 2, 3} <= set((lanes // 64).tolist())


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kb", KBS)
def test_cpu_foreign_rule_is_stricter_than_the_enclosing_node(oracle, kb, curve):
    tree = hs.aniso_tree(oracle, kb, curve)
    halo = hs.Halo(tree, hs.aniso_radii(tree, Box(hs.ANISO), "small")[0], Box(hs.ANISO, (1, 0, 2)), 64)
    pairs = [halo.brute_boxes(f, l) for f, l in foreign_ranges(tree.nl)]
    assert all((foreign[:, 6] <= plain[:, 6]).all() for plain, foreign in pairs)
    check_foreign_premise(pairs)


# ---- find_overlaps ---------------------------------------------------------------------------------------------------

RANKS = (0, 1, 5, 31, 37)  # 37 must act as 5


def overlap_records(oracle, kb, curve):
    """the boxes the first and the last 150 leaves export in the periodic box (some reach below 0 or beyond R), the exporting rank
    cycling through RANKS, every seventh record switched off"""
    tree = hs.aniso_tree(oracle, kb, curve)
    box = Box(hs.ANISO, (1, 1, 1))
    halo = hs.Halo(tree, hs.aniso_radii(tree, box, "small")[0], box, 64)
    rec = np.concatenate([halo.brute_boxes(0, 150)[0], halo.brute_boxes(tree.nl - 150, tree.nl)[0]])
    assert (rec[:, 0:6:2] < 0).any() and (rec[:, 1:6:2] > tree.R).any()
    rec[:, 6] = 1
    rec[::7, 6] = 0
    rec[:, 7] = np.resize(np.array(RANKS), 300)
    return tree, rec


def overlap_cases(tree, rec):
    nl = tree.nl
    ranges = [(0, nl), (0, 257), (nl - 257, nl), ((nl - 65) // 2, (nl - 65) // 2 + 65), (5, 6), (nl // 3, nl // 3)]
    return [(n, f, l) for n in (1, 255, 256, 257, 300) for f, l in ranges]


def check_overlap_premises(tree, rec):
    full = hs.brute_overlaps(tree, rec, 0, tree.nl)
    assert (full & np.uint32(0x80000000)).any()                                   # bit 31 survives as uint32
    assert any(bin(int(w)).count("1") >= 2 for w in full)                         # two ranks on one leaf
    on = rec.copy()
    on[:, 6] = 1
    assert not np.array_equal(hs.brute_overlaps(tree, on, 0, tree.nl), full)     # a switched-off record overlaps
    only37 = rec[rec[:, 7] == 37]
    w37 = hs.brute_overlaps(tree, only37, 0, tree.nl)
    assert w37.any() and set(w37.tolist()) <= {0, 32}


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kb", KBS)
def test_cpu_find_overlaps(oracle, kb, curve):
    tree, rec = overlap_records(oracle, kb, curve)
    check_overlap_premises(tree, rec)
    for n, f, l in overlap_cases(tree, rec):
        want = hs.brute_overlaps(tree, rec[:n], f, l)
        got = oracle.find_overlaps(curve, tree.leaves, rec[:n], f, l).view(np.uint32)
        assert np.array_equal(got, want), (n, f, l)
        assert np.array_equal(got != 0, want != 0)
    zero = rec.copy()
    zero[:, 7] = 0  # what halo_boxes writes: plain 0/1 flags
    got = oracle.find_overlaps(curve, tree.leaves, zero, 0, tree.nl)
    assert set(got.tolist()) == {0, 1} and np.array_equal(got != 0, hs.brute_overlaps(tree, rec, 0, tree.nl) != 0)
    one = hs.single_tree(oracle, kb, curve)
    want = hs.brute_overlaps(one, rec, 0, 1)
    assert want[0] == sum(1 << r for r in (0, 1, 5, 31))
    assert np.array_equal(oracle.find_overlaps(curve, one.leaves, rec, 0, 1).view(np.uint32), want)


# ---- halo_radii ------------------------------------------------------------------------------------------------------

LEAF_SIZES = (0, 1, 15, 16, 17, 63, 64, 65, 129, 200)
MAX_AT = (0, 5, 15, 16, 20, 32, 40, 48, 60, 63, 64, 70, 100, 128, 150, 199)  # the four slots, the ragged tail, the rounds


def radii_layout(hb, seed=3):
    """(h, layout): one leaf per (size, position of its maximum); the other values lie below every maximum"""
    rng = np.random.default_rng(seed)
    sizes, at = [], []
    for s in LEAF_SIZES:
        for p in sorted({p for p in MAX_AT if p < s} | ({s - 1} if s else set())) or [None]:
            sizes.append(s)
            at.append(p)
    layout = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    h = rng.uniform(0.1, 1.0, int(layout[-1])).astype(real_dtype(hb))
    for k, p in enumerate(at):
        if p is not None:
            h[layout[k] + p] = real_dtype(hb)(rng.uniform(2.0, 3.0))
    assert max(sizes) > 128
    return h, layout


def radii_cases(hb):
    """(h, layout, first, last, nl, ext)"""
    h, layout = radii_layout(hb)
    n = layout.size - 1
    out = [(h, layout, f, f + n, nl, ext) for f, nl in ((0, n), (7, n + 20)) for ext in (0.0, 1.0, 1.5)]
    three = np.array([0, 129, 129, 329], dtype=np.uint32)  # one workgroup strides over about 5000 outside slots
    out += [(h, three, 2481, 2484, 5000, 1.5), (h, three, 0, 3, 5000, 1.0), (h, three, 4997, 5000, 5000, 1.0)]
    out += [(h, layout[:1], 40, 40, 300, 1.0), (h, layout[:1], 0, 0, 1, 1.0)]  # first == last
    return out


@pytest.mark.parametrize("hb", RBS)
def test_cpu_halo_radii(oracle, hb):
    for h, layout, f, l, nl, ext in radii_cases(hb):
        want = hs.model_halo_radii(h, layout, f, l, nl, ext)
        assert np.array_equal(oracle.halo_radii(h, layout, f, l, nl, ext), want), (f, l, nl, ext)
        assert (want[:f] == 0).all() and (want[l:] == 0).all()


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint32, np.uint64):
        a = a.view(np.int32 if a.dtype == np.uint32 else np.int64)
    return torch.from_numpy(a.copy()).cuda()


class DevTree:
    _last = None  # (tree, its device copy): the cases of one tree run back to back, so one entry serves

    def __init__(self, tree):
        self.leaves = _dev(tree.leaves)
        self.o = {k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in tree.o.items()}

    @classmethod
    def of(cls, tree):
        if cls._last is None or cls._last[0] is not tree:
            cls._last = (tree, cls(tree))
        return cls._last[1]


def cbox(box):
    import cstone_amd

    return cstone_amd.make_cbox(box.lim, box.bc)


def check_gpu(hip, oracle, problems, foreign=True):
    for what, halo, ranges in problems:
        tree = halo.tree
        d, radii, cb = DevTree.of(tree), _dev(halo.radii), cbox(halo.box)
        for f, l in ranges:
            want = halo.brute_find_halos(f, l)
            ref = oracle.find_halos(tree.curve, tree.o, tree.leaves, halo.radii, halo.box, f, l, halo.rb)
            got = hip.find_halos(tree.curve, d.o, d.leaves, radii, cb, f, l, halo.rb)  # on pre-zeroed flags
            hip.sync()  # raises if the sticky device-side error word is set (a stack overflow sets it)
            got = got.cpu().numpy()
            assert np.array_equal(got, ref) and np.array_equal(got, want), (what, f, l, "find_halos")
            if l == f:
                continue  # no box to write: the wrapper has no buffer to pass for an empty range
            plain, proven = halo.brute_boxes(f, l)
            got = hip.halo_boxes(tree.curve, d.leaves, radii, cb, f, l, halo.rb).cpu().numpy()
            assert np.array_equal(got, plain), (what, f, l, "halo_boxes")
            if foreign:
                got = hip.halo_boxes_foreign(tree.curve, d.o, d.leaves, radii, cb, f, l, halo.rb)
                hip.sync()
                assert np.array_equal(got.cpu().numpy(), proven), (what, f, l, "halo_boxes_foreign")


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("kb", KBS)
@pytest.mark.parametrize("bc", list(hs.BCS))
def test_hip_aniso(hip, oracle, bc, kb, rb, curve):
    check_aniso_premises(oracle, bc, kb, rb, curve)
    check_gpu(hip, oracle, aniso_problems(oracle, bc, kb, rb, curve))


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("kb", KBS)
@pytest.mark.parametrize("name", SMALL)
def test_hip_small_trees(hip, oracle, name, kb, rb, curve):
    check_gpu(hip, oracle, small_problems(oracle, name, kb, rb, curve))


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("kb", KBS)
def test_hip_halo_boxes_foreign_on_every_box(hip, oracle, kb, rb, curve):
    """columns 0..5 and 7 as halo_boxes writes them, column 6 by the proven rule, for every box of ranges whose foreign
    boxes lie at lanes on both sides of lane 32 and in the waves 1..3 of a workgroup"""
    tree = hs.aniso_tree(oracle, kb, curve)
    box = Box(hs.ANISO, (1, 0, 2))
    halo = hs.Halo(tree, hs.aniso_radii(tree, box, "small")[0], box, rb)
    d, radii, cb = DevTree.of(tree), _dev(halo.radii), cbox(box)
    pairs = [halo.brute_boxes(f, l) for f, l in foreign_ranges(tree.nl)]
    check_foreign_premise(pairs)
    for (f, l), (plain, proven) in zip(foreign_ranges(tree.nl), pairs):
        got_p = hip.halo_boxes(curve, d.leaves, radii, cb, f, l, rb).cpu().numpy()
        got_f = hip.halo_boxes_foreign(curve, d.o, d.leaves, radii, cb, f, l, rb)
        hip.sync()
        got_f = got_f.cpu().numpy()
        cols = [0, 1, 2, 3, 4, 5, 7]
        assert np.array_equal(got_p, plain) and np.array_equal(got_f[:, cols], got_p[:, cols]), (f, l)
        assert np.array_equal(got_f[:, 6], proven[:, 6]), (f, l)


@pytest.mark.gpu
@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kb", KBS)
def test_hip_find_overlaps(hip, oracle, kb, curve):
    tree, rec = overlap_records(oracle, kb, curve)
    check_overlap_premises(tree, rec)
    d = DevTree.of(tree)
    for n, f, l in overlap_cases(tree, rec):
        want = hs.brute_overlaps(tree, rec[:n], f, l)
        got = hip.find_overlaps(curve, d.o, d.leaves, _dev(rec[:n]), f, l)
        hip.sync()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want), (n, f, l)
    one = hs.single_tree(oracle, kb, curve)
    d1 = DevTree.of(one)
    for n in (1, 2, 257, 300):  # the root is a leaf: the walk ends at its first test
        got = hip.find_overlaps(curve, d1.o, d1.leaves, _dev(rec[:n]), 0, 1)
        hip.sync()
        assert np.array_equal(got.cpu().numpy().view(np.uint32), hs.brute_overlaps(one, rec[:n], 0, 1)), n
    wide = hs.wide_tree(oracle, kb, curve)  # a record as wide as the periodic box: the front outgrows 128 entries
    R = wide.R
    big = np.array([[1 - R, 2 * R - 1] * 3 + [1, 31]], dtype=np.int32)
    go = hs.node_interest(wide, big[0, 0:6:2].astype(np.int64), big[0, 1:6:2].astype(np.int64), 0, wide.nl, True)
    assert 128 < hs.wave_peak(wide, go) < 1024
    dw = DevTree.of(wide)
    got = hip.find_overlaps(curve, dw.o, dw.leaves, _dev(big), 100, wide.nl - 77)
    hip.sync()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), hs.brute_overlaps(wide, big, 100, wide.nl - 77))


@pytest.mark.gpu
@pytest.mark.parametrize("hb", RBS)
def test_hip_halo_radii(hip, hb):
    """the ABI itself on an output pre-filled with NaN: the model bit for bit, and no NaN left anywhere in [0, nl)"""
    import torch

    for h, layout, f, l, nl, ext in radii_cases(hb):
        want = hs.model_halo_radii(h, layout, f, l, nl, ext)
        out = torch.full((nl + 8,), float("nan"), dtype=torch.float32, device="cuda")
        hd, ld = _dev(h), _dev(layout)
        rc = hip.lib.cstone_hip_halo_radii(hip.h, C.c_int(hb), C.c_void_p(hd.data_ptr()), C.c_void_p(ld.data_ptr()),
                                           C.c_int(f), C.c_int(l), C.c_int(nl), C.c_float(ext),
                                           C.c_void_p(out.data_ptr()))
        assert rc == 0
        hip.sync()
        got = out.cpu().numpy()
        assert not np.isnan(got[:nl]).any(), (f, l, nl, ext, np.flatnonzero(np.isnan(got[:nl]))[:8])
        assert np.array_equal(got[:nl].view(np.uint32), want.view(np.uint32)), (f, l, nl, ext)
        assert np.isnan(got[nl:]).all()  # and nothing behind the array


@pytest.mark.gpu
def test_hip_bad_arguments_launch_nothing(hip, oracle):
    """null pointers, last < first, a curve that is neither, unsupported bit widths: CSTONE_E_ARG from all five entries,
    and the outputs keep their sentinel"""
    import torch

    tree = hs.eight_tree(oracle, 64, HILBERT)
    d = DevTree.of(tree)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    radii = _dev(np.full(8, 0.1, dtype=np.float32))
    flags = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    boxes = torch.full((8, 8), -7, dtype=torch.int32, device="cuda")
    rout = torch.full((8,), -7.0, dtype=torch.float32, device="cuda")
    h, lay = _dev(np.ones(8)), _dev(np.arange(9, dtype=np.uint32))
    cb = cbox(Box([0, 1]))
    lib, ctx, null = hip.lib, hip.h, C.c_void_p(0)
    tri = [P(d.o["prefixes"]), P(d.o["child_offsets"]), P(d.o["internal_to_leaf"])]
    I = C.c_int  # noqa: E741

    def find(curve=1, kb=64, rb=64, ptrs=None, f=0, l=8, box=C.byref(cb), out=P(flags), r=P(radii)):
        return lib.cstone_hip_find_halos(ctx, I(curve), I(kb), I(rb), *(ptrs or tri), P(d.leaves), r, box, I(f), I(l), out)

    def foreign(curve=1, kb=64, rb=64, ptrs=None, f=0, l=8, box=C.byref(cb), out=P(boxes), r=P(radii)):
        return lib.cstone_hip_halo_boxes_foreign(ctx, I(curve), I(kb), I(rb), *(ptrs or tri), P(d.leaves), r, box, I(f),
                                                 I(l), out)

    def plain(curve=1, kb=64, rb=64, leaves=P(d.leaves), f=0, l=8, box=C.byref(cb), out=P(boxes), r=P(radii)):
        return lib.cstone_hip_halo_boxes(ctx, I(curve), I(kb), I(rb), leaves, r, box, I(f), I(l), out)

    def serve(curve=1, kb=64, ptrs=None, recs=P(boxes), n=8, f=0, l=8, out=P(flags)):
        return lib.cstone_hip_find_overlaps(ctx, I(curve), I(kb), *(ptrs or tri), P(d.leaves), recs, I(n), I(f), I(l), out)

    def rad(hb=64, hp=P(h), lp=P(lay), f=0, l=8, nl=8, out=P(rout)):
        return lib.cstone_hip_halo_radii(ctx, I(hb), hp, lp, I(f), I(l), I(nl), C.c_float(1.0), out)

    bad = []
    for fn in (find, foreign):
        bad += [fn(ptrs=tri[:k] + [null] + tri[k + 1:]) for k in range(3)]
        bad += [fn(out=null), fn(r=null), fn(box=null), fn(f=5, l=3), fn(f=-1), fn(curve=2), fn(curve=-1), fn(kb=16),
                fn(rb=16), fn(kb=48, rb=64)]
    bad += [plain(leaves=null), plain(out=null), plain(r=null), plain(box=null), plain(f=5, l=3), plain(f=-1),
            plain(curve=2), plain(kb=16), plain(rb=80)]
    bad += [serve(ptrs=tri[:k] + [null] + tri[k + 1:]) for k in range(3)]
    bad += [serve(out=null), serve(recs=null), serve(n=-1), serve(f=5, l=3), serve(f=-1), serve(curve=7), serve(kb=16)]
    bad += [rad(out=null), rad(hp=null), rad(lp=null), rad(f=5, l=3), rad(f=-1), rad(l=9), rad(hb=16)]
    assert bad and all(rc == E_ARG for rc in bad), bad
    hip.sync()
    assert (flags == -7).all() and (boxes == -7).all() and (rout == -7.0).all()
    assert find() == 0 and rad() == 0  # the context still serves
    hip.sync()
