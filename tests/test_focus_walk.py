"""The focus-tree kernels of csrc/focus.hip on the trees, boxes, focus ranges and sizes the other suites never show them:
the MAC walk markMacsKernel against a brute force over all (target, node) pairs, and the per-node and per-leaf kernels
(essential / MAC-refine decisions, protect_ancestors, enforce_keys, range_count, the SFC gaps, add_macs, the MAC spheres
and the source centres) against plain models written from the contracts in include/cstone_hip.h.  The models are in
tests/focus_support.py and share no code with the kernels or with the oracle.  Every comparison is `==`.

Every test body runs on two backends (tests/let_ops_support.py): `cpu` puts the oracle in the kernel's place behind the
same C ABI and, where the reference has the function (mark_macs and the spheres: Hilbert keys only), adds the
reference's own code: model == oracle == reference.  `hip` (@gpu) lets the model judge the kernel.  Each case asserts,
from the model, the premise that makes it reach its branch.

The stack of the walk.  A step pops up to 8 entries and pushes up to 64 internal children, so after the step that
pushes level k the stack holds at most 64 + 56 (k - 2) entries, and only internal nodes are pushed: k <= 9 for 32-bit
keys (456 entries), k <= 20 for 64-bit keys.  Up to k = 19 that is 1016 <= 1024.  Only a 64-bit tree in which 64 open
internal nodes sit below 8 siblings on EVERY level from 2 to 20 -- a chain of fully refined groups nested twenty deep,
all of them failing the MAC against one target -- gets to 1072; the kernel then sets code 4 in the error word and
stops that walk, it does not write past the stack.  No case here goes near it (the widest front, on the uniform tree
of five levels, is 176), and none may try: a case must not provoke a device error.

Two rules of the walk cannot be told from their neighbours by any output, and no case pretends to:
* the out-of-grid branch of containedIn answering "not contained" always: it answers "contained" only for a focus that is
  the whole key range, and then every node lies inside the focus and nothing is marked whether the target is walked
  or not (answering "contained" always is told apart: test_mark_macs_corner_focus);
* the floor of maxSourceLevel at 0: only a level-0 target reaches it, that target is the whole key range, and it is
  skipped before the level is used (test_mark_macs_small_trees asserts that it is skipped)."""
import ctypes as C

import numpy as np
import pytest

import focus_support as fs
import halos_support as hs
import let_ops_support as S
from helpers import Box, end_key, key_dtype, max_level, random_cloud, real_dtype
from oracle.oracle import HILBERT, MORTON

gpu = pytest.mark.gpu
KBS, RBS, CURVES = [32, 64], [32, 64], [MORTON, HILBERT]
KB = pytest.mark.parametrize("kb", KBS)
UNIT = [0, 1]
NEG = [-3.0, -1.0, -0.5, 0.25, -2.0, 6.0]  # a box with negative limits


@pytest.fixture(params=["cpu", pytest.param("hip", marks=gpu)])
def be(request):
    if request.param == "cpu":
        return S.cpu_backend()
    return S.HipBackend(request.getfixturevalue("hip"))


class Hold:
    """uploads an array, keeps the allocation alive until the test ends, returns the device pointer: an allocation made
    inside an argument list would be freed, and reused by the next upload, before the call reads it"""

    def __init__(self, be):
        self.be, self.bufs = be, []

    def __call__(self, a):
        self.bufs.append(self.be.to_dev(a))
        return self.be.ptr(self.bufs[-1])


def reference_of(request, be):
    """the reference's own code, on the cpu leg only"""
    return request.getfixturevalue("reference") if be.name == "cpu" else None


# ----------------------------------------------------------------------------------------------------------------------
# 1. mark_macs
# ----------------------------------------------------------------------------------------------------------------------

def preset(tree, seed):
    """a tenth of the nodes 1, a twentieth 2"""
    u = np.random.default_rng(seed).random(tree.child.size)
    return np.where(u < 0.1, 1, np.where(u < 0.15, 2, 0)).astype(np.int8)


def centres_of(kind, tree, box, rb):
    T = real_dtype(rb)
    if kind in ("geo0.5", "geo0.8"):
        return fs.geo_spheres_model(tree, box, rb, 1.0 / float(kind[3:]) + 0.5)
    c = fs.geo_spheres_model(tree, box, rb, 2.5)
    if kind == "zero":
        c[:, 3] = 0
    elif kind == "negative":
        c[:, 3] = -c[:, 3]
    else:
        assert kind == "huge"
        c[:, 3] = T(fs.HUGE)
    return c


def check_mark_macs(be, oracle, reference, tree, centers, box, rb, focus_nodes, limit, initial, what):
    """model == backend (== oracle == reference on the cpu leg); returns the model"""
    focus_nodes = np.ascontiguousarray(focus_nodes, dtype=key_dtype(tree.kb))
    model = fs.MacModel(tree, centers, box, rb, focus_nodes, limit, initial)
    got = fs.call_mark_macs(be, tree, centers, box, rb, focus_nodes, limit, model.initial)
    assert np.array_equal(got, model.marks), (what, int(got.sum()), int(model.marks.sum()))
    assert np.array_equal(got[model.initial != 0], model.initial[model.initial != 0])  # markings are not cleared
    if be.name == "cpu":
        direct = oracle.mark_macs(tree.curve, tree.o, centers, box, focus_nodes, limit, model.initial)
        assert np.array_equal(direct, model.marks), what
        if tree.curve == HILBERT:
            ref = reference.mark_macs(tree.curve, tree.o, centers, box, focus_nodes, limit, model.initial)
            assert ref is not None and np.array_equal(ref, model.marks), what
    return model


CENTRE_KINDS = ("geo0.5", "geo0.8", "zero", "negative", "huge")


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("curve", CURVES)
@KB
def test_mark_macs_aniso(be, oracle, request, kb, curve, rb):
    """about 1300 leaves; focus ranges of 1, 63, 64, 65, 255, 256 and 257 leaves at the start, in the middle and at the
    end, the whole tree and the empty range; the six boundary mixes; both boxes; the five kinds of centres; limit_source
    0 and 1; markings zero and preset"""
    reference = reference_of(request, be)
    tree = hs.aniso_tree(oracle, kb, curve)
    assert 1000 <= tree.nl <= 1500
    ranges = hs.ranges_of(tree.nl)
    assert {l - f for f, l in ranges} >= set(hs.LENGTHS) | {0, tree.nl}
    seen = {"marked": 0, "walked": 0, "skipped": 0, "kinds": set(), "fold2": 0, "nofold": 0, "nofabs": 0, "lt": 0}
    for i, (f, l) in enumerate(ranges):
        for j in range(2):
            k = 2 * i + j
            bc = list(hs.BCS)[k % 6]
            box = Box(hs.ANISO if (k // 6) % 2 == 0 else UNIT, hs.BCS[bc])
            kind = CENTRE_KINDS[k % 5]
            limit = (k // 2) % 2
            centers = centres_of(kind, tree, box, rb)
            initial = preset(tree, k) if k % 3 else np.zeros(tree.child.size, np.int8)
            focus = tree.leaves[f:l + 1]
            what = (f, l, bc, kind, limit)
            m = check_mark_macs(be, oracle, reference, tree, centers, box, rb, focus, limit, initial, what)
            new = int(((m.initial == 0) & (m.marks == 1)).sum())
            if l == f:
                assert new == 0                                   # num_focus_nodes = 0: OK and nothing written
                continue
            if l - f == tree.nl:
                assert m.skipped.all() and new == 0               # the whole tree: every target skipped
                assert (m.branch == fs.OUT_OF_GRID).any() and (m.branch == fs.ENVELOPE_INSIDE).any()
                continue
            assert m.walked.size > 0
            if kind == "zero":
                assert new == 0
            elif kind == "huge":                                  # every node outside the focus that is shallow enough
                deepest = int(m.level[m.walked].max()) - 1 if limit else tree.L
                assert np.array_equal(m.marks != 0, (m.initial != 0) | (~m.in_focus & (tree.node_level <= deepest)))
            else:
                assert new > 0
            seen["marked"] += new
            seen["walked"] += m.walked.size
            seen["skipped"] += int(m.skipped.sum())
            seen["kinds"].add(kind)
            for variant, key in (("fold2", "fold2"), ("nofold", "nofold"), ("nofabs", "nofabs"), ("lt_level", "lt")):
                if (variant == "fold2" and 2 not in hs.BCS[bc]) or (variant == "nofold" and 1 not in hs.BCS[bc]) or \
                        (variant == "nofabs" and kind != "negative") or (variant == "lt_level" and not limit):
                    continue
                other = fs.MacModel(tree, centers, box, rb, focus, limit, initial, variant=variant)
                differs = not np.array_equal(other.marks, m.marks)
                if variant == "nofold":  # ... with a radius beyond half the length of a periodic axis
                    length = (box.lim[1::2] - box.lim[0::2])[np.array(hs.BCS[bc]) == 1]
                    differs = differs and bool((np.sqrt(np.abs(centers[:, 3].astype(np.float64))) > 0.5 * length.min()).any())
                seen[key] += int(differs)
    # the premises: targets skipped and walked, every kind of centre, and cases that tell the rule from its neighbours:
    # a fixed (type 2) axis that must not fold, a periodic axis on which the fold decides (the radius reaches past half
    # the box length), the sign of the fourth entry, and the deepest source level that limit_source admits
    assert seen["marked"] > 0 and seen["walked"] > 0 and seen["skipped"] > 0 and seen["kinds"] == set(CENTRE_KINDS)
    assert seen["fold2"] > 0 and seen["nofold"] > 0 and seen["nofabs"] > 0 and seen["lt"] > 0, seen


SMALL = ["single", "eight", "deep-corner", "deep-mixed"]


def small_tree(oracle, name, kb, curve):
    if name == "single":
        return hs.single_tree(oracle, kb, curve)
    if name == "eight":
        return hs.eight_tree(oracle, kb, curve)
    return hs.deep_tree(oracle, kb, curve, name.split("-")[1])


@pytest.mark.parametrize("curve", CURVES)
@KB
@pytest.mark.parametrize("name", SMALL)
def test_mark_macs_small_trees(be, oracle, request, name, kb, curve):
    """the root-only tree (childOffsets[0] == 0; its one target has level 0, is the whole key range and is skipped), the
    root's eight children (level-1 targets: maxSourceLevel 0 with limit_source) and the trees refined along one key
    path to the deepest level (targets and sources of edge 1)"""
    reference = reference_of(request, be)
    tree = small_tree(oracle, name, kb, curve)
    L = max_level(kb)
    assert tree.nl == {"single": 1, "eight": 8}.get(name, 7 * L + 1)
    assert (tree.child[0] == 0) == (name == "single")
    if name.startswith("deep"):
        assert (tree.level == L).sum() == 8 and (tree.node_level == L).sum() == 8
        fine = int(np.flatnonzero(tree.level == L)[0])
        ranges = [(fine, fine + 8), (fine + 2, fine + 3), (0, fine), (fine + 8, tree.nl)] + hs.ranges_of(tree.nl)
    else:
        ranges = [(f, l) for f in range(tree.nl) for l in range(f, tree.nl + 1)][:40]
    marked = 0
    for k, (f, l) in enumerate(ranges):
        for rb in RBS:
            for limit in (0, 1):
                bc = list(hs.BCS)[(k + limit) % 6]
                box = Box(hs.ANISO if k % 2 else UNIT, hs.BCS[bc])
                kind = ("geo0.5", "huge", "geo0.8", "negative")[(k + rb // 32) % 4]
                centers = centres_of(kind, tree, box, rb)
                initial = preset(tree, k) if k % 2 else np.zeros(tree.child.size, np.int8)
                m = check_mark_macs(be, oracle, reference, tree, centers, box, rb, tree.leaves[f:l + 1], limit, initial,
                                    (name, f, l, bc, kind, limit, rb))
                new = int(((m.initial == 0) & (m.marks == 1)).sum())
                marked += new
                if l - f == tree.nl:
                    assert m.skipped.all() and new == 0
                    if name == "single":
                        assert m.level.tolist() == [0] and m.branch.tolist() == [fs.OUT_OF_GRID]
                elif l > f and name == "eight":
                    assert (m.level == 1).all() and m.walked.size == l - f  # every child touches the grid's faces
                    if kind == "huge":  # with limit_source: level 0 and nothing deeper, so the root alone
                        want = ~m.in_focus & ((tree.node_level <= 0) if limit else True)
                        assert np.array_equal(m.marks != 0, (m.initial != 0) | want)
                        other = fs.MacModel(tree, centers, box, rb, tree.leaves[f:l + 1], limit, initial, "lt_level")
                        assert not limit or initial[0] != 0 or not np.array_equal(other.marks, m.marks)
    assert marked > 0 or name == "single"


@pytest.mark.parametrize("curve", CURVES)
@KB
def test_mark_macs_wide_front(be, oracle, request, kb, curve):
    """the uniform tree of five levels with every node failing the MAC: the front of the wave walk grows to 176 entries
    (64 + 56 + 56 with the internal nodes of level 4 on top), past anything the other trees reach"""
    reference = reference_of(request, be)
    tree = hs.wide_tree(oracle, kb, curve)
    assert tree.nl == 8 ** hs.WIDE_LEVEL
    box = Box(UNIT, (1, 1, 1))
    for rb, t in ((32, 0), (64, tree.nl // 2 + 5)):
        centers = centres_of("huge", tree, box, rb)
        m = check_mark_macs(be, oracle, reference, tree, centers, box, rb, tree.leaves[t:t + 2], 0, None, (t, rb))
        assert m.walked.size == 1
        peak = m.peak(tree)
        assert peak == 176 and peak < 1024, peak
        assert int(m.marks.sum()) == tree.child.size - 1  # everything but the focus leaf


def interior_focus(tree):
    """512 finest cells that fill one aligned cube of edge 8 in the middle of the grid, as a cornerstone array"""
    R = tree.R
    key = int(fs.encode_cells([[R // 2 + 16, R // 4 + 8, R // 8 + 24]], tree.curve, tree.kb)[0]) // 512 * 512
    return np.arange(key, key + 513, dtype=np.uint64).astype(key_dtype(tree.kb))


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("curve", CURVES)
@KB
def test_mark_macs_interior_focus_probes(be, oracle, request, kb, curve, rb):
    """a focus deep inside the grid, of 512 deepest-level targets that are not leaves of the tree: a target is skipped
    exactly if its cube grown by one cell stays inside the focus cube (6^3 of them), both outcomes of the envelope
    branch.  One probe leaf per target (probe_centers) makes the marks show WHICH targets were walked; a third of the
    probes has radius 0 (a distance of 0 is not below it), a third a negative radius (|.| is taken)"""
    reference = reference_of(request, be)
    tree = hs.aniso_tree(oracle, kb, curve)
    focus = interior_focus(tree)
    box = Box(hs.ANISO, hs.BCS["012"])
    sign = lambda i: (1.0, 0.0, -1.0)[i % 3]
    centers, probe = fs.probe_centers(tree, box, rb, focus, sign)
    m = check_mark_macs(be, oracle, reference, tree, centers, box, rb, focus, 0, None, "interior")
    assert (m.level == tree.L).all() and not (m.branch == fs.OUT_OF_GRID).any()
    assert int(m.skipped.sum()) == 6 ** 3 and m.walked.size == 512 - 6 ** 3
    # the marks of the probes are the walked targets, less those whose probe has radius 0
    assert np.array_equal(m.marks[probe] != 0, ~m.skipped & (np.arange(512) % 3 != 1))
    # the shape tells these rules from their neighbours: the high corner minus one, `<`, |radius|
    for variant in ("ehi", "le", "nofabs"):
        other = fs.MacModel(tree, centers, box, rb, focus, 0, None, variant=variant)
        assert not np.array_equal(other.marks, m.marks), variant
    assert int(fs.MacModel(tree, centers, box, rb, focus, 0, None, variant="ehi").skipped.sum()) == 5 ** 3


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("curve", CURVES)
@KB
def test_mark_macs_corner_focus(be, oracle, request, kb, curve, rb):
    """a focus at the corner of the grid where the curve starts: the grown cubes of the targets on the faces leave the
    grid, so these targets are walked although their neighbourhood may lie inside the focus.  With probes; also a focus
    array COARSER than the tree's leaves (the same particles, bucket 64, restricted to a range), which the header
    allows, with limit_source"""
    reference = reference_of(request, be)
    tree = hs.aniso_tree(oracle, kb, curve)
    box = Box(hs.ANISO, hs.BCS["111"])
    x, y, z = random_cloud(2000, Box(hs.ANISO), 64, 5, "clustered")
    keys = np.sort(oracle.compute_sfc_keys(curve, kb, x, y, z, Box(hs.ANISO)))
    coarse, _ = oracle.compute_octree(keys, 64)
    assert 8 < coarse.size - 1 < tree.nl // 3 and np.isin(coarse, tree.leaves).all()
    for focus, limit in ((tree.leaves[:200], 0), (coarse[:coarse.size // 2], 1), (coarse[coarse.size // 3:], 1)):
        centers, probe = fs.probe_centers(tree, box, rb, focus)
        m = check_mark_macs(be, oracle, reference, tree, centers, box, rb, focus, limit, preset(tree, 3), "corner")
        out = m.branch == fs.OUT_OF_GRID
        assert out.any() and not m.skipped[out].any() and (m.branch == fs.ENVELOPE_OUTSIDE).any()
        if limit == 0:
            assert (m.branch == fs.ENVELOPE_INSIDE).any()
            assert np.array_equal(m.marks[probe] != 0, ~m.skipped | (m.initial[probe] != 0))
            # ... and would be wrong if a cube that leaves the grid counted as contained
            other = fs.MacModel(tree, centers, box, rb, focus, limit, m.initial, variant="outgrid_true")
            assert not np.array_equal(other.marks, m.marks), int(other.skipped.sum()) - int(m.skipped.sum())
    assert int(coarse[1]) - int(coarse[0]) >= end_key(kb) // 64  # the coarse focus starts with a target of level <= 2


@pytest.mark.parametrize("curve", CURVES)
@KB
def test_encoder_inverts_the_decoder(kb, curve):
    fs.check_encoder(curve, kb)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the per-node and per-leaf kernels
# ----------------------------------------------------------------------------------------------------------------------

def node_trees(oracle, kb):
    """(name, leaves): root only, the root's children, deepest-level leaves, about 1300 leaves, and 255 / 256 / 257 nodes"""
    out = [("single", hs.single_tree(oracle, kb, HILBERT).leaves), ("eight", hs.eight_tree(oracle, kb, HILBERT).leaves),
           ("deep", hs.deep_tree(oracle, kb, HILBERT, "mixed").leaves), ("aniso", hs.aniso_tree(oracle, kb, HILBERT).leaves)]
    # 1 + 8 s nodes after s splits: 257 nodes (225 leaves); 255 and 256 nodes do not exist for an octree, the node
    # counts either side of the 256-thread workgroup are 249 and 257, and the leaf counts 253 and 260
    out += [("n249", S.split_tree(kb, 31, 7)), ("n257", S.split_tree(kb, 32, 7)), ("l253", S.split_tree(kb, 36, 8)),
            ("l260", S.split_tree(kb, 37, 8))]
    return out


def focus_ranges(leaves, kb):
    """(name, first leaf, last leaf): empty, whole, one leaf, and a range that cuts through a sibling group on both sides"""
    nl = leaves.size - 1
    out = [("empty", nl // 2, nl // 2), ("whole", 0, nl), ("one", nl // 3, nl // 3 + 1)]
    if nl >= 16:
        lv = S.leaf_levels(leaves)
        # first leaves of sibling groups: a leaf whose key is a multiple of eight times its span
        heads = [i for i in range(nl - 7) if int(leaves[i]) % (8 * (int(leaves[i + 1]) - int(leaves[i]))) == 0
                 and (lv[i:i + 8] == lv[i]).all()]
        a, b = heads[len(heads) // 4], heads[3 * len(heads) // 4]
        out.append(("cut", a + 3, b + 5))
    return out


def call_essential(be, kb, o, counts, macs, fs_, fe, bucket):
    up = Hold(be)
    nn = o["num_nodes"]
    ops = be.filled(nn, np.int32, 77)
    par = o["parents"] if o["parents"].size else np.zeros(1, np.int32)
    be.chk(be.lib.cstone_hip_rebalance_decision_essential(
        be.ctx, C.c_int(kb), up(o["prefixes"]), up(o["child_offsets"]),
        up(par), up(counts), up(macs), C.c_uint64(fs_), C.c_uint64(fe),
        C.c_uint(bucket), be.ptr(ops), C.c_int(nn)), "essential")
    return be.to_host(ops, np.int32)


def call_protect(be, kb, o, ops):
    up = Hold(be)
    d = be.to_dev(ops)
    conv = C.c_int(-1)
    par = o["parents"] if o["parents"].size else np.zeros(1, np.int32)
    be.chk(be.lib.cstone_hip_protect_ancestors(be.ctx, C.c_int(kb), up(o["prefixes"]),
                                               up(par), be.ptr(d), C.c_int(o["num_nodes"]),
                                               C.byref(conv)), "protect")
    return be.to_host(d, np.int32), bool(conv.value)


@KB
def test_rebalance_decisions(be, oracle, request, kb):
    """rebalance_decision_essential, mac_refine_decision and protect_ancestors on the root-only tree, the root's
    children, leaves at the deepest level, 249 / 257 nodes and 253 / 260 leaves (an octree has 1 + 8 s nodes and 1 + 7 s
    leaves: these are the counts either side of the 256-thread workgroup); focus empty, whole, one leaf and cut through
    a sibling group on both sides; counts at bucket, bucket + 1 and 2^32 - 1; macs all 0, all 1 and random"""
    up = Hold(be)
    reference = reference_of(request, be)
    L = max_level(kb)
    bucket = 16
    seen = {0: 0, 1: 0, 8: 0, "fringe": 0, "deepest": 0, "sizes": set()}
    for name, leaves in node_trees(oracle, kb):
        o = S.linked(oracle, leaves)
        nn, nl = o["num_nodes"], leaves.size - 1
        seen["sizes"].add(nn)
        nk = fs.node_keys(o, kb)
        l2i = np.ascontiguousarray(o["leaf_to_internal"][o["num_internal"]:])
        deepest_leaves = sum(1 for n in l2i.tolist() if nk[n][1] == L)
        if name == "deep":
            assert deepest_leaves == 8
        seen["deepest"] += deepest_leaves
        rng = np.random.default_rng(nn)
        for cname, counts in (("edge", rng.permutation(np.resize(np.array([bucket, bucket + 1, 0, 0xFFFFFFFF], np.uint32), nn))),
                              ("big", np.full(nn, bucket + 1, np.uint32))):
            assert {bucket, bucket + 1, 0xFFFFFFFF} <= set(counts.tolist()) or nn < 9 or cname == "big"
            for mname, macs in (("m0", np.zeros(nn, np.int8)), ("m1", np.ones(nn, np.int8)),
                                ("mr", (rng.random(nn) < 0.4).astype(np.int8))):
                for fname, f, l in focus_ranges(leaves, kb):
                    what = (name, cname, mname, fname)
                    fs_, fe = int(leaves[f]), int(leaves[l])
                    want = fs.essential_model(o, kb, counts, macs, fs_, fe, bucket)
                    got = call_essential(be, kb, o, counts, macs, fs_, fe, bucket)
                    assert np.array_equal(got, want), what
                    for v in (0, 1, 8):
                        seen[v] += int((want == v).sum())
                    seen["fringe"] += int(not np.array_equal(
                        want, fs.essential_model(o, kb, counts, macs, fs_, fe, bucket, variant="nofringe")))
                    if reference is not None:
                        assert np.array_equal(reference.essential_ops(o, counts, macs, fs_, fe, bucket), want), what

                    # protect_ancestors: the sequential rule, a fixed point, the converged flag
                    want_p, want_c = fs.protect_model(o, kb, want)
                    got_p, got_c = call_protect(be, kb, o, want)
                    assert np.array_equal(got_p, want_p) and got_c == want_c, what
                    again, again_c = call_protect(be, kb, o, got_p)
                    assert np.array_equal(again, got_p) and again_c == want_c, what
                    assert want_c == bool((want_p == 1).all())
                    if reference is not None:
                        rp, rc = reference.protect_ancestors(o, want)
                        assert np.array_equal(rp, want_p) and rc == want_c, what

                    ops = be.filled(nl, np.int32, 77)
                    be.chk(be.lib.cstone_hip_mac_refine_decision(
                        be.ctx, C.c_int(kb), up(o["prefixes"]), up(macs),
                        up(l2i), C.c_int(nl), C.c_int(f), C.c_int(l), be.ptr(ops)), "mac_refine")
                    want_r = fs.mac_refine_model(o, kb, macs, f, l)
                    assert np.array_equal(be.to_host(ops, np.int32), want_r), what
                    if reference is not None:
                        assert np.array_equal(reference.mac_refine_ops(o, macs, nl, f, l), want_r), what
                    if name == "deep" and mname == "m1" and fname == "empty":
                        # leaves at the deepest level are never split: the `level < maxLevel` guards
                        deep_nodes = [n for n in l2i.tolist() if nk[n][1] == L]
                        assert (want[deep_nodes] != 8).all() and (want_r[[nk[n][1] == L for n in l2i.tolist()]] == 1).all()
                        assert (want_r == 8).sum() == nl - 8
    be.chk(be.lib.cstone_hip_ctx_sync(be.ctx), "ctx_sync")
    assert seen[0] and seen[1] and seen[8] and seen["fringe"] and seen["deepest"] >= 8, seen
    assert {1, 9, 249, 257} <= seen["sizes"], seen["sizes"]


def enforce_cases(oracle, kb):
    """(name, octree, ops, keys, the status the case is built for)"""
    L = max_level(kb)
    end = end_key(kb)
    tree = hs.deep_tree(oracle, kb, HILBERT, "mixed")
    o = tree.o
    nk = fs.node_keys(o, kb)
    nn = o["num_nodes"]
    leaf_nodes = [n for n in range(nn) if o["child_offsets"][n] == 0]
    shallow = [n for n in leaf_nodes if 2 <= nk[n][1] <= L - 4 and nk[n][0] != 0]
    deepest = [n for n in leaf_nodes if nk[n][1] == L]
    assert len(deepest) == 8 and len(shallow) > 20
    rng = np.random.default_rng(kb)
    keep = np.ones(nn, np.int32)
    merge = np.where(np.array([nk[n][1] for n in range(nn)]) >= 2, 0, 1).astype(np.int32)
    merge[rng.random(nn) < 0.2] = 8  # splits among the siblings of the ancestors: a cancelled merge must not undo them
    merge[0] = 1
    starts = [nk[n][0] for n in shallow]
    below1 = [nk[n][0] + 3 * (nk[n][2] // 8) for n in shallow]
    below3 = [nk[n][0] + 5 * (nk[n][2] // 512) for n in shallow]
    at_deepest = [nk[n][0] for n in deepest if nk[n][0] % 8 != 0]  # keys of leaves at the deepest level
    out = [
        ("status0", o, keep, [0, end] + starts + at_deepest, 0),       # boundaries that exist, nothing to merge
        ("status1", o, merge, [0, end] + starts + at_deepest, 1),      # boundaries that exist, their nodes merge
        ("status2", o, merge, [0, end] + starts + below1, 2),          # one level below a leaf
        ("status3", o, merge, [0, end] + starts + below1 + below3[:1], 3),  # one key three levels below a leaf
        ("status2keep", o, keep, below1, 2),
        ("one", o, merge, below3[3:4], 3),
    ]
    # all keys share the same ancestors: the children and grandchildren of ONE deep leaf
    n = max(shallow, key=lambda n: nk[n][1])
    same = [nk[n][0] + i * (nk[n][2] // 64) for i in range(1, 64)]
    out.append(("shared", o, merge, same, 3))
    # key counts 1, 63, 64, 65, 1000 on the big tree, keys of every kind
    big = hs.aniso_tree(oracle, kb, HILBERT)
    bo, bk = big.o, fs.node_keys(big.o, kb)
    bl = [n for n in range(bo["num_nodes"]) if bo["child_offsets"][n] == 0 and bk[n][1] <= L - 3]
    bops = rng.choice(np.array([0, 1, 8], np.int32), bo["num_nodes"])
    bops[0] = 1
    for count in (1, 63, 64, 65, 1000):
        pick = rng.choice(bl, count)
        kind = rng.integers(0, 3, count)
        keys = [bk[n][0] + (0, 3 * (bk[n][2] // 8), 5 * (bk[n][2] // 512))[k] for n, k in zip(pick.tolist(), kind.tolist())]
        out.append((f"n{count}", bo, bops, keys, None))
    return out


@KB
def test_enforce_keys(be, oracle, request, kb):
    """enforce_keys against the reference's sequential loop restated: each status is the maximum once; keys 0 and the end
    key; boundaries that exist whose nodes merge; keys one and three levels below a leaf; keys of leaves at the deepest
    level (no key lies below such a leaf, the `haveLevel < maxLevel` guard cannot fire); all keys under one leaf; 1,
    63, 64, 65 and 1000 keys; and the list reversed: the result must not depend on the order.  Ops preset to 8 among the
    siblings of the cancelled merges tell the atomicMax there from a plain store of 1, a lone status 3 among 2s the one
    on the status; the split request always writes 8, the largest op there is, so there a plain store is the same"""
    up = Hold(be)
    reference = reference_of(request, be)
    reached = set()
    for name, o, ops, keys, status in enforce_cases(oracle, kb):
        keys = np.array(keys, dtype=key_dtype(kb))
        want, want_status = fs.enforce_model(keys, o, kb, ops)
        if status is not None:
            assert want_status == status, name
        reached.add(want_status)
        back, back_status = fs.enforce_model(keys[::-1], o, kb, ops)
        assert np.array_equal(back, want) and back_status == want_status, name  # the rule itself is order-free
        par = o["parents"] if o["parents"].size else np.zeros(1, np.int32)
        for order in (keys, np.ascontiguousarray(keys[::-1])):
            d = be.to_dev(ops)
            st = C.c_int(-1)
            be.chk(be.lib.cstone_hip_enforce_keys(be.ctx, C.c_int(kb), up(order), C.c_int(order.size),
                                                  up(o["prefixes"]), up(o["child_offsets"]),
                                                  up(par), be.ptr(d), C.byref(st)), "enforce_keys")
            assert np.array_equal(be.to_host(d, np.int32), want) and st.value == want_status, name
        if reference is not None:
            ref, ref_status = reference.enforce_keys(keys, o, ops)
            assert np.array_equal(ref, want) and ref_status == want_status, name
        if name == "status1":
            assert (ops == 8).sum() == (want == 8).sum() and (want == 0).sum() < (ops == 0).sum()  # splits survive
    assert reached == {0, 1, 2, 3}
    be.chk(be.lib.cstone_hip_ctx_sync(be.ctx), "ctx_sync")


def refine_into(start, span, count, seed):
    """`count` = 1 + 7 s leaves tiling the node [start, start + span), split s times at random"""
    assert (count - 1) % 7 == 0
    rng = np.random.default_rng(seed)
    keys = [start, start + span]
    while len(keys) - 1 < count:
        ok = [i for i in range(len(keys) - 1) if keys[i + 1] - keys[i] >= 8]
        i = ok[int(rng.integers(0, len(ok)))]
        step = (keys[i + 1] - keys[i]) // 8
        keys[i + 1:i + 1] = [keys[i] + s * step for s in range(1, 8)]
    return keys[:-1]


@KB
def test_range_count(be, oracle, request, kb):
    """range_count with 1, 15, 16, 17 and 257 listed leaves and duplicates among them; focus leaves that cover exactly 1,
    8, 15, 16, 17, 22, 64 and 1009 global leaves (a NODE splits into 1 + 7 s leaves; the contract only speaks of
    consecutive keys of leaves_focus, so 16 and 17 are the key ranges of two and three neighbouring nodes: 1 + 15 and
    1 + 15 + 1); leaves_focus identical to leaves; sums of exactly 2^32 - 1, one below and far above; entries that are
    not listed keep their preset value"""
    up = Hold(be)
    reference = reference_of(request, be)
    end = end_key(kb)
    span = end // 64
    sizes = [1, 15, 1, 8, 22, 1009, 1, 64, 36, 29] + [1] * 54  # global leaves under leaf i of the uniform level-2 tree
    focus = np.array([i * span for i in range(65)], dtype=key_dtype(kb))
    glob = []
    for i, s in enumerate(sizes):
        glob += refine_into(i * span, span, s, i)
    glob = np.array(glob + [end], dtype=key_dtype(kb))
    ng = glob.size - 1
    focus16, focus17 = np.delete(focus, [1]), np.delete(focus, [1, 2])
    covered = lambda f: np.diff(np.searchsorted(glob, f)).tolist()
    assert covered(focus) == sizes and covered(focus16)[0] == 16 and covered(focus17)[0] == 17 and max(sizes) > 1000
    rng = np.random.default_rng(kb)
    counts = rng.integers(1, 50, ng).astype(np.uint32)
    sat = counts.copy()
    lo = np.searchsorted(glob, focus).tolist()
    sat[lo[5]:lo[6]] = 0
    sat[lo[5] + 700], sat[lo[5] + 1] = 0xFFFFFFFF - 5, 5             # exactly 2^32 - 1 under focus leaf 5
    sat[lo[4]:lo[5]] = 0
    sat[lo[4] + 20], sat[lo[4] + 3] = 0xFFFFFFFF - 5, 4              # one below under focus leaf 4
    sat[lo[7]:lo[8]] = 0x10000000                                    # 64 x 2^28 = 2^34 under focus leaf 7
    lists = {1: [5], 15: list(range(15)), 16: list(range(16)), 17: list(range(16)) + [4],
             257: [int(v) for v in rng.integers(0, 60, 257)]}
    for name, focus_arr in (("level2", focus), ("sixteen", focus16), ("seventeen", focus17), ("identical", glob)):
        nfa = focus_arr.size - 1
        for cname, cnt in (("plain", counts), ("saturated", sat)):
            for n, idx in lists.items():
                idx = np.array(idx, dtype=np.int32)
                if name == "identical":
                    idx = rng.integers(0, nfa, n).astype(np.int32)
                    idx[-1] = idx[0]
                assert idx.size == n and idx.max() < nfa and (n < 17 or np.unique(idx).size < n)  # duplicates
                start = rng.integers(1, 1000, nfa).astype(np.uint32)
                want = fs.range_count_model(glob, cnt, focus_arr, idx, start)
                out = be.to_dev(start)
                be.chk(be.lib.cstone_hip_range_count(be.ctx, C.c_int(kb), up(glob), C.c_int(ng),
                                                     up(cnt), up(focus_arr),
                                                     up(idx), C.c_int(n), be.ptr(out)), "range_count")
                assert np.array_equal(be.to_host(out, np.uint32), want), (name, cname, n)
                rest = np.setdiff1d(np.arange(nfa), idx)
                assert rest.size and np.array_equal(want[rest], start[rest])
                if reference is not None:
                    assert np.array_equal(reference.range_count(glob, cnt, focus_arr, idx, start), want), (name, cname, n)
                if name == "level2" and cname == "saturated" and n >= 15:
                    assert want[5] == 0xFFFFFFFF and want[4] == 0xFFFFFFFE and want[7] == 0xFFFFFFFF
                if name == "identical":
                    assert np.array_equal(want[idx], cnt[idx])
    be.chk(be.lib.cstone_hip_ctx_sync(be.ctx), "ctx_sync")


def gap_arrays(oracle, kb):
    L, end = max_level(kb), end_key(kb)
    e8 = end // 8
    leaves = hs.aniso_tree(oracle, kb, HILBERT).leaves
    rng = np.random.default_rng(kb)
    out = [("root", [0, end]),
           ("cells", [0, 1, 2, 8, 9, 64, end - 9, end - 8, end - 1, end]),                 # one finest cell apart
           ("levels", [0, 1, e8, 5 * e8 + 1, 5 * e8 + 2, 6 * e8, end]),                    # level 1 <-> the deepest level
           ("zero digit", [0, 0o101, 0o1000, 0o1000 + 0o1001 * 8, 3 * e8 + 0o70, end]),    # digits 0 between others
           ("cornerstone", [int(k) for k in leaves])]
    for n in (255, 256, 257):
        pick = np.sort(rng.choice(np.arange(1, leaves.size - 1), n - 1, replace=False))
        out.append((f"p{n}", [0] + [int(k) for k in leaves[pick]] + [end]))
    return out


@KB
def test_sfc_gaps(be, oracle, request, kb):
    """count_sfc_gaps / fill_sfc_gaps against "the fewest aligned nodes that tile [a, b)": the pair [0, endKey); keys one
    finest cell apart; from a level-1 boundary to a deepest-level key and back; starts with zero digits between
    non-zero ones; a full cornerstone array (every count 1); 255, 256 and 257 pairs.  The terminal key is written and
    nothing behind it"""
    up = Hold(be)
    reference = reference_of(request, be)
    L = max_level(kb)
    kdt = key_dtype(kb)
    sentinel = 0x2BADBADB
    for name, keys in gap_arrays(oracle, kb):
        m = len(keys) - 1
        tiles = [fs.tile(keys[i], keys[i + 1], kb) for i in range(m)]
        want_counts = np.array([len(t) for t in tiles], dtype=np.int32)
        for t, a, b in zip(tiles, keys[:-1], keys[1:]):   # the model tiles: aligned nodes, end to end
            sizes = [y - x for x, y in zip(t, t[1:] + [b])]
            assert t[0] == a and all(s & (s - 1) == 0 and s.bit_length() % 3 == 1 and x % s == 0 for x, s in zip(t, sizes))
        if name == "cornerstone":
            assert (want_counts == 1).all()
        if name == "root":
            assert want_counts.tolist() == [1]
        if name == "levels":
            assert want_counts.tolist()[1:3] == [7 * (L - 1), 4 + 1] and max(want_counts) == 7 * (L - 1)
        if name == "zero digit":
            digits = lambda a: [(a >> (3 * i)) & 7 for i in range(L)]
            assert any(0 in digits(a)[digits(a).index(next(d for d in digits(a) if d)):(a ^ b).bit_length() // 3 - 1]
                       for a, b in zip(keys[1:-1], keys[2:]) if a)
        tree = be.to_dev(np.array(keys, dtype=kdt))
        ops = be.filled(m + 1, np.int32, 77)
        be.chk(be.lib.cstone_hip_count_sfc_gaps(be.ctx, C.c_int(kb), be.ptr(tree), C.c_int(m), be.ptr(ops)), "count_gaps")
        got = be.to_host(ops, np.int32)
        assert np.array_equal(got[:m], want_counts) and got[m] == 77, name
        scan = np.concatenate([[0], np.cumsum(want_counts)]).astype(np.int32)
        total = int(scan[-1])
        new = be.filled(total + 1 + 8, kdt, sentinel)
        be.chk(be.lib.cstone_hip_fill_sfc_gaps(be.ctx, C.c_int(kb), be.ptr(tree), C.c_int(m), up(scan),
                                               be.ptr(new)), "fill_gaps")
        want = np.array([k for t in tiles for k in t] + [keys[-1]] + [sentinel] * 8, dtype=kdt)
        assert np.array_equal(be.to_host(new, kdt), want), name
        if reference is not None:
            for i in range(m):
                assert reference.span_sfc_range(kb, keys[i], keys[i + 1]).tolist() == tiles[i], (name, i)
    be.chk(be.lib.cstone_hip_ctx_sync(be.ctx), "ctx_sync")


def test_add_macs(be):
    """add_macs on its own: flags preset to 0, 1 and 5 (only a 0 becomes 1); 0, 1, 255, 256 and 257 leaves; MAC marks on
    internal nodes only set nothing"""
    up = Hold(be)
    rng = np.random.default_rng(3)
    for nl in (0, 1, 255, 256, 257):
        nn = nl + 40
        l2i = rng.permutation(nn)[:nl].astype(np.int32)
        internal = np.setdiff1d(np.arange(nn), l2i)
        flags = rng.choice(np.array([0, 1, 5], np.int32), nl)
        for kind in ("random", "internal", "all"):
            macs = (rng.random(nn) < 0.5).astype(np.int8) if kind == "random" else np.ones(nn, np.int8)
            if kind == "internal":
                macs[l2i] = 0
                assert macs[internal].all()
            want = np.where((macs[l2i] != 0) & (flags == 0), 1, flags).astype(np.int32)
            out = be.to_dev(np.concatenate([flags, [9, 9]]).astype(np.int32))
            be.chk(be.lib.cstone_hip_add_macs(be.ctx, up(macs), up(np.concatenate([l2i, [0]]).astype(np.int32)),
                                              C.c_int(nl), be.ptr(out)), "add_macs")
            got = be.to_host(out, np.int32)
            assert np.array_equal(got[:nl], want) and got[nl:].tolist() == [9, 9], (nl, kind)
            if kind == "internal":
                assert np.array_equal(want, flags)
            if nl >= 255 and kind != "internal":
                assert {0, 1, 5} <= set(flags.tolist()) and (want != flags).any() and (want == 5).any()
    be.chk(be.lib.cstone_hip_ctx_sync(be.ctx), "ctx_sync")


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("curve", CURVES)
@KB
def test_mac_spheres(be, oracle, request, kb, curve, rb):
    """geo_mac_spheres and set_mac against the numpy model in T: the anisotropic box and a box with negative limits, both
    curves on trees of their own, nodes at the deepest level, two opening angles; set_mac with mass 0 and with the
    centre exactly at the geometric centre"""
    reference = reference_of(request, be)
    T = real_dtype(rb)
    for tree in (hs.aniso_tree(oracle, kb, curve), hs.deep_tree(oracle, kb, curve, "mixed")):
        nn = tree.child.size
        assert tree.nl > 1000 or (tree.node_level == tree.L).sum() == 8
        pre = be.to_dev(tree.o["prefixes"])
        for lim, bc in ((hs.ANISO, (0, 0, 0)), (NEG, (1, 2, 0))):
            box = Box(lim, bc)
            cb = fs.cbox(box)
            for inv_theta in (2.5, 1.0 / 0.8 + 0.5):
                want = fs.geo_spheres_model(tree, box, rb, inv_theta)
                sph = be.filled(4 * nn, T, -7)
                be.chk(be.lib.cstone_hip_geo_mac_spheres(be.ctx, C.c_int(curve), C.c_int(kb), C.c_int(rb), be.ptr(pre),
                                                         C.c_int(nn), be.ptr(sph), C.c_float(inv_theta), C.byref(cb)),
                       "geo_mac_spheres")
                assert np.array_equal(be.to_host(sph, T).reshape(nn, 4), want), (lim, inv_theta)
                rng = np.random.default_rng(nn)
                com = want.copy()
                com[:, :3] += (rng.uniform(-1, 1, (nn, 3)) * 0.01).astype(T)
                com[:, 3] = (rng.random(nn) < 0.8).astype(T) * T(3.5)
                com[::5, :3] = want[::5, :3]  # exactly at the geometric centre
                assert (com[:, 3] == 0).any() and (com[::5, 3] != 0).any()
                want2 = fs.set_mac_model(tree, box, rb, inv_theta, com)
                assert (want2[com[:, 3] == 0, 3] == 0).all() and np.array_equal(want2[::5, 3][com[::5, 3] != 0],
                                                                                 want[::5, 3][com[::5, 3] != 0])
                cd = be.to_dev(com.reshape(-1))
                be.chk(be.lib.cstone_hip_set_mac(be.ctx, C.c_int(curve), C.c_int(kb), C.c_int(rb), be.ptr(pre), C.c_int(nn),
                                                 be.ptr(cd), C.c_float(inv_theta), C.byref(cb)), "set_mac")
                assert np.array_equal(be.to_host(cd, T).reshape(nn, 4), want2), (lim, inv_theta)
                if reference is not None and curve == HILBERT:
                    assert np.array_equal(reference.mac_spheres(curve, 0, tree.o["prefixes"], box, inv_theta, rb), want)
                    assert np.array_equal(reference.mac_spheres(curve, 1, tree.o["prefixes"], box, inv_theta, rb, com), want2)
    be.chk(be.lib.cstone_hip_ctx_sync(be.ctx), "ctx_sync")


def particle_layouts(nl, rng):
    """(name, particles per leaf)"""
    mixed = np.array([(0, 1, 64, 65, 2, 0, 3, 5)[i % 8] for i in range(nl)])
    if nl > 8:
        mixed[nl // 2] = 700
        mixed[nl // 2 + 1] = 0   # an empty leaf next to a full one
    one = np.zeros(nl, dtype=np.int64)
    one[nl // 3] = 900           # one leaf holds everything
    return [("mixed", mixed), ("one", one)]


@pytest.mark.parametrize("tc,tm,tf", [(64, 64, 64), (64, 32, 64), (32, 32, 32)])
def test_source_centers(be, oracle, request, tc, tm, tf):
    """leaf_source_centers, upsweep_centers and move_centers against a serial loop in Tf: empty leaves, leaves of 1, 64,
    65 and 700 particles, one leaf holding everything, a subtree whose masses are all zero (centre (0,0,0), mass 0, and
    the parent's inv = 1 branch) among negative masses, the three type triples, the root-only tree"""
    up = Hold(be)
    reference = reference_of(request, be)
    kb = 64
    Tf = real_dtype(tf)
    rng = np.random.default_rng(tc + tm)
    for tname, leaves in (("l253", S.split_tree(kb, 36, 8)), ("root", hs.single_tree(oracle, kb, HILBERT).leaves),
                          ("eight", hs.eight_tree(oracle, kb, HILBERT).leaves)):
        o = S.linked(oracle, leaves)
        nn, nl = o["num_nodes"], leaves.size - 1
        l2i = np.ascontiguousarray(o["leaf_to_internal"][o["num_internal"]:])
        child = o["child_offsets"]
        for lname, per_leaf in particle_layouts(nl, rng):
            layout = np.concatenate([[0], np.cumsum(per_leaf)]).astype(np.uint32)
            n = int(layout[-1])
            x, y, z = [rng.uniform(-2, 3, n).astype(real_dtype(tc)) for _ in range(3)]
            m = rng.uniform(-1, 1, n).astype(real_dtype(tm))
            zero_parent = None
            if tname == "l253" and lname == "mixed":
                # an internal node, not the root, all of whose children are leaves and hold particles: masses zero
                leaf_of = {int(node): i for i, node in enumerate(l2i)}
                for p in range(1, nn):
                    kids = range(int(child[p]), int(child[p]) + 8)
                    if child[p] and all(child[k] == 0 for k in kids) and sum(per_leaf[leaf_of[k]] for k in kids) > 100:
                        zero_parent = p
                        for k in kids:
                            m[layout[leaf_of[k]]:layout[leaf_of[k] + 1]] = 0
                        break
                assert zero_parent is not None and (m < 0).any()
            want = fs.source_centers_model(x, y, z, m, l2i, layout, nn, Tf)
            ctr = be.filled(4 * nn, Tf, 0)
            be.chk(be.lib.cstone_hip_leaf_source_centers(
                be.ctx, C.c_int(tc), C.c_int(tm), C.c_int(tf), up(x), up(y),
                up(z), up(m), up(l2i), C.c_int(nl), up(layout),
                be.ptr(ctr)), "leaf_source_centers")
            assert np.array_equal(be.to_host(ctr, Tf).reshape(nn, 4), want), (tname, lname)
            empty = l2i[per_leaf == 0]
            assert (want[empty] == 0).all() and (empty.size > 0 or nl == 1)
            swept = fs.upsweep_model(o, want)
            lr = np.ascontiguousarray(o["level_range"], dtype=np.int32)
            be.chk(be.lib.cstone_hip_upsweep_centers(be.ctx, C.c_int(tf), C.c_int(max_level(kb)),
                                                     lr.ctypes.data_as(C.c_void_p), up(child), be.ptr(ctr)),
                   "upsweep_centers")
            assert np.array_equal(be.to_host(ctr, Tf).reshape(nn, 4), swept), (tname, lname)
            assert not np.isnan(swept).any()
            if tname == "root":
                assert nn == 1 and np.array_equal(swept, want)  # no level to sweep
            if zero_parent is not None:
                assert (swept[zero_parent] == 0).all() and swept[0, 3] > 0
                assert np.isnan(fs.upsweep_model(o, want, variant="noguard")[zero_parent]).any()
            if reference is not None:
                ref = reference.leaf_source_centers(x, y, z, m, l2i, layout, nn, tf)
                assert np.array_equal(ref, want), (tname, lname)
                assert np.array_equal(reference.upsweep_centers(o, ref, max_level(kb)), swept), (tname, lname)
            if hasattr(be.lib, "cstone_hip_move_centers"):  # (the CPU restatement behind the ABI has no such entry)
                src = np.ascontiguousarray(swept[:, :3]).reshape(-1)
                dst = be.filled(4 * nn + 4, Tf, -7)
                be.chk(be.lib.cstone_hip_move_centers(be.ctx, C.c_int(tf), up(src), C.c_int(nn), be.ptr(dst)),
                       "move_centers")
                got = be.to_host(dst, Tf)
                assert np.array_equal(got[:4 * nn].reshape(nn, 4)[:, :3], swept[:, :3]) and (got[3:4 * nn:4] == 1).all()
                assert (got[4 * nn:] == -7).all()
    be.chk(be.lib.cstone_hip_ctx_sync(be.ctx), "ctx_sync")
