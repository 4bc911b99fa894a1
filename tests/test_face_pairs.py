"""The neighbour walk and friends-of-friends on pairs across a cell face at a distance within one ulp of the search radius
(tests/face_support.py): the one place where the walk's node test and its pair test can disagree.  There the walk reports
a pair from ONE side only -- the node test of the other particle's leaf, or of an ancestor, fails by a rounding although
the pair test would pass.  This is the reference's behaviour (its own findNeighbors does the same, asserted below), so
cstone_hip_find_neighbors must drop exactly those pairs; cstone_hip_friends_of_friends links a pair that EITHER walk
reports, so its groups must not depend on which of the two particles has the larger index.

The model (face_support.walk_relation) is built from the two tables of tests/neighbors_support.py alone; the CPU tests
establish that the oracle's lists are the model's and the reference's, that every shape has one-sided pairs of both
orientations, and that a fused multiply-add in the node test would change which pairs are dropped.  All comparisons
are ==.  Across ranks (the last test) every rank walks its own focus tree, of which there is no model here: the cloud
there is compared with the brute force over the whole cloud, which is the closure wherever no pair is missed from both
sides."""
import numpy as np
import pytest

import face_support as fa
import fof_support as fs

RBS = [32, 64]
NAMES = list(fa.SHAPES)
FOF_PAIRS = 32  # one-sided pairs of each orientation that get a friends-of-friends call of their own


def listed(lists, counts, n):
    """got[t, j]: j is among the first counts[t] entries of row t; no entry twice"""
    got = np.zeros((counts.size, n), dtype=bool)
    m = np.arange(lists.shape[1])[None, :] < counts[:, None]
    got[np.nonzero(m)[0], lists[m]] = True
    assert np.array_equal(got.sum(1), counts)
    return got


def oracle_lists(fc, impl):
    case = fc.case
    ngmax = int(case.pair_table().sum(1).max()) + 1
    lists, counts = case.find(impl, 0, case.n, ngmax)
    assert counts.max() < ngmax
    return lists, counts, ngmax


def check_premise(oracle, name, rb):
    """at least 4 one-sided pairs of each orientation, none missed from both sides, the brute force links every pair"""
    fc = fa.face_case(oracle, name, rb)
    sides = fa.one_sided(fc)
    a, b = fa.threshold_pairs(fc)
    nb = fc.case.pair_table()
    assert fc.n <= 1200 and a.size >= 250
    assert nb[a, b].all() and nb[b, a].all()
    assert len(sides.blind_larger) >= 4 and len(sides.blind_smaller) >= 4, (len(sides.blind_larger), len(sides.blind_smaller))
    assert len(sides.neither) == 0
    return fc, sides


# ---- CPU -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", NAMES)
def test_premise_one_sided_pairs_of_both_orientations(oracle, name, rb):
    """every shape: at most 1200 particles, at least 250 threshold pairs in different leaves, each linked by the brute
    force from both sides (the brute force is symmetric), at least 4 that the walk reports from the smaller index only and
    4 from the larger index only, and none that it misses from both sides -- so the symmetric closure of the walk is the
    brute force on these shapes.  A pair's two thresholds (one per target: the fold is the target's) are equal throughout"""
    fc, sides = check_premise(oracle, name, rb)
    a, _ = fa.threshold_pairs(fc)
    print(f"{name} f{rb}: n {fc.n}, nodes {fc.case.o['num_nodes']}, threshold pairs {a.size}, seen from both sides "
          f"{len(sides.both)}, larger index blind {len(sides.blind_larger)}, smaller index blind "
          f"{len(sides.blind_smaller)}, missed from both sides {len(sides.neither)}")
    assert np.array_equal(fc.case.h, fc.case.h[fc.partner])
    axes = set(fc.axis[np.concatenate([sides.blind_larger[:, 0], sides.blind_smaller[:, 0]])].tolist())
    assert axes == {0, 1, 2}  # every displacement axis contributes


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_lists_equal_the_model(oracle, name, rb):
    """walk_relation == the oracle's find_neighbors lists as sets, every target at the threshold h of its own partner"""
    fc = fa.face_case(oracle, name, rb)
    lists, counts, _ = oracle_lists(fc, oracle)
    assert np.array_equal(listed(lists, counts, fc.n), fa.walk_relation(fc.case))


@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_reference(oracle, reference, name, rb):
    """the reference's own findNeighbors on the same inputs: counts and lists, entry for entry.  The one-sidedness is the
    reference's behaviour"""
    fc = fa.face_case(oracle, name, rb)
    lo, co, ngmax = oracle_lists(fc, oracle)
    lr, cr = fc.case.find(reference, 0, fc.n, ngmax)
    assert np.array_equal(co, cr) and np.array_equal(lo, lr)
    sides = fa.one_sided(fc, listed(lr, cr, fc.n))
    mine = fa.one_sided(fc)
    assert np.array_equal(sides.blind_larger, mine.blind_larger) and np.array_equal(sides.blind_smaller, mine.blind_smaller)


def test_a_fused_node_test_drops_other_pairs(oracle):
    """the mutant of the model whose node test rounds every a * b + c once, as the kernel would if neighbors.hip or fof.hip
    were compiled with contraction: on at least one float32 shape the one-sided set differs -- the GPU tests below would
    see such a kernel"""
    differs = []
    for name in NAMES:
        fc = fa.face_case(oracle, name, 32)
        mine = fa.one_sided(fc)
        fused = fa.one_sided(fc, fa.relation_from(fc.case, fa.node_table_fused(fc.case)))
        same = all(np.array_equal(getattr(mine, k), getattr(fused, k)) for k in ("blind_larger", "blind_smaller", "neither"))
        print(f"{name} f32, fused node test: larger index blind {len(fused.blind_larger)} (unfused {len(mine.blind_larger)}),"
              f" smaller index blind {len(fused.blind_smaller)} ({len(mine.blind_smaller)}), missed from both sides "
              f"{len(fused.neither)}")
        differs.append(not same)
    assert any(differs)


def test_closure_labels_on_a_hand_made_relation():
    rel = np.zeros((6, 6), dtype=bool)
    rel[4, 1] = rel[2, 5] = rel[5, 4] = rel[0, 3] = True  # one-sided throughout
    assert fa.closure_labels(rel, 0, 6).tolist() == [0, 1, 1, 0, 1, 1]
    assert fa.closure_labels(rel, 1, 5).tolist() == [1, 2, 3, 1]  # 0 and 5 are no targets: they link nothing


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


class DevCloud:
    """the arrays of a case on the device, uploaded once"""

    def __init__(self, hip, case):
        import cstone_amd

        self.hip, self.case = hip, case
        self.x, self.y, self.z = (_dev(a) for a in (case.x, case.y, case.z))
        self.tree = dict(child_offsets=_dev(case.o["child_offsets"]), internal_to_leaf=_dev(case.o["internal_to_leaf"]))
        self.layout, self.cen, self.siz = _dev(case.layout), _dev(case.cen), _dev(case.siz)
        self.cbox = cstone_amd.make_cbox(case.box.lim, case.box.bc)

    def fof(self, b):
        """(labels, sizes, number of groups) of one cstone_hip_friends_of_friends over the whole cloud"""
        lab, gs, ng = self.hip.friends_of_friends(self.x, self.y, self.z, 0, self.case.n, self.cbox, self.tree, self.layout,
                                                  self.cen, self.siz, b)
        self.hip.sync()  # raises if the sticky device-side error word is set
        return _u32(lab), _u32(gs), ng


_models = {}


def fof_model(fc, key, h):
    """(labels, sizes, number of groups) of the model's symmetric closure with every particle at h, and the labels of a
    link pass that unites from the larger index only"""
    if key + (float(h),) not in _models:
        rel = fa.walk_relation(fa.uniform_case(fc.case, h))
        labels = fa.closure_labels(rel, 0, fc.n)
        _models[key + (float(h),)] = (labels, fs.sizes_of(labels, 0), int((labels == np.arange(fc.n)).sum()),
                                      fa.larger_only_labels(rel, 0, fc.n))
    return _models[key + (float(h),)]


def linking_length(case, h):
    """b = 2 h as the double the call takes, with T(0.5) * T(b) == h exactly"""
    T = case.x.dtype.type
    b = 2.0 * float(h)
    assert fs.half_length(T, b) == h
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", NAMES)
def test_hip_find_neighbors_drops_exactly_the_models_pairs(hip, oracle, name, rb):
    """one call of find_neighbors over all targets, each at the threshold h of its partner, and one of
    find_neighbors_groups on fixed groups of 64: counts and lists equal the oracle's entry for entry, and of the threshold
    pairs exactly those are missing that the model drops, in both orientations.  A node test that is not the reference's,
    rounding for rounding (a contraction, another order of the sum), fails here"""
    fc, sides = check_premise(oracle, name, rb)
    case, n = fc.case, fc.n
    ref_l, ref_c, ngmax = oracle_lists(fc, oracle)
    d = DevCloud(hip, case)
    h = _dev(case.h)
    plain = hip.find_neighbors(d.x, d.y, d.z, h, 0, n, d.cbox, d.tree, d.layout, d.cen, d.siz, ngmax)
    groups = hip.compute_fixed_groups(0, n, 64)
    assert groups.numel() - 1 == (n + 63) // 64
    grouped = hip.find_neighbors_groups(d.x, d.y, d.z, h, 0, n, groups, d.cbox, d.tree, d.layout, d.cen, d.siz, ngmax)
    hip.sync()
    stored = np.arange(ngmax)[None, :] < ref_c[:, None]
    a, b = fa.threshold_pairs(fc)
    for what, (lists, counts) in (("plain", plain), ("groups", grouped)):
        lists, counts = _u32(lists), _u32(counts)
        bad = np.flatnonzero(counts != ref_c)
        assert bad.size == 0, (what, "counts", bad[:8].tolist(), counts[bad[:8]].tolist(), ref_c[bad[:8]].tolist())
        bad = np.flatnonzero(((lists != ref_l) & stored).any(1))
        assert bad.size == 0, (what, "rows", bad[:8].tolist(), lists[bad[:3]].tolist(), ref_l[bad[:3]].tolist())
        got = fa.one_sided(fc, listed(lists, counts, n))
        for k in ("both", "blind_larger", "blind_smaller", "neither"):
            assert np.array_equal(getattr(got, k), getattr(sides, k)), (what, k, len(getattr(got, k)), len(getattr(sides, k)))
    print(f"{name} f{rb}: {a.size} threshold pairs, dropped from the larger index {len(sides.blind_larger)}, from the "
          f"smaller {len(sides.blind_smaller)}")


def chosen_pairs(fc, sides):
    """up to FOF_PAIRS one-sided pairs of each orientation whose b = 2 h the call takes: [(a, b, larger index blind)]"""
    out = []
    for pairs, larger in ((sides.blind_larger, True), (sides.blind_smaller, False)):
        ok = [(int(a), int(b), larger) for a, b in pairs if fa.admissible(fc.case, 2.0 * float(fc.case.h[a]))]
        out += ok[:FOF_PAIRS]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
@pytest.mark.parametrize("name", NAMES)
def test_hip_fof_links_a_pair_seen_from_either_side(hip, oracle, name, rb):
    """for up to 32 one-sided pairs of each orientation: one call on the whole cloud at b = 2 h of the pair; labels, sizes
    and the number of groups equal the symmetric closure of the model's relation at that b, and the two particles of the
    pair share a label.  A link pass that unites only from the larger index leaves the pairs apart whose larger index is
    blind"""
    fc, sides = check_premise(oracle, name, rb)
    pairs = chosen_pairs(fc, sides)
    assert sum(p[2] for p in pairs) >= 4 and sum(not p[2] for p in pairs) >= 4 and len(pairs) <= 2 * FOF_PAIRS
    d = DevCloud(hip, fc.case)
    bad, sharp = [], 0
    for a, b, larger_blind in pairs:
        h = fc.case.h[a]
        want_l, want_s, want_n, one_way = fof_model(fc, (name, rb), h)
        assert want_l[a] == want_l[b]
        assert larger_blind or one_way[a] == one_way[b]
        sharp += int(one_way[a] != one_way[b])  # (the others are joined through third particles under either rule)
        lab, gs, ng = d.fof(linking_length(fc.case, h))
        if not (np.array_equal(lab, want_l) and np.array_equal(gs, want_s) and ng == want_n and lab[a] == lab[b]):
            bad.append((a, b, "larger index blind" if larger_blind else "smaller index blind",
                        int((lab != want_l).sum()), ng - want_n))
    print(f"{name} f{rb}: {len(pairs)} calls, {sum(p[2] for p in pairs)} with the larger index blind; "
          f"{len(bad)} differ from the closure, {sum(p[2] == 'larger index blind' for p in bad)} of them with the larger "
          f"index blind")
    print(f"a link pass from the larger index only would leave {sharp} of these pairs apart")
    assert sharp >= 1
    assert not bad, bad[:8]


def reversed_mirror(oracle, fc, sides, rb):
    """the first pair with the larger index blind that a link pass from the larger index only would leave apart and whose
    mirror (face_support.mirror) holds the two in the other order"""
    for a, b in sides.blind_larger:
        got = fa.mirror(oracle, fc, int(a), int(b))
        if got is None:
            continue
        m, face, off = got
        was = (a, b) if fc.on_face[a] else (b, a)
        if (was[0] < was[1]) != (face < off) and m.case.h[face] == m.case.h[off] and \
                fa.admissible(fc.case, 2.0 * float(fc.case.h[a])) and fa.admissible(m.case, 2.0 * float(m.case.h[face])):
            one_way = fof_model(fc, ("mirror", "as built", rb), fc.case.h[a])[3]
            if one_way[a] != one_way[b]:  # only this pair's own link joins the two
                return int(a), int(b), m, face, off
    return None


@pytest.mark.parametrize("rb", RBS)
def test_a_mirrored_pair_changes_its_order_in_the_arrays(oracle, rb):
    """premise of the index-dependence check: there is a pair with the larger index blind whose off-face particle, moved
    to the other side of the face, comes to lie on the other side of its partner in SFC order"""
    fc, sides = check_premise(oracle, "aniso-open", rb)
    assert reversed_mirror(oracle, fc, sides, rb) is not None


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
def test_hip_fof_does_not_depend_on_the_order_of_a_pair(hip, oracle, rb):
    """a pair whose larger index is blind, and the same cloud with the pair's order in the arrays reversed (the off-face
    particle moved to the other side of the face): in both the pair gets one label, and all labels equal the closure"""
    fc, sides = check_premise(oracle, "aniso-open", rb)
    a, b, m, face, off = reversed_mirror(oracle, fc, sides, rb)
    for what, c, p, q in (("as built", fc, a, b), ("mirrored", m, face, off)):
        h = c.case.h[p]
        want_l, want_s, want_n, _ = fof_model(c, ("mirror", what, rb), h)
        lab, gs, ng = DevCloud(hip, c.case).fof(linking_length(c.case, h))
        assert lab[p] == lab[q], (what, p, q, int(lab[p]), int(lab[q]))
        assert np.array_equal(lab, want_l) and np.array_equal(gs, want_s) and ng == want_n, what


@pytest.mark.gpu
def test_hip_fof_joins_threshold_pairs_across_two_ranks():
    """the cloud "faces" of tests/fof_mr_support.py (f64, the anisotropic open box: 600 pairs across cell faces, all 0.1
    cell edges apart up to rounding, b at the median threshold) on 2 gloo ranks through tests/fof_mr_worker.py: global
    labels, sizes and the number of groups equal the brute force over the whole cloud -- the closure wherever no pair is
    missed from both sides --, whichever rank holds which particle of a pair.  Premises: the domain's fitted limits are
    the box's, the brute force joins some pairs and leaves others apart, and joined pairs straddle the rank boundary.
    Observed on an MI355X: 509 of the 600 pairs joined, 32 of them across the boundary, 677 groups; a link pass that
    unites from the larger index only gives 710 groups here (33 pairs left apart) and fails this test"""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29971", os.path.join(root, "tests", "fof_mr_worker.py"), "faces"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=root)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("FOF_MR_RESULT ")]
    assert lines, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(lines[-1][len("FOF_MR_RESULT "):])
    print(json.dumps(res))
    assert p.returncode == 0 and res["ok"], str(res["bad"])[:3000] + p.stderr[-2000:]
    figs = res["clouds"]["faces"]
    assert res["ranks"] == 2 and figs["rounds"] == figs["model_rounds"] and all(h > 0 for h in figs["halos"])
    assert figs["pairs"] == 600 and 60 <= figs["pairs_joined"] <= 540
    assert figs["joined_across_ranks"] >= 1
