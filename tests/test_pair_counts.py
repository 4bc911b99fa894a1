"""Pair counts in radial bins (csrc/pair_counts.hip: cstone_hip_pair_counts, cstone_hip_pair_counts_cross, the domains'
calls, cstone_hip_xi_natural): DD(r) and the natural estimator of the two-point correlation function.

The reference is the numpy restatement of the rule in tests/pair_counts_support.py, the brute force over all (target,
source) pairs.  Counts are compared with ==, sums within the bound of an arbitrary order of addition derived in that module
(power-of-two weights with ==); nothing measured went into a tolerance.  Outputs are pre-filled with a sentinel and carry
PAD more entries than bins: those, and every output of a refused call, must keep it.  Every comparison asserts that the
reference's first and last bins are non-empty (the one case that is ABOUT empty bins aside), so no test compares zeros
with zeros.  Every GPU test fails at the missing symbol without the feature."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pair_counts_support as ps
import sphere_support as ss
from helpers import Box, random_cloud, real_dtype
from neighbors_support import ANISO, Case, deep_case
from oracle.oracle import HILBERT, MORTON

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cstone_hip_pair_counts", "cstone_hip_pair_counts_cross", "cstone_hip_domain_pair_counts",
               "cstone_hip_domain_pair_counts_cross", "cstone_hip_domain_mr_pair_counts",
               "cstone_hip_domain_mr_pair_counts_cross", "cstone_hip_xi_natural")
E_ARG = -1
PAD = 3
UNIT = [0, 1, 0, 1, 0, 1]
RBS = [32, 64]


def volume_edges(nb, inner, outer):
    """NB + 1 edges from inner to outer whose shells have equal volumes: a uniform cloud fills every bin alike"""
    return [(inner ** 3 + (outer ** 3 - inner ** 3) * k / nb) ** (1.0 / 3.0) for k in range(nb + 1)]


# ---- CPU -------------------------------------------------------------------------------------------------------------

def test_header_declares_and_the_bindings_export_the_calls():
    import cstone_amd
    from cstone_amd.distributed import NativeDistributedDomain
    from cstone_amd.domain import Domain

    text = open(os.path.join(ROOT, "include", "cstone_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = cstone_amd.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", code) and name in cstone_amd.EXPORTS and hasattr(lib, name), name
    assert int(re.search(r"#define CSTONE_PAIR_MAX_BINS (\d+)", code).group(1)) == cstone_amd.PAIR_MAX_BINS == ps.MAX_BINS
    for owner, method in ((cstone_amd.Context, "pair_counts"), (cstone_amd.Context, "pair_counts_cross"),
                          (Domain, "pair_counts"), (Domain, "pair_counts_cross"), (NativeDistributedDomain, "pair_counts"),
                          (NativeDistributedDomain, "pair_counts_cross"), (cstone_amd, "xi_natural")):
        assert callable(getattr(owner, method, None)), (owner, method)
    hpp = open(os.path.join(ROOT, "cornerstone-octree_amd", "include", "cstone_amd", "cstone_amd.hpp")).read()
    for name in ("pairCountsGpu", "pairCountsCrossGpu", "pairCountsGlobal", "pairCountsCrossGlobal", "xiNatural"):
        assert name in hpp, name


@pytest.mark.parametrize("rb", RBS)
def test_numpy_rule_edges_are_half_open(rb):
    """coordinates are multiples of 2^-10, every d2 is exact: a pair at exactly an inner edge goes to the outer bin, at
    exactly edges[NB] it is out; self is excluded while a coincident twin is counted iff edges[0] == 0; the ordered counts
    of a full range are even"""
    T = real_dtype(rb)
    x = np.array([0.5, 0.75, 1.0, 0.5, 0.5 + 2.0 ** -10], dtype=T)  # from particle 0: 0.25, 0.5, 0 (a twin), 2^-10
    pos = [x, np.full(5, 0.5, dtype=T), np.full(5, 0.5, dtype=T)]
    w = np.array([1.0, 2.0, 4.0, 8.0, 16.0])
    box = [0, 2, 0, 2, 0, 2]
    p = ps.auto_reference(pos, w, 0, 5, 0, 1, box, (0, 0, 0), [0.125, 0.25, 0.5])
    assert p.counts.tolist() == [0, 1] and p.sums.tolist() == [0.0, 2.0]  # 0.25 -> outer bin; 0.5 == edges[NB] is out
    p = ps.auto_reference(pos, w, 0, 5, 0, 1, box, (0, 0, 0), [0.0, 2.0 ** -10, 0.5 + 2.0 ** -10])
    assert p.counts.tolist() == [1, 3] and p.sums.tolist() == [8.0, 22.0]  # the twin in bin 0, never particle 0 itself
    p = ps.auto_reference(pos, w, 0, 5, 0, 1, box, (0, 0, 0), [2.0 ** -11, 2.0 ** -10, 0.5])
    assert p.counts.tolist() == [0, 2]  # edges[0] > 0: the twin is in no bin
    full = ps.auto_reference(pos, None, 0, 5, 0, 5, box, (0, 0, 0), [0.0, 0.2, 0.3, 1.0])
    assert (full.counts % 2 == 0).all() and int(full.counts.sum()) == 20
    # the cross counts exclude nothing: a query on particle 0 counts it and its twin at d2 = 0
    c = ps.cross_reference(pos, w, 0, 5, [[0.5, 0.5, 0.5]], None, box, (0, 0, 0), [0.0, 2.0 ** -10, 0.5 + 2.0 ** -10])
    assert c.counts.tolist() == [2, 3] and c.sums.tolist() == [9.0, 22.0]
    # targets a strict subset of the sources
    part = ps.auto_reference(pos, None, 1, 4, 2, 3, box, (0, 0, 0), [0.0, 1.0])
    assert part.counts.tolist() == [2]


@pytest.mark.parametrize("rb", RBS)
def test_numpy_rule_periodic_face(rb):
    """a pair through a periodic face is found, through an open face it is not"""
    T = real_dtype(rb)
    pos = [np.array([0.9375, 0.0625], dtype=T), np.array([0.5, 0.5], dtype=T), np.array([0.5, 0.5], dtype=T)]
    edges = [0.0625, 0.25]
    assert ps.auto_reference(pos, None, 0, 2, 0, 2, UNIT, (1, 0, 0), edges).counts.tolist() == [2]
    assert ps.auto_reference(pos, None, 0, 2, 0, 2, UNIT, (0, 1, 1), edges).counts.tolist() == [0]


def test_xi_natural_on_a_full_lattice():
    """A full cubic lattice of k^3 points with spacing a in a periodic box of edge k a: every point has 6 partners at a, 12
    at sqrt(2) a and 8 at sqrt(3) a.  With edges [a/2, 1.2 a, 1.5 a, 1.8 a] the ordered counts are n x (6, 12, 8) and
    xi_b = that / (n (n - 1) (4 pi / 3) (e1^3 - e0^3) / V) - 1 in closed form.  Roundings of one evaluation, relative to
    xi + 1: each cube carries 2 u and the difference amplifies them by (e1^3 + e0^3) / (e1^3 - e0^3) <= 3.75 here, 7.5 u;
    the subtraction, 4 pi / 3, three products and two divisions add 8 u: under 16 u, so two evaluations lie within 32 u
    of each other, whatever their order of operations.  The NaN cases too"""
    import cstone_amd

    k, a = 8, 0.125
    n, V = k ** 3, (k * a) ** 3
    pos = ps.lattice(k, a, np.float64)
    edges = [0.5 * a, 1.2 * a, 1.5 * a, 1.8 * a]
    ref = ps.auto_reference(pos, None, 0, n, 0, n, UNIT, (1, 1, 1), edges)
    assert ref.counts.tolist() == [6 * n, 12 * n, 8 * n]
    xi = cstone_amd.xi_natural(ref.counts, edges, n, n - 1, V)
    closed = np.array([c * n / (n * (n - 1) * (4 * np.pi / 3) * (e1 ** 3 - e0 ** 3) / V) - 1
                       for c, e0, e1 in zip((6, 12, 8), edges[:-1], edges[1:])])
    assert xi.dtype == np.float64 and (np.abs(xi - closed) <= 32 * 2.0 ** -53 * (np.abs(closed) + 1)).all(), (xi, closed)
    assert (np.abs(xi - ps.xi_natural(ref.counts, edges, n, n - 1, V)) <= 32 * 2.0 ** -53 * (np.abs(closed) + 1)).all()
    assert -0.2 < closed[0] < 0 < closed[1]  # (6 / 6.71 and 12 / 7.42 partners of a uniform cloud's: by hand)
    # no expected pairs: no targets, no partners; bad edges are refused (a shell of zero volume cannot be passed at all)
    assert np.isnan(cstone_amd.xi_natural([1, 2, 3], edges, 0, n - 1, V)).all()
    assert np.isnan(cstone_amd.xi_natural([1, 2, 3], edges, n, 0, V)).all()
    assert np.isnan(ps.xi_natural([1], [0.5, 0.5], n, n, V)).all()
    for bad in ([0.1, 0.1], [0.2, 0.1], [-0.1, 0.2], [0.0, float("nan")]):
        with pytest.raises(cstone_amd.CstoneError):
            cstone_amd.xi_natural([1], bad, n, n - 1, V)


_face = {}


def face_setup(oracle, rb, bc):
    """(case, targets in waves of 64, edges): tests/pair_counts_support.py, face_waves"""
    if (rb, bc) not in _face:
        x, y, z, qc, R = ps.face_waves(real_dtype(rb), ANISO, bc)
        _face[rb, bc] = (Case(oracle, x, y, z, np.zeros_like(x), Box(ANISO, bc), 16), qc, [0.0, 0.6 * R, R])
    return _face[rb, bc]


@pytest.mark.parametrize("bc", [(0, 0, 0), (1, 1, 1)])
@pytest.mark.parametrize("rb", RBS)
def test_node_test_needs_its_absolute_margin_at_cell_faces(oracle, rb, bc):
    """the restated node test on groups of targets an ulp or a few from a cell face, with partners across the face at
    distances that straddle edges[NB] by an ulp (tests/pair_counts_support.py: face_waves): with the kernel's margin no
    pair that passes the pair test lies in a pruned node; the relative term alone, 16 eps of an outer edge of 4 eps, is
    nothing beside the cancellation in |c_node - c_box| - size - size, a few ulps of the COORDINATE"""
    case, qc, edges = face_setup(oracle, rb, bc)
    pos = (case.x, case.y, case.z)
    tpos = [np.ascontiguousarray(qc[:, a]) for a in range(3)]
    ref = ps.cross_reference(pos, None, 0, case.n, qc, None, ANISO, bc, edges)
    just_out = ps.cross_reference(pos, None, 0, case.n, qc, None, ANISO, bc, [edges[-1], 1.5 * edges[-1]])
    assert ref.counts[0] > 0 and ref.counts[-1] > 0 and just_out.counts[0] > 0  # partners an ulp inside and AT the edge
    hit = ps.group_hits(pos, tpos, None, ANISO, bc, edges)
    assert hit.sum() == int(ref.counts.sum())  # (one target per wave has partners, and every pair is another particle)
    ranges, _, _ = ps.target_groups(tpos, edges, real_dtype(rb))
    assert len(ranges) > qc.shape[0] // 64  # (targets 10^-3 apart and bins of a few ulps: the waves are cut into groups)
    assert ss.particles_lost(case, ps.group_skip_table(case, tpos, edges), hit) == 0
    lost = ss.particles_lost(case, ps.group_skip_table(case, tpos, edges, absolute=False), hit)
    print(f"rb {rb} bc {bc}: relative-only margin loses {lost} of {int(hit.sum())} (group, particle) pairs")


def _compile_example(exe):
    libdir = os.path.join(ROOT, "cornerstone-octree_amd", "lib")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Wno-comment", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "cornerstone-octree_amd", "include"),
                    os.path.join(ROOT, "examples", "pair_counts_example.cpp"), "-L", libdir, "-lcstone_hip",
                    f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)


def test_cpp_example_compiles_with_a_host_compiler(tmp_path):
    """examples/pair_counts_example.cpp (Domain::pairCounts, pairCountsGpu, pairCountsCrossGpu, xiNatural)"""
    _compile_example(tmp_path / "pair_counts_example")


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


class Raw:
    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


class Setup:
    """a Case on the device; auto() / cross(): one call on sentinel-filled outputs with PAD more entries"""

    def __init__(self, hip, case, w=None):
        import cstone_amd

        self.hip, self.case, self.T = hip, case, case.x.dtype.type
        self.host = (case.x, case.y, case.z)
        self.pos = [_dev(a) for a in self.host]
        self.w_host, self.w = w, (None if w is None else _dev(w))
        self.tree = [_dev(case.o["child_offsets"]), _dev(case.o["internal_to_leaf"]), _dev(case.layout), _dev(case.cen),
                     _dev(case.siz)]
        self.cbox = cstone_amd.make_cbox(case.box.lim, case.box.bc)

    def _run(self, fn, args, out, hip, expect, stats):
        import torch

        st = (C.c_uint64 * 2)(7, 7) if stats else None
        torch.cuda.synchronize()  # (the outputs are filled on torch's stream, a second context runs on its own)
        rc = fn(*args.values(), st)
        assert rc == expect, (rc, hip.lib.cstone_hip_last_error(hip.h))
        hip.sync()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got["stats"] = None if st is None else (int(st[0]), int(st[1]))
        return got

    def _common(self, hip, w, first, last, edges):
        import torch

        import cstone_amd

        nb = len(edges) - 1
        out = dict(counts=torch.full((max(nb, 1) + PAD,), ps.SENT_COUNT, dtype=torch.int64, device="cuda"),
                   sums=torch.full((max(nb, 1) + PAD,), ps.SENT_SUM, dtype=torch.float64, device="cuda"))
        e, _ = cstone_amd.sphere_edges(edges)
        P = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        head = dict(ctx=hip.h, real_bits=self.pos[0].element_size() * 8, w_bits=64 if w is None else w.element_size() * 8,
                    x=P(self.pos[0]), y=P(self.pos[1]), z=P(self.pos[2]), w=P(w), first=first,
                    last=self.case.n if last is None else last)
        tree = dict(box=C.cast(C.byref(self.cbox), C.c_void_p), co=P(self.tree[0]), i2l=P(self.tree[1]), layout=P(self.tree[2]),
                    cen=P(self.tree[3]), siz=P(self.tree[4]))
        tail = dict(edges=e, nb=nb, counts=P(out["counts"]), sums=P(out["sums"]))
        return nb, out, head, tree, tail, P

    def auto(self, edges, first=0, last=None, t_first=None, t_last=None, w="own", hip=None, expect=0, stats=False, **override):
        hip = hip or self.hip
        w = self.w if isinstance(w, str) else w
        nb, out, head, tree, tail, _ = self._common(hip, w, first, last, edges)
        args = dict(head, t_first=head["first"] if t_first is None else t_first,
                    t_last=head["last"] if t_last is None else t_last, **tree, **tail)
        args.update(override)
        got = self._run(hip.lib.cstone_hip_pair_counts, args, out, hip, expect, stats)
        got["nb"] = nb
        return got

    def cross(self, qc, edges, qw=None, first=0, last=None, w="own", hip=None, expect=0, stats=False, num_queries=None,
              **override):
        hip = hip or self.hip
        w = self.w if isinstance(w, str) else w
        qc = np.asarray(qc, dtype=self.T).reshape(-1, 3)
        nb, out, head, tree, tail, P = self._common(hip, w, first, last, edges)
        keep = [_dev(qc if qc.size else np.zeros((1, 3), dtype=self.T)), None if qw is None else _dev(qw)]
        args = dict(head, **tree, query_centers=P(keep[0]), query_w=P(keep[1]),
                    Q=qc.shape[0] if num_queries is None else num_queries, **tail)
        args.update(override)
        got = self._run(hip.lib.cstone_hip_pair_counts_cross, args, out, hip, expect, stats)
        got["nb"] = nb
        return got

    def auto_ref(self, edges, first=0, last=None, t_first=None, t_last=None, w="own"):
        last = self.case.n if last is None else last
        return ps.auto_reference(self.host, self.w_host if isinstance(w, str) else w, first, last,
                                 first if t_first is None else t_first, last if t_last is None else t_last, self.case.box.lim,
                                 self.case.box.bc, edges)

    def cross_ref(self, qc, edges, qw=None, first=0, last=None, w="own"):
        return ps.cross_reference(self.host, self.w_host if isinstance(w, str) else w, first,
                                  self.case.n if last is None else last, qc, qw, self.case.box.lim, self.case.box.bc, edges)


def untouched(got, start=0, keys=("counts", "sums")):
    sent = dict(counts=ps.SENT_COUNT, sums=ps.SENT_SUM)
    for k in keys:
        assert (got[k][start:] == sent[k]).all(), k


def agree(got, ref, sums="bound", filled=True):
    """counts ==; sums within the bound ("bound"), == ("exact") or untouched (None); the padding keeps the sentinel"""
    nb = got["nb"]
    if filled:
        assert ref.counts[0] > 0 and ref.counts[-1] > 0, ref.counts
    assert np.array_equal(got["counts"][:nb].view(np.uint64), ref.counts), (got["counts"][:nb], ref.counts)
    if sums == "exact":
        assert got["sums"][:nb].tobytes() == ref.sums.tobytes()
    elif sums == "bound":
        err, bound = np.abs(got["sums"][:nb] - ref.sums), ref.sum_bound()
        assert (err <= bound).all(), (err, bound, ref.counts)
        assert (got["sums"][:nb][ref.counts > 0] != 0).all()
    else:
        untouched(got, keys=("sums",))
    untouched(got, start=nb)
    if got["stats"] is not None:
        assert got["stats"][1] == int(ref.counts.sum()) and got["stats"][0] >= got["stats"][1]


_clouds = {}
N_CLOUD = 3000


def cloud_setup(hip, oracle, kind, rb, bc, curve=HILBERT, kb=64, bucket=16, n=N_CLOUD, wbits=64):
    key = (kind, rb, bc, curve, kb, bucket, n, wbits)
    if key not in _clouds:
        box = Box(ANISO, bc)
        x, y, z = random_cloud(n, box, rb, 5 + rb, kind)
        case = Case(oracle, x, y, z, np.zeros_like(x), box, bucket, curve=curve, kb=kb)
        _clouds[key] = Setup(hip, case, ps.weights(n, wbits, 6))
    return _clouds[key]


# boundary conditions x (type, curve, key width): both real types, both key widths and both curves meet every box
AUTO_CASES = [(kind, bc, rb, curve, kb)
              for kind in ("uniform", "clustered")
              for bc, combos in (((0, 0, 0), ((32, HILBERT, 32), (64, MORTON, 64))),
                                 ((1, 1, 1), ((32, MORTON, 64), (64, HILBERT, 32))),
                                 ((1, 0, 1), ((32, HILBERT, 64), (64, MORTON, 32))))
              for rb, curve, kb in combos]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,bc,rb,curve,kb", AUTO_CASES)
def test_hip_auto_counts_equal_the_brute_force(hip, oracle, kind, bc, rb, curve, kb):
    """3 000 particles in the anisotropic box, bucket 16, uniform and clustered, open, periodic and mixed; NB = 1, 16, 64
    with shells of equal volume out to 0.3 (under half of the shortest periodic edge, 0.35); without weights, with float32
    and float64 ones and with powers of two (==); stats[1] == the total of the counts"""
    s = cloud_setup(hip, oracle, kind, rb, bc, curve, kb)
    n = s.case.n
    w32, w2 = ps.weights(n, 32, 7), ps.pow2_weights(n, 8)
    agree(s.auto(volume_edges(1, 0.0, 0.3), w=None, stats=True), s.auto_ref(volume_edges(1, 0.0, 0.3), w=None), sums=None)
    e16 = volume_edges(16, 0.01, 0.3)
    agree(s.auto(e16, w=_dev(w32), stats=True), s.auto_ref(e16, w=w32))
    agree(s.auto(e16, w=_dev(w2)), s.auto_ref(e16, w=w2), sums="exact")
    e64 = volume_edges(64, 0.0, 0.3)
    agree(s.auto(e64, stats=True), s.auto_ref(e64))


@pytest.mark.gpu
@pytest.mark.parametrize("bc", [(0, 0, 0), (1, 1, 1)])
@pytest.mark.parametrize("rb", RBS)
def test_hip_cross_counts_at_cell_faces(hip, oracle, rb, bc):
    """targets a few ulps from cell faces (and, periodic, from the faces of the box), partners across the face one ulp
    inside the outer edge and exactly at it: == the brute force.  This pins the margin of the node test;
    test_node_test_needs_its_absolute_margin_at_cell_faces shows on the restated node test what a relative-only margin
    loses here.  The particles themselves as targets of the auto counts, with the same edges, too"""
    case, qc, edges = face_setup(oracle, rb, bc)
    s = Setup(hip, case, ps.weights(case.n, 64, 9))
    agree(s.cross(qc, edges, stats=True), s.cross_ref(qc, edges))
    agree(s.auto(edges, w=None), s.auto_ref(edges, w=None), sums=None, filled=False)


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
def test_hip_target_ranges(hip, oracle, rb):
    """t_first no multiple of 64, 1, 63, 64 and 65 targets, targets a strict subset of the sources (which must matter: the
    reference differs from the call with sources == targets), sources that cut leaves at both ends, an empty target range"""
    s = cloud_setup(hip, oracle, "uniform", rb, (1, 0, 1))  # (uniform: no 64 targets are a blob with all their partners)
    n = s.case.n
    edges = volume_edges(16, 0.0, 0.3)
    for t_first, num in ((37, 1), (37, 63), (100, 64), (1001, 65), (n - 65, 65)):
        wide = s.auto_ref(edges, 0, n, t_first, t_first + num)
        narrow = s.auto_ref(edges, t_first, t_first + num, t_first, t_first + num)
        assert not np.array_equal(wide.counts, narrow.counts)
        agree(s.auto(edges, 0, n, t_first, t_first + num, stats=True), wide, filled=num > 1)  # (one target fills few bins)
        agree(s.auto(edges, t_first, t_first + num, t_first, t_first + num), narrow, filled=False)
    lay = s.case.layout.astype(np.int64)
    split = np.flatnonzero(np.diff(lay) >= 2)  # leaves of two particles or more: cut behind their first particle
    first, last = int(lay[split[3]]) + 1, int(lay[split[-3]]) + 1
    assert first not in s.case.layout and last not in s.case.layout and 0 < first < last < n
    agree(s.auto(edges, first, last, first + 70, last - 70), s.auto_ref(edges, first, last, first + 70, last - 70))
    got = s.auto(edges, 0, n, 100, 100, stats=True)
    assert (got["counts"][:16] == 0).all() and (got["sums"][:16] == 0).all() and got["stats"] == (0, 0)
    untouched(got, start=16)


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
def test_hip_shapes_of_the_walk(hip, oracle, rb):
    """a one-leaf tree; leaves of more than 64 particles (bucket 128); the deepest tree a 64-bit Morton key allows, with
    coincident particles; an open box with edges[NB] beyond its diagonal -- every pair is counted, the total is
    n_t (n - 1), every node is opened: the stack's worst case; edges[NB] below the smallest separation: all zeros"""
    T = real_dtype(rb)
    x, y, z = random_cloud(40, Box(UNIT), rb, 31, "uniform")
    one = Setup(hip, Case(oracle, x, y, z, np.zeros_like(x), Box(UNIT), 64), ps.weights(40, 64, 9))
    assert one.case.o["num_nodes"] == 1
    agree(one.auto(volume_edges(4, 0.0, 0.6)), one.auto_ref(volume_edges(4, 0.0, 0.6)))

    big = cloud_setup(hip, oracle, "clustered", rb, (1, 1, 1), bucket=128, n=2000)
    assert big.case.leaf_counts.max() > 64
    agree(big.auto(volume_edges(16, 0.0, 0.3)), big.auto_ref(volume_edges(16, 0.0, 0.3)))

    from helpers import max_level

    deep = Setup(hip, deep_case(oracle, rb, 21), None)
    n = deep.case.n
    assert int(deep.case.o["level_range"][max_level(64)]) < int(deep.case.o["level_range"][max_level(64) + 1])  # level 21 exists
    w2 = ps.pow2_weights(n, 10)
    edges = [0.0, 2.0 ** -30, 2.0 ** -8, 0.25, 2.0]  # 2 > sqrt(3), the diagonal of the unit box
    ref = deep.auto_ref(edges, w=w2)
    assert int(ref.counts.sum()) == n * (n - 1) and int(ref.counts[0]) == n  # every particle has one twin, at d2 = 0
    agree(deep.auto(edges, w=_dev(w2), stats=True), ref, sums="exact")
    ref = deep.auto_ref(edges, 0, n, 37, 137, w=None)
    assert int(ref.counts.sum()) == 100 * (n - 1)
    agree(deep.auto(edges, 0, n, 37, 137, w=None), ref, sums=None)
    got = deep.auto([2.0 ** -40, 2.0 ** -30], w=None)  # edges[0] > 0: the twins are in no bin
    assert deep.auto_ref([2.0 ** -40, 2.0 ** -30], w=None).counts.tolist() == [0] and got["counts"][0] == 0

    full = cloud_setup(hip, oracle, "uniform", rb, (0, 0, 0), n=1500)
    n = full.case.n
    diag = float(np.sqrt(3.4 ** 2 + 0.7 ** 2 + 12.0 ** 2))
    edges = [0.0, 1.0, 4.0, 1.01 * diag]
    ref = full.auto_ref(edges, w=None)
    assert int(ref.counts.sum()) == n * (n - 1)
    got = full.auto(edges, w=None, stats=True)
    agree(got, ref, sums=None)
    assert got["stats"] == (n * n, n * (n - 1))  # every leaf opened for every wave, every particle tested

    k, a = 10, 1.0 / 16
    lat = ps.lattice(k, a, T)
    ls = Setup(hip, Case(oracle, *lat, np.zeros_like(lat[0]), Box(UNIT), 16), None)
    edges = [0.0, 0.25 * a, 0.5 * a, 0.999 * a]
    assert ls.auto_ref(edges).counts.tolist() == [0, 0, 0]
    got = ls.auto(edges)
    assert (got["counts"][:3] == 0).all()
    untouched(got, start=3)
    agree(ls.auto([0.0, 0.5 * a, 1.001 * a]), ls.auto_ref([0.0, 0.5 * a, 1.001 * a]), sums=None, filled=False)
    assert ls.auto_ref([0.0, 0.5 * a, 1.001 * a]).counts.tolist() == [0, 6 * k ** 3 - 6 * k * k]


@pytest.mark.gpu
def test_hip_bits_are_the_same_in_every_run_and_on_every_context(hip, oracle):
    """two calls back to back, a call after an unrelated call on the stream and a call on a second context with a stream
    of its own give byte-equal sums and counts; 32-bit weights give the bits of the 64-bit call on the same values"""
    import torch

    import cstone_amd

    s = cloud_setup(hip, oracle, "clustered", 64, (1, 0, 1))
    edges = volume_edges(64, 0.0, 0.3)
    qc = np.stack([a[::7] for a in s.host], axis=1)
    qw = ps.weights(qc.shape[0], 64, 11)
    a, b = s.auto(edges), s.auto(edges)
    ca, cb = s.cross(qc, edges, qw), s.cross(qc, edges, qw)
    hip.sequence(torch.zeros(5000, dtype=torch.int32, device="cuda"), 3)
    c = s.auto(edges)
    other = cstone_amd.Context(0, use_torch_stream=False)
    try:
        d, cd = s.auto(edges, hip=other), s.cross(qc, edges, qw, hip=other)
    finally:
        other.close()
    for k in ("counts", "sums"):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes() == d[k].tobytes(), k
        assert ca[k].tobytes() == cb[k].tobytes() == cd[k].tobytes(), k
    agree(a, s.auto_ref(edges))
    agree(ca, s.cross_ref(qc, edges, qw))
    w32 = ps.weights(s.case.n, 32, 12)
    narrow, wide = s.auto(edges, w=_dev(w32)), s.auto(edges, w=_dev(w32.astype(np.float64)))
    assert narrow["sums"].tobytes() == wide["sums"].tobytes() and narrow["counts"].tobytes() == wide["counts"].tobytes()
    agree(narrow, s.auto_ref(edges, w=w32))


BAD_EDGES = ([0.5], [0.0] + [0.001 * k for k in range(1, 66)], [0.0, np.nan], [0.0, np.inf], [-0.1, 0.2], [0.0, 0.2, 0.2],
             [0.0, 0.25, 0.2], [0.0, 0.5 * (ANISO[3] - ANISO[2])], [0.0, 0.36])  # (half of the periodic y edge, and above)


@pytest.mark.gpu
def test_hip_refusals_write_nothing_and_leave_the_context_usable(hip, oracle):
    s = cloud_setup(hip, oracle, "clustered", 64, (1, 1, 1))
    n = s.case.n
    edges = volume_edges(4, 0.0, 0.3)
    qc = np.asarray([[0.0, 0.5, 0.0]] * 4)
    null = C.c_void_p(0)
    common = (dict(x=null), dict(z=null), dict(counts=null), dict(sums=null), dict(box=null), dict(co=null), dict(siz=null),
              dict(real_bits=16), dict(w_bits=16), dict(first=10, last=9))
    for override in common + (dict(t_first=10, t_last=9), dict(first=5, t_first=4), dict(t_last=n + 1), dict(last=n - 1, t_last=n)):
        untouched(s.auto(edges, expect=E_ARG, stats=True, **override))
    for override in common + (dict(query_centers=null),):
        untouched(s.cross(qc, edges, expect=E_ARG, stats=True, **override))
    untouched(s.cross(qc, edges, qw=ps.weights(4, 64, 1), w=None, expect=E_ARG))  # a query_w without a w
    for bad in BAD_EDGES:
        untouched(s.auto(bad, expect=E_ARG))
        untouched(s.cross(qc, bad, expect=E_ARG))
    under = [0.0, float(np.nextafter(0.5 * (ANISO[3] - ANISO[2]), 0))]  # one ulp under half the edge: taken
    assert np.array_equal(s.auto(under, w=None)["counts"][:1].view(np.uint64), s.auto_ref(under, w=None).counts)
    # a w_bits nobody reads is not looked at; no queries and an empty source range are fine and zero the outputs
    agree(s.auto(edges, w=None, w_bits=16), s.auto_ref(edges, w=None), sums=None)
    for got in (s.cross(qc, edges, num_queries=0, stats=True), s.cross(qc, edges, first=7, last=7, stats=True)):
        assert (got["counts"][:4] == 0).all() and (got["sums"][:4] == 0).all() and got["stats"] == (0, 0)
        untouched(got, start=4)
    hip.sync()
    agree(s.auto(edges), s.auto_ref(edges))


def cross_queries(s, Q, seed):
    """Q centres in a shuffled order: a third ON particles (counted at d2 = 0), a third at random points of the box, a
    third outside the cloud's extent on the open axes"""
    T = s.T
    if Q < 3:
        return np.stack([a[:Q] for a in s.host], axis=1).astype(T)
    qc = ss.mixed_queries(s.host, s.case.box.lim, s.case.box.bc, Q, seed, T)
    return qc[np.random.default_rng(seed + 1).permutation(Q)]


CROSS_CASES = [("uniform", (0, 0, 0), 32), ("clustered", (0, 0, 0), 64), ("uniform", (1, 1, 1), 64), ("clustered", (1, 1, 1), 32),
               ("uniform", (1, 0, 1), 32), ("clustered", (1, 0, 1), 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,bc,rb", CROSS_CASES)
def test_hip_cross_counts_equal_the_brute_force_and_the_sphere_profiles(hip, oracle, kind, bc, rb):
    """Q = 1, 63, 64, 65, 1 000 queries in a shuffled order, some outside an open box, some on particles: counts == the
    brute force, == for a second permutation of the queries, and == the column sums of cstone_hip_sphere_profiles for the
    same centres at scale 1 -- there e_b = T(1) * T(edges[b]) = T(edges[b]) exactly, so the two rules agree for ALL edges
    and every bin is compared.  Sums with query weights within the bound, with powers of two =="""
    s = cloud_setup(hip, oracle, kind, rb, bc)
    n = s.case.n
    tree = dict(child_offsets=s.tree[0], internal_to_leaf=s.tree[1])
    for Q, nb in ((1, 4), (63, 16), (64, 1), (65, 64), (1000, 16)):
        edges = volume_edges(nb, 0.0 if Q % 2 else 0.01, 0.3)
        qc = cross_queries(s, Q, 20 + Q)
        qw = ps.weights(Q, 64, 21)
        ref = s.cross_ref(qc, edges, qw)
        got = s.cross(qc, edges, qw, stats=True)
        agree(got, ref, filled=Q > 1)
        perm = np.random.default_rng(22).permutation(Q)
        again = s.cross(qc[perm], edges, qw[perm])
        assert again["counts"].tobytes() == got["counts"].tobytes()
        prof, _, flags = hip.sphere_profiles(*s.pos, None, 0, n, s.cbox, tree, s.tree[2], s.tree[3], s.tree[4], _dev(qc), edges)
        hip.sync()
        assert not flags.cpu().numpy().any()
        assert np.array_equal(prof.cpu().numpy().sum(axis=0).view(np.uint64), ref.counts)
    qc = cross_queries(s, 200, 23)
    edges = volume_edges(16, 0.0, 0.3)
    w2, qw2 = ps.pow2_weights(n, 24), ps.pow2_weights(200, 25)
    agree(s.cross(qc, edges, qw2, w=_dev(w2)), s.cross_ref(qc, edges, qw2, w=w2), sums="exact")
    agree(s.cross(qc, edges, None, w=_dev(w2)), s.cross_ref(qc, edges, None, w=w2), sums="exact")  # no query_w: 1
    agree(s.cross(qc, edges, None, w=None), s.cross_ref(qc, edges, None, w=None), sums=None)
    agree(s.cross(qc, edges, qw2, 100, n - 100, w=_dev(w2)), s.cross_ref(qc, edges, qw2, 100, n - 100, w=w2), sums="exact")


@pytest.mark.gpu
@pytest.mark.parametrize("rb", RBS)
def test_hip_domain_pair_counts_equal_the_calls_on_the_view(hip, oracle, rb):
    """Domain.pair_counts and Domain.pair_counts_cross after a sync == Context.pair_counts / pair_counts_cross on the
    view's arrays, bit for bit, and == the brute force on the synced arrays; before the first sync they are refused"""
    import torch

    import cstone_amd
    from cstone_amd.domain import Domain

    T = real_dtype(rb)
    tdt = torch.float32 if rb == 32 else torch.float64
    n = 4000
    box = Box(UNIT, (1, 1, 0))
    hx, hy, hz = random_cloud(n, box, rb, 43, "clustered")
    x, y, z = [torch.from_numpy(a.copy()).cuda() for a in (hx, hy, hz)]
    h = torch.full((n,), 0.01, dtype=tdt, device="cuda")
    w = torch.from_numpy(ps.weights(n, 64, 44)).cuda()
    dom = Domain(hip, cstone_amd.HILBERT, 64, rb, 64, 16, 0.5, cstone_amd.make_cbox(box.lim, box.bc))
    rng = np.random.default_rng(45)
    qc = torch.from_numpy(rng.uniform(0, 1, (300, 3)).astype(T)).cuda()
    qw = torch.from_numpy(ps.weights(300, 64, 46)).cuda()
    edges = volume_edges(12, 0.0, 0.2)
    with pytest.raises(cstone_amd.CstoneError):
        dom.pair_counts(x, y, z, w, edges)
    with pytest.raises(cstone_amd.CstoneError):
        dom.pair_counts_cross(x, y, z, w, qc, edges, qw)
    keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    scratch = [torch.empty(n, dtype=tdt, device="cuda") for _ in range(3)]
    keys, x, y, z, h, _, _ = dom.sync(keys, x, y, z, h, scratch)
    w = dom.reapply_sync(w)
    hip.sync()
    v = dom.view()
    assert (v.start_index, v.end_index, v.num_particles_with_halos) == (0, n, n)
    tree = dict(child_offsets=Raw(v.child_offsets), internal_to_leaf=Raw(v.internal_to_leaf))
    pos = [a.cpu().numpy() for a in (x, y, z)]

    counts, sums, stats = dom.pair_counts(x, y, z, w, edges, with_stats=True)
    c2, s2, st2 = hip.pair_counts(x, y, z, w, 0, n, v.box, tree, Raw(v.layout), Raw(v.centers), Raw(v.sizes), edges,
                                  with_stats=True)
    hip.sync()
    assert torch.equal(counts, c2) and sums.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes() and stats == st2
    ref = ps.auto_reference(pos, w.cpu().numpy(), 0, n, 0, n, list(v.box.lim), tuple(v.box.bc), edges)
    assert np.array_equal(counts.cpu().numpy().view(np.uint64), ref.counts) and ref.counts[0] > 0 and ref.counts[-1] > 0
    assert (np.abs(sums.cpu().numpy() - ref.sums) <= ref.sum_bound()).all() and stats[1] == int(ref.counts.sum())

    counts, sums, stats = dom.pair_counts_cross(x, y, z, w, qc, edges, qw, with_stats=True)
    c2, s2, st2 = hip.pair_counts_cross(x, y, z, w, 0, n, v.box, tree, Raw(v.layout), Raw(v.centers), Raw(v.sizes), qc, edges,
                                        query_w=qw, with_stats=True)
    hip.sync()
    assert torch.equal(counts, c2) and sums.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes() and stats == st2
    ref = ps.cross_reference(pos, w.cpu().numpy(), 0, n, qc.cpu().numpy(), qw.cpu().numpy(), list(v.box.lim), tuple(v.box.bc),
                             edges)
    assert np.array_equal(counts.cpu().numpy().view(np.uint64), ref.counts) and ref.counts[0] > 0 and ref.counts[-1] > 0
    assert (np.abs(sums.cpu().numpy() - ref.sums) <= ref.sum_bound()).all()
    # xi of the counts through the bindings: the clustered cloud is clustered
    xi = cstone_amd.xi_natural(dom.pair_counts(x, y, z, None, edges)[0].cpu().numpy(), edges, n, n - 1, 1.0)
    assert xi[0] > 1.0


@pytest.mark.gpu
def test_hip_cpp_example_runs_and_a_uniform_cloud_has_no_correlation(tmp_path):
    """examples/pair_counts_example.cpp: exit status 0 (it compares Domain::pairCounts with pairCountsGpu on the domain's
    octree bit for bit, and the cross counts about the particles themselves with the auto counts plus the selves).  Its
    uniform cloud: the ordered count of a bin is twice the unordered one, which is Poisson with mean E / 2 for E expected
    ordered pairs, so xi_b = DD_b / E - 1 has the standard deviation sqrt(2 / E); the bound |xi_b| <= 5 / sqrt(E) is 3.5 of
    them, asserted on the bins with E >= 10^4.  The seed is fixed in the example"""
    exe = tmp_path / "pair_counts_example"
    _compile_example(exe)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "identical" in p.stdout
    rows = re.findall(r"^bin\s+(\d+)\s+\[\s*(\S+),\s*(\S+)\)\s+xi_clustered\s+(\S+)\s+xi_uniform\s+(\S+)\s+expected\s+(\S+)$",
                      p.stdout, flags=re.M)
    assert len(rows) >= 8
    checked = 0
    for _, _, _, xc, xu, expected in rows:
        if float(expected) >= 1.0e4:
            checked += 1
            assert abs(float(xu)) <= 5.0 / np.sqrt(float(expected)), (xu, expected)
    assert checked >= 4 and float(rows[0][3]) > 1.0  # and the clustered cloud is clustered at small r
