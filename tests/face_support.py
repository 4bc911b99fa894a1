"""Clouds and the model of tests/test_face_pairs.py (host side only: numpy and plain Python).

The neighbour walk makes two floating-point tests: the node test (|c - x_i| - size, folded, right-folded squares,
< 4 h^2 ext^2) and the pair test (dx^2 + dy^2 + dz^2 < 4 h^2).  For a particle ON a cell face whose partner lies at a
distance within one ulp of the search radius the two can disagree: the pair test passes, but the node test of the partner's
leaf, or of one of its ancestors, fails by a rounding, and the walk never gets to the pair test.  The clouds here consist
of nothing but such pairs; the model says, from the two tables of tests/neighbors_support.py alone, which of them the walk
reports from which side."""
import numpy as np

import fof_support as fs
from helpers import Box, real_dtype
from neighbors_support import ANISO, Case
from oracle.oracle import HILBERT

UNIT = [0, 1, 0, 1, 0, 1]
# In the unit box every face and every node centre is a binary fraction, and c - x_j is exact whenever x_j lies within a
# factor of two of c: a pair can only be one-sided where the off-face particle lies in the lowest cells of its axis.  The
# unit shapes therefore take the face k = 1 only (all seven faces gave 2 + 3 one-sided pairs in 600).
SHAPES = {  # name: (box limits, boundary conditions, the faces k to draw from or None for all)
    "aniso-open": (ANISO, (0, 0, 0), None),
    "aniso-pbc": (ANISO, (1, 1, 1), None),
    "unit-open": (UNIT, (0, 0, 0), (1,)),
    "unit-pbc": (UNIT, (1, 1, 1), (1,)),
}
N_FACE, LEVEL, BUCKET = 1200, 3, 16


def face_cloud(T, lim, bc, axis_mix=True, n=N_FACE, level=LEVEL, seed=31, faces=None, edge_every=4, shift=(0.05, 1.2)):
    """(x, y, z, partner, axis) of n // 2 pairs: particle 2p lies ON a face of a cell of `level`, at
    lo + T(k) * (len / T(2^level)) with k drawn from `faces` (default 1 .. 2^level - 1) along its axis and at random
    along the other two; particle 2p + 1, its partner, has the same two other coordinates and is displaced along the
    axis by +-U(*shift) cell edges, shift = (0.05, 1.2) by default (wrapped on a periodic axis, turned round on an open one if it would leave the
    box).  partner[k] is the index of k's partner, axis[k] the displacement axis of k's pair.

    With axis_mix the axis cycles through x, y, z; without, it is x.  What y and z give: in the anisotropic box the three
    edges and origins differ (3.4 from -1.3, 0.7 from 0.2, 12 from -5), so each axis rounds lo + k * edge and c - x_i
    differently, and with 64-bit Hilbert keys a face normal to y or z separates other pairs of leaves and ancestors than
    one normal to x: pairs are pruned by the node test of an ANCESTOR there that x alone reaches rarely, and both
    orientations of the one-sidedness get their share in every box.  In the unit box the faces are binary fractions on
    every axis and few pairs are one-sided on any of them; three axes bring the count over the bar that x alone misses.

    Every edge_every-th pair is an EDGE pair (0: none): its first particle lies on a face of the next axis as well, i.e.
    on an edge of its cell, and the partner is displaced along both axes.  A pair displaced along one axis has the other
    two terms of every node test on its path at exactly 0 (the partner's leaf and its ancestors contain the target's
    other two coordinates), so the SUM of the node test never rounds there and a fused multiply-add in it would go
    unnoticed; across an edge two terms are non-zero and a contraction of dx * dx + (dy * dy + dz * dz) changes which
    pairs are dropped (test_a_fused_node_test_drops_other_pairs)."""
    rng = np.random.default_rng(seed)
    m, cells = n // 2, 2 ** level
    limT = np.array(lim).astype(T)
    lo, hi = limT[0::2], limT[1::2]
    edge = (hi - lo) / T(cells)
    axis = (np.arange(m) % 3) if axis_mix else np.zeros(m, dtype=np.int64)
    pick = np.arange(1, cells) if faces is None else np.array(faces)
    k, k2 = rng.choice(pick, m), rng.choice(pick, m)
    lo_s, hi_s = shift
    shift = rng.uniform(lo_s, hi_s, m) * rng.choice([-1.0, 1.0], m)
    shift2 = rng.uniform(lo_s, hi_s, m) * rng.choice([-1.0, 1.0], m)
    p = np.stack([(lo[d] + (hi[d] - lo[d]) * rng.uniform(0.02, 0.98, m).astype(T)).astype(T) for d in range(3)], axis=1)
    q = p.copy()

    def place(t, a, face, by):
        """particle t onto face `face` of axis a, its partner `by` cell edges from it"""
        p[t, a] = lo[a] + T(face) * edge[a]
        v = p[t, a] + T(by) * edge[a]
        if not lo[a] < v < hi[a]:
            if int(bc[a]) == 1:
                v = v + (hi[a] - lo[a]) if v <= lo[a] else v - (hi[a] - lo[a])
            else:
                v = p[t, a] - T(by) * edge[a]
        q[t, a] = v

    for t in range(m):
        place(t, axis[t], k[t], shift[t])
        if edge_every and t % edge_every == edge_every - 1:
            place(t, (axis[t] + 1) % 3, k2[t], shift2[t])
    assert p.dtype == T and q.dtype == T
    pts = np.empty((2 * m, 3), dtype=T)
    pts[0::2], pts[1::2] = p, q
    partner = np.arange(2 * m) ^ 1
    x, y, z = [np.ascontiguousarray(pts[:, d]) for d in range(3)]
    return x, y, z, partner, np.repeat(axis, 2)


class FaceCase:
    """a face cloud in SFC order: case (neighbors_support.Case; case.h[i] is the threshold h of i's partner), partner and
    axis per particle in that order"""

    def __init__(self, oracle, x, y, z, partner, axis, box, bucket=BUCKET, on_face=None):
        keys = oracle.compute_sfc_keys(HILBERT, 64, x, y, z, box)
        _, order = oracle.sort_pairs(keys, np.arange(x.size))
        order = np.asarray(order).astype(np.int64)
        self.case = Case(oracle, x, y, z, np.zeros_like(x), box, bucket)
        assert np.array_equal(self.case.x, x[order]) and np.array_equal(self.case.z, z[order])
        rank = np.empty(x.size, dtype=np.int64)
        rank[order] = np.arange(x.size)
        self.partner = rank[partner[order]]
        self.axis = axis[order]
        self.on_face = (np.arange(x.size) % 2 == 0 if on_face is None else on_face)[order]  # face_cloud: the even ones
        idx = np.arange(x.size)
        assert np.array_equal(self.partner[self.partner], idx)
        self.case.h = threshold_h(self.case, idx, self.partner)
        self.case._pairs, self.case._nodes = None, {}
        self._rel = None

    @property
    def n(self):
        return self.case.n


def _d2(case, i, j, h):
    """d2 of the pairs (i[k], j[k]) as the walk of target i[k] evaluates it at h[k]: the fold is used when the +-2h cube
    of the target leaves the box and an axis is periodic"""
    T = case.x.dtype.type
    lim = case.box.lim.astype(T)
    lo, hi = lim[0::2], lim[1::2]
    ln = hi - lo
    inv = T(1) / ln
    P = (case.x, case.y, case.z)
    periodic = [int(b) == 1 for b in case.box.bc]
    s = T(2) * h
    inside = np.ones(i.size, dtype=bool)
    for d in range(3):
        inside &= (P[d][i] - s >= lo[d]) & (P[d][i] + s <= hi[d])
    use = (~inside) & any(periodic)
    d2 = None
    for d in range(3):
        dx = P[d][j] - P[d][i]
        if periodic[d]:
            dx = np.where(use, dx - ln[d] * np.rint(dx * inv[d]), dx)
        sq = dx * dx
        d2 = sq if d2 is None else d2 + sq
    assert d2.dtype == case.x.dtype
    return d2


def _smallest_h(T, d2):
    """the smallest h in T with d2 < T(4) * h * h (the rounded product is monotone in h)"""
    ok = lambda h: d2 < T(4) * h * h  # noqa: E731
    h = (np.sqrt(d2) * T(0.5)).astype(T)
    for _ in range(4):
        h = np.where(ok(h), h, np.nextafter(h, T(np.inf)))
    for _ in range(4):
        down = np.nextafter(h, T(0))
        h = np.where(ok(down), down, h)
    assert ok(h).all() and not ok(np.nextafter(h, T(0))).any()
    return h.astype(T)


def threshold_h(case, i, j):
    """the smallest h in T with d2(i, j) < T(4) * h * h, d2 evaluated as the walk of target i evaluates it, fold included.
    Whether the fold is used depends on the +-2h cube of target i: iterated until h is stable.  i, j: index arrays"""
    T = case.x.dtype.type
    i, j = np.atleast_1d(np.asarray(i, dtype=np.int64)), np.atleast_1d(np.asarray(j, dtype=np.int64))
    h = _smallest_h(T, _d2(case, i, j, np.zeros(i.size, dtype=T)))
    for _ in range(6):
        new = _smallest_h(T, _d2(case, i, j, h))
        if np.array_equal(new, h):
            return h
        h = new
    raise AssertionError("threshold_h: the fold decision does not settle")


def leaf_nodes(case):
    """node_of[j]: the node of the linked octree that is the leaf of particle j"""
    o = case.o
    nodes = np.flatnonzero(o["child_offsets"][:o["num_nodes"]] == 0)
    node_of_leaf = np.empty(o["num_leaves"], dtype=np.int64)
    node_of_leaf[o["internal_to_leaf"][nodes]] = nodes
    leaf = np.searchsorted(case.layout, np.arange(case.n), side="right") - 1
    return node_of_leaf[leaf]


def path_table(case, ov):
    """ok[i, node]: node and every ancestor of it pass the node test of target i.  The parent of node c is
    parents[(c - 1) // 8]; nodes are stored level by level, so a parent comes before its children"""
    o = case.o
    nn = o["num_nodes"]
    ok = np.zeros((case.n, nn), dtype=bool)
    ok[:, 0] = ov[:, 0]
    if nn > 1:
        parent = np.asarray(o["parents"])[(np.arange(1, nn) - 1) // 8]
        assert (parent < np.arange(1, nn)).all()
        for c in range(1, nn):
            ok[:, c] = ov[:, c] & ok[:, parent[c - 1]]
    return ok


def relation_from(case, ov):
    return case.pair_table() & path_table(case, ov)[:, leaf_nodes(case)]


def walk_relation(case):
    """rel[i, j] = pair_table[i, j] and every node on the path from j's leaf to the root passes node_table[i, node]: what
    the walk of target i reports, as a matrix"""
    return relation_from(case, case.node_table())


def node_table_fused(case):
    """the MUTANT of Case.node_table (ext = 1) for float32: every a * b + c rounded once, as a fused multiply-add would
    -- the fold dx - len * rint(dx * inv) and the sum dx * dx + (dy * dy + dz * dz) = fma(dx, dx, fma(dy, dy, dz * dz)).
    Products of two float32 are exact in float64; the sum is rounded to float64 and then to float32 (a second rounding
    that matters for one sum in 2^29)"""
    T, P, ln, inv, periodic, use = case._fold_setup()
    assert T is np.float32
    f64 = np.float64
    cell = T(4) * case.h * case.h
    half = []
    for d in range(3):
        dx = case.cen[:, d][None, :] - P[d][:, None]
        if periodic[d]:
            folded = (dx.astype(f64) - f64(ln[d]) * np.rint(dx * inv[d]).astype(f64)).astype(T)
            dx = np.where(use[:, None], folded, dx)
        dx = np.abs(dx) - case.siz[:, d][None, :]
        dx = dx + np.abs(dx)
        half.append(dx * T(0.5))
    zz = half[2] * half[2]
    inner = (half[1].astype(f64) * half[1].astype(f64) + zz.astype(f64)).astype(T)
    outer = (half[0].astype(f64) * half[0].astype(f64) + inner.astype(f64)).astype(T)
    return outer < cell[:, None]


def closure_labels(rel, first, last):
    """min_labels of tests/fof_support.py over rel | rel.T restricted to the targets [first, last)"""
    sym = rel | rel.T
    sym[:first] = False
    sym[last:] = False
    sym[:, :first] = False
    sym[:, last:] = False
    return fs.labels_of(sym, first, last)


def larger_only_labels(rel, first, last):
    """the labels of a link pass that unites only from the LARGER index (rel[i, j] with j < i, as the kernel once did):
    used to pick the pairs on which that rule and the closure differ -- a one-sided pair can still be joined through
    third particles"""
    return closure_labels(np.tril(rel), first, last)


class Sides:
    """the constructed pairs (a, b), a < b, that lie in different leaves and have one threshold from both sides, by what
    the walk makes of them: seen from both sides, larger index blind (a reports b, b does not report a), smaller index
    blind, missed from both sides.  Each an array [k, 2]"""

    def __init__(self, both, blind_larger, blind_smaller, neither):
        self.both, self.blind_larger, self.blind_smaller, self.neither = both, blind_larger, blind_smaller, neither


def threshold_pairs(fc):
    """the pairs (a, b), a < b = partner[a], in different leaves, with h[a] == h[b]"""
    case = fc.case
    a = np.flatnonzero(np.arange(fc.n) < fc.partner)
    b = fc.partner[a]
    node = leaf_nodes(case)
    keep = (node[a] != node[b]) & (case.h[a] == case.h[b])
    return a[keep], b[keep]


def one_sided(fc, rel=None):
    """Sides of the threshold pairs under rel (default: walk_relation of the case)"""
    if rel is None:
        if fc._rel is None:
            fc._rel = walk_relation(fc.case)
        rel = fc._rel
    a, b = threshold_pairs(fc)
    ab, ba = rel[a, b], rel[b, a]
    pick = lambda m: np.stack([a[m], b[m]], axis=1)  # noqa: E731
    return Sides(pick(ab & ba), pick(ab & ~ba), pick(~ab & ba), pick(~ab & ~ba))


def uniform_case(case, h):
    """the same cloud and tree with one h for every particle (what friends-of-friends walks at b = 2 h)"""
    c = Case.__new__(Case)
    c.__dict__.update(case.__dict__)
    c.h = np.full(case.n, h, dtype=case.x.dtype)
    c._pairs, c._nodes = None, {}
    return c


def admissible(case, b):
    """cstone_hip_friends_of_friends takes b: below half of every periodic edge"""
    lim = case.box.lim
    return all(int(case.box.bc[d]) != 1 or b < 0.5 * (lim[2 * d + 1] - lim[2 * d]) for d in range(3))


def mirror(oracle, fc, a, b):
    """the cloud of fc with the off-face particle of the pair (a, b) moved to the other side of its face, at the same
    distance up to rounding: (FaceCase, index of the face particle, index of the moved one) or None if the moved particle
    would leave the box.  For pairs that are not wrapped round a periodic edge (the open shapes)"""
    case = fc.case
    T = case.x.dtype.type
    d = int(fc.axis[a])
    P = [case.x.copy(), case.y.copy(), case.z.copy()]
    lim = case.box.lim.astype(T)
    face, off = (a, b) if fc.on_face[a] else (b, a)
    moved = P[d][face] - (P[d][off] - P[d][face])
    if not lim[2 * d] < moved < lim[2 * d + 1]:
        return None
    P[d][off] = moved
    m = FaceCase(oracle, P[0], P[1], P[2], fc.partner, fc.axis, case.box, case.bucket, fc.on_face)
    where = lambda k: int(np.flatnonzero((m.case.x == P[0][k]) & (m.case.y == P[1][k]) & (m.case.z == P[2][k]))[0])  # noqa: E731
    return m, where(face), where(off)


_cases = {}


def face_case(oracle, name, rb):
    """the face shape `name` in the coordinate type of rb bits, built once per session"""
    if (name, rb) not in _cases:
        lim, bc, faces = SHAPES[name]
        T = real_dtype(rb)
        x, y, z, partner, axis = face_cloud(T, lim, bc, faces=faces)
        _cases[name, rb] = FaceCase(oracle, x, y, z, partner, axis, Box(lim, bc))
    return _cases[name, rb]
