"""Builders and the two plain references of tests/test_neighbors.py (host side only, numpy and plain Python).

* pair_table: the brute force.  For target i the particles j != i with dx*dx + dy*dy + dz*dz < 4 h_i h_i, evaluated in
  the coordinate type, left to right, products not fused, dx = x_j - x_i folded by dx - len * rint(dx * inv) with
  inv = T(1) / len on periodic axes when the target's +-2h cube leaves the box (insideBox, R/findneighbors.hpp:118).
* node_table + walk_lists / wave_stats: the depth-first loop of R/traversal/traversal.hpp:69-110 restated over the
  oracle's arrays: children 0..7, leaves searched at once, internal children pushed, the last pushed popped first; the
  node test is minDistance with the same fold against 4 h^2 ext^2.  Per target it gives the ordered list; per wave of
  64 targets, walking the union of the lanes' interests, it gives the four counters of cstone_hip_find_neighbors_stats.
  The predicates are evaluated for all (target, node) and (target, particle) pairs at once with numpy; the walks
  themselves are plain Python loops over those tables."""
import numpy as np

from helpers import Box, random_cloud, real_dtype
from oracle.oracle import HILBERT, MORTON

ANISO = [-1.3, 2.1, 0.2, 0.9, -5, 7]  # BOXES[1] of test_gpu_parity.py
SENT = np.uint32(0xFFFFFFFF)          # what the tests fill lists and counts with before a call


class Case:
    """a cloud in SFC order with its octree, as the neighbour search takes it"""

    def __init__(self, oracle, x, y, z, h, box, bucket, curve=HILBERT, kb=64):
        self.rb = x.dtype.itemsize * 8
        self.box, self.bucket, self.curve = box, bucket, curve
        keys = oracle.compute_sfc_keys(curve, kb, x, y, z, box)
        ks, order = oracle.sort_pairs(keys, np.arange(x.size))
        self.x, self.y, self.z, self.h = [np.ascontiguousarray(a[order]) for a in (x, y, z, h)]
        self.n = x.size
        tree, counts = oracle.compute_octree(ks, bucket)
        self.leaf_counts = counts
        self.o = oracle.build_octree(tree)
        self.layout = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        self.cen, self.siz = oracle.node_centers(curve, self.o["prefixes"], box, self.rb)
        self._pairs, self._nodes = None, {}

    def find(self, impl, first, last, ngmax, ext=1.0):
        """(lists [last - first, ngmax], counts) of the oracle or the reference"""
        return impl.find_neighbors(self.x, self.y, self.z, self.h, first, last, self.box, self.o, self.layout, self.cen,
                                   self.siz, ngmax, ext)

    def _fold_setup(self):
        T = self.x.dtype.type
        lim = self.box.lim.astype(T)
        lo, hi = lim[0::2], lim[1::2]
        ln = hi - lo
        inv = T(1) / ln
        P = (self.x, self.y, self.z)
        s = T(2) * self.h
        inside = np.ones(self.n, dtype=bool)
        for d in range(3):
            inside &= (P[d] - s >= lo[d]) & (P[d] + s <= hi[d])
        periodic = [int(b) == 1 for b in self.box.bc]
        use = (~inside) & any(periodic)
        return T, P, ln, inv, periodic, use

    def pair_table(self):
        """nb[i, j]: j is a neighbour of target i (the brute force)"""
        if self._pairs is None:
            T, P, ln, inv, periodic, use = self._fold_setup()
            d2 = None
            for d in range(3):
                dx = P[d][None, :] - P[d][:, None]
                if periodic[d]:
                    dx = np.where(use[:, None], dx - ln[d] * np.rint(dx * inv[d]), dx)
                sq = dx * dx
                d2 = sq if d2 is None else d2 + sq
            assert d2.dtype == self.x.dtype
            nb = d2 < (T(4) * self.h * self.h)[:, None]
            np.fill_diagonal(nb, False)
            self._pairs = nb
        return self._pairs

    def node_table(self, ext=1.0):
        """ov[i, node]: the walk of target i descends into node"""
        if ext not in self._nodes:
            T, P, ln, inv, periodic, use = self._fold_setup()
            cell = T(4) * self.h * self.h * np.float32(ext) * np.float32(ext)
            assert cell.dtype == self.x.dtype
            sq = []
            for d in range(3):
                dx = self.cen[:, d][None, :] - P[d][:, None]
                if periodic[d]:
                    dx = np.where(use[:, None], dx - ln[d] * np.rint(dx * inv[d]), dx)
                dx = np.abs(dx) - self.siz[:, d][None, :]
                dx = dx + np.abs(dx)
                dx = dx * T(0.5)
                sq.append(dx * dx)
            self._nodes[ext] = sq[0] + (sq[1] + sq[2]) < cell[:, None]  # right fold, R/util/array.hpp:253-256
        return self._nodes[ext]


def walk_lists(case, first, last, ext=1.0):
    """the restated walk, one target at a time: (ordered neighbour list per target, deepest stack position)"""
    nb, ov = case.pair_table(), case.node_table(ext)
    co, i2l, lay = case.o["child_offsets"].tolist(), case.o["internal_to_leaf"].tolist(), case.layout.tolist()
    lists, deepest = [], 0
    for i in range(first, last):
        ovi, nbi, out = ov[i].tolist(), nb[i].tolist(), []

        def search(node):
            a, b = lay[i2l[node]], lay[i2l[node] + 1]
            out.extend(j for j in range(a, b) if nbi[j])

        if ovi[0]:
            if co[0] == 0:
                search(0)
            else:
                stack, node = [0], 0
                while True:
                    c0 = co[node]
                    for child in range(c0, c0 + 8):
                        if not ovi[child]:
                            continue
                        if co[child] == 0:
                            search(child)
                        else:
                            stack.append(child)
                            deepest = max(deepest, len(stack))
                    node = stack.pop()
                    if node == 0:
                        break
        lists.append(out)
    return lists, deepest


def wave_stats(case, first, last, ext=1.0):
    """the restated walk per wave of 64 consecutive targets on the union of the lanes' interests:
    [sumP2P, maxP2P, maxStack, issued tests] as cstone_hip_find_neighbors_stats counts them: a lane is charged the
    particles of every leaf its own walk reaches, maxStack is the stack position after a push (the root occupies
    position 0), issued tests are 64 x the particles of every leaf any lane of the wave reaches"""
    ov = case.node_table(ext)
    co, i2l, lay = case.o["child_offsets"].tolist(), case.o["internal_to_leaf"].tolist(), case.layout.tolist()
    sum_p2p = max_p2p = max_stack = issued = 0
    for chunk in range(first, last, 64):
        ovw = np.ascontiguousarray(ov[chunk:min(chunk + 64, last)].T)  # [node, lane]
        tests = np.zeros(ovw.shape[1], dtype=np.int64)

        def search(node, mask):
            nonlocal issued
            particles = lay[i2l[node] + 1] - lay[i2l[node]]
            issued += particles
            tests[mask] += particles

        if ovw[0].any():
            if co[0] == 0:
                search(0, ovw[0])
            else:
                stack, node, mask = [(0, ovw[0])], 0, ovw[0]
                while True:
                    c0 = co[node]
                    for child in range(c0, c0 + 8):
                        m = mask & ovw[child]
                        if not m.any():
                            continue
                        if co[child] == 0:
                            search(child, m)
                        else:
                            stack.append((child, m))
                            max_stack = max(max_stack, len(stack))
                    node, mask = stack.pop()
                    if node == 0:
                        break
        sum_p2p += int(tests.sum())
        max_p2p = max(max_p2p, int(tests.max()))
    return [sum_p2p, max_p2p, max_stack, 64 * issued]


# ---- the clouds ------------------------------------------------------------------------------------------------------

def smoothing(n, T, seed):
    """0.12 U(0.5, 1.5), every 97th 0.2: there 2h = 0.4 is beyond half the y length (0.7) of the anisotropic box"""
    h = (0.12 * np.random.default_rng(seed).uniform(0.5, 1.5, n)).astype(T)
    h[::97] = T(0.2)
    return h


def deep_cloud(T, levels):
    """for every level l = 1..levels the cell at the (1,1,1) corner of level l - 1 of the unit box: two coincident
    particles in each of its octants 0..6, at the octant's low corner plus a quarter of its edge"""
    pts = []
    for lvl in range(1, levels + 1):
        lo, edge = 1.0 - 2.0 ** -(lvl - 1), 2.0 ** -lvl
        for octant in range(7):
            p = [lo + ((octant >> s) & 1) * edge + edge / 4 for s in (2, 1, 0)]
            pts += [p, p]
    pts = np.array(pts)
    return [np.ascontiguousarray(pts[:, d]).astype(T) for d in range(3)]


def make_groups(first, last, n):
    """target groups over [first, last) as (starts, ends, covered): cut at lengths 1, 63, 64, 65, 130 in turn, one
    empty group, one group that starts before first, one that ends behind last, one stretch of 50 targets in no group;
    covered[t] tells whether target first + t belongs to a group"""
    starts, ends = [], []
    covered = np.zeros(last - first, dtype=bool)

    def add(a, b):
        starts.append(a)
        ends.append(b)
        covered[max(a, first) - first:max(min(b, last), first) - first] = True

    pos = first
    if first >= 5:
        pos = min(first + 20, last)
        add(first - 5, pos)
    cuts, k = (1, 63, 64, 65, 130), 0
    while pos < last:
        if k == 3:
            add(pos, pos)
        if k == 5:
            pos = min(pos + 50, last)  # in no group
        end = pos + cuts[k % 5]
        if end >= last:
            end = min(last + 7, n)
        if pos < last:
            add(pos, end)
        pos, k = end, k + 1
    if not starts:
        add(first, first)
    return np.array(starts, dtype=np.uint32), np.array(ends, dtype=np.uint32), covered


class Spec:
    def __init__(self, case, ranges, ngmax, exts=(1.0,)):
        self.case, self.ranges, self.ngmax, self.exts = case, ranges, ngmax, exts


N_BIG = 3000    # the clustered shapes
N_ANISO = 2000  # the uniform cloud of the anisotropic boxes
BCS = {"111": (1, 1, 1), "102": (1, 0, 2), "010": (0, 1, 0), "221": (2, 2, 1), "000": (0, 0, 0)}
DEEP_LEVELS = 21

NAMES = ([f"aniso-{bc}-b{b}" for bc in BCS for b in (16, 200)] + ["clustered-b200", "clump300"] +
         [f"single-n{n}-{p}" for n in (1, 2, 63, 64, 65, 200) for p in ("open", "pbc")] + ["deep"])

_specs = {}


def spec(oracle, name, rb):
    """the shape `name` in the coordinate type of rb bits, built once per session"""
    if (name, rb) not in _specs:
        _specs[name, rb] = _build(oracle, name, rb)
    return _specs[name, rb]


def _build(oracle, name, rb):
    T = real_dtype(rb)
    kind = name.split("-")[0]
    if kind == "aniso":
        _, bc, b = name.split("-")
        box = Box(ANISO, BCS[bc])
        x, y, z = random_cloud(N_ANISO, box, rb, 5, "uniform")  # reaches the faces of the box
        case = Case(oracle, x, y, z, smoothing(N_ANISO, T, 6), box, int(b[1:]))
        return Spec(case, [(37, N_ANISO - 11)], 8, (1.0, 1.5))
    if kind == "clustered":
        box = Box(ANISO, BCS["102"])
        x, y, z = random_cloud(N_BIG, box, rb, 5, "clustered")
        case = Case(oracle, x, y, z, smoothing(N_BIG, T, 6), box, 200)
        return Spec(case, [(37, N_BIG - 11)], 24)
    if kind == "clump300":
        box = Box(ANISO, BCS["111"])
        x, y, z = random_cloud(N_BIG, box, rb, 5, "clustered")
        for a in (x, y, z):
            a[-300:] = a[0]  # a leaf that cannot be split
        case = Case(oracle, x, y, z, smoothing(N_BIG, T, 6), box, 64)
        return Spec(case, [(37, N_BIG - 11)], 24)
    if kind == "single":
        _, n, p = name.split("-")
        n = int(n[1:])
        box = Box(ANISO, BCS["111"] if p == "pbc" else BCS["000"])
        x, y, z = random_cloud(n, box, rb, seed=n, kind="uniform")
        h = (0.8 * np.random.default_rng(n).uniform(0.5, 1.5, n)).astype(T)
        case = Case(oracle, x, y, z, h, box, n + 1)
        ranges = [(0, n)] + ([(77, 78), (70, 120)] if n == 200 else [])
        return Spec(case, ranges, 24)
    if kind == "deep":
        return Spec(deep_case(oracle, rb, DEEP_LEVELS), [(0, 14 * DEEP_LEVELS)], 14 * DEEP_LEVELS)
    raise ValueError(name)


def deep_case(oracle, rb, levels):
    T = real_dtype(rb)
    x, y, z = deep_cloud(T, levels)
    h = np.full(x.size, 0.9, dtype=T)  # 2h >= sqrt(3): every node of the unit box overlaps
    return Case(oracle, x, y, z, h, Box([0, 1]), 1, curve=MORTON, kb=64)
