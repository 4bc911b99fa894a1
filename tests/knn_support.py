"""The plain restatement of the k-nearest-neighbour query (include/cstone_hip.h: cstone_hip_knn) and the clouds of
tests/test_knn.py.  Host side only: numpy.

Offsets, the fold and d2 are those of the sphere queries, evaluated in the coordinate dtype (sphere_support.d2_table:
d = r_j - c_q; d - len * rint(d * inv) on periodic axes for every particle; d2 = dx*dx + dy*dy + dz*dz left to right).
Particle j of [first, last) is a candidate iff j != s_q and d2 < r_q * r_q (the product in the coordinate dtype; +inf
without a limit); the candidates are ordered with np.lexsort((j, d2)) and the first k are the answer.  All (query,
particle) pairs are looked at: no tree.  Every comparison with the device is ==."""
import numpy as np

import sphere_support as ss

MAX_K = 256
NONE = 0xFFFFFFFF
SENT_INDEX = 0x5A5A5A5A  # what the tests fill neighbors with
SENT_DIST = -777.25
SENT_COUNT = 0x5B5B5B5B


class Knn:
    """neighbors [Q, k] uint32, dist2 [Q, k] in the coordinate type, counts [Q] uint32; unfilled slots NONE and +inf"""

    def __init__(self, pos, first, last, lim, bc, qc, k, rmax=None, qself=None, d2=None):
        T = pos[0].dtype.type
        qc = np.asarray(qc, dtype=T).reshape(-1, 3)
        Q, n = qc.shape[0], pos[0].size
        with np.errstate(over="ignore", invalid="ignore"):
            if d2 is None:
                d2 = ss.d2_table(pos, qc, lim, bc)
            r2 = np.full(Q, np.inf, dtype=T) if rmax is None else np.asarray(rmax, dtype=T) * np.asarray(rmax, dtype=T)
        assert d2.dtype == pos[0].dtype and r2.dtype == pos[0].dtype and d2.shape == (Q, n)
        self.d2_table = d2
        self.neighbors = np.full((Q, k), NONE, dtype=np.uint32)
        self.dist2 = np.full((Q, k), np.inf, dtype=T)
        self.counts = np.zeros(Q, dtype=np.uint32)
        j = np.arange(n)
        in_range = (j >= first) & (j < last)
        for q in range(Q):
            with np.errstate(invalid="ignore"):
                cand = in_range & (d2[q] < r2[q])
            if qself is not None:
                cand &= j != int(qself[q])
            idx = np.flatnonzero(cand)
            idx = idx[np.lexsort((idx, d2[q][idx]))][:k]
            m = idx.size
            self.neighbors[q, :m] = idx
            self.dist2[q, :m] = d2[q][idx]
            self.counts[q] = m
        for a in (self.neighbors, self.dist2, self.counts):
            a.flags.writeable = False


def lattice(T, spacing_log2=4):
    """the cubic lattice i * 2^-spacing_log2 of the unit box, i = 0 .. 2^spacing_log2 - 1 per axis: every coordinate and
    every d2 to a lattice point or a cell centre is exact in float32"""
    g = np.arange(2 ** spacing_log2) * 2.0 ** -spacing_log2
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    return [a.ravel().astype(T) for a in (X, Y, Z)]


def tie_sizes(d2_row, k):
    """how many particles share the d2 of the k-th nearest (0 if there are fewer than k)"""
    s = np.sort(d2_row)
    return int((s == s[k - 1]).sum()) if k <= s.size else 0


def leaves(oracle, case, qc):
    """(leaf of every particle, leaf of every query point), leaves numbered as in the cornerstone array: a point belongs
    to the leaf that holds its SFC key, which is how a particle comes to lie in a node"""
    ks = np.sort(oracle.compute_sfc_keys(case.curve, 64, case.x, case.y, case.z, case.box))
    tree, counts = oracle.compute_octree(ks, case.bucket)
    assert np.array_equal(np.concatenate([[0], np.cumsum(counts)]), case.layout)
    qc = np.asarray(qc, dtype=case.x.dtype)
    qk = oracle.compute_sfc_keys(case.curve, 64, *[np.ascontiguousarray(qc[:, a]) for a in range(3)], case.box)
    of_particle = np.searchsorted(case.layout, np.arange(case.n), side="right") - 1
    return of_particle, np.searchsorted(tree, qk, side="right") - 1
