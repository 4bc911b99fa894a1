"""The plain restatement of the pair counts (include/cstone_hip.h: cstone_hip_pair_counts, cstone_hip_pair_counts_cross) and
the inputs of tests/test_pair_counts.py.  Host side only: numpy and plain Python.

Counts.  Offsets, the fold, d2 and the squared edges are evaluated in the coordinate dtype exactly as the rule says
(d = r_j - r_i; d - len * rint(d * inv) on periodic axes for every pair; d2 = dx*dx + dy*dy + dz*dz left to right; e2_b =
T(edges[b]) * T(edges[b])).  Bins are found by the comparisons e2_b <= d2 < e2_{b+1} over ALL (target, source) pairs, in
blocks of targets: no tree.  Auto counts leave out j == i by index.  Counts are exact.

Sums.  The term of a pair is p = double(w_i) * double(w_j), one rounding (none for float32 weights: 48 bits fit).  The
device adds the n terms of a bin in some fixed order: per lane, then a butterfly, then rows.  For ANY order of adding n
doubles the computed sum is sum_k p_k (1 + theta_k), |theta_k| <= gamma_{n-1} (Higham, Accuracy and Stability of Numerical
Algorithms, eq. 4.4); with the rounding of the product |theta_k| <= gamma_n, gamma_n = n u / (1 - n u), u = 2^-53.  So the
device's sum lies within gamma_n * sum |p_k| of the exact sum of the exact products.  The reference here is math.fsum over
the ROUNDED products: correctly rounded, and each term off by u |p_k|, so it lies within (2 u) sum |p_k| <= gamma_n sum
|p_k| of the same exact value for n >= 2 (n = 1: both are the one rounded product, equal bits).  Hence

    |device - reference| <= 2 gamma_n sum |double(w_i) double(w_j)|

and nothing measured goes into it.  Weights that are powers of two with few distinct exponents make every product and
every partial sum exact: those are compared with ==.

The node test.  target_groups restates how the kernel groups 64 consecutive targets under one box, group_skip_table its
pruning test -- the group's box against a node, folded centre offset, |d| - size_node - size_box clamped at 0, against
(e_NB (1 + 16 eps) + 256 eps L)^2 -- with the absolute term of its margin or without."""
import math

import numpy as np

import sphere_support as ss

MAX_BINS = 64
U = 2.0 ** -53
SENT_COUNT = -0x0123456789ABCDEF  # what the tests fill counts with (int64 storage of the u64 array)
SENT_SUM = -777.25
BLOCK = 512


def edges2(edges, T):
    e = np.asarray(edges, dtype=np.float64).astype(T)
    e2 = e * e
    assert e2.dtype == T
    return e2


class PairCounts:
    """counts [NB] uint64, sums [NB] float64 (fsum of the rounded products), abs_sums [NB].  tpos: the targets' coordinates
    (three arrays), tw their weights or None (1); t_index: the index of target t among the sources, or None where nothing
    is excluded"""

    def __init__(self, pos, w, first, last, tpos, tw, t_index, lim, bc, edges):
        T = pos[0].dtype.type
        nb = len(edges) - 1
        e2 = edges2(edges, T)
        _, _, ln, inv = ss.box_arrays(lim, T)
        src = [np.ascontiguousarray(p[first:last]) for p in pos]
        w64 = None if w is None else np.asarray(w).astype(np.float64)[first:last]
        nt = tpos[0].size
        tw64 = None if w is None else (np.ones(nt) if tw is None else np.asarray(tw).astype(np.float64))
        counts = np.zeros(nb, dtype=np.uint64)
        terms = [[] for _ in range(nb)]
        jidx = np.arange(first, last)
        for t0 in range(0, nt, BLOCK):
            t1 = min(t0 + BLOCK, nt)
            d2 = None
            for a in range(3):
                d = src[a][None, :] - np.asarray(tpos[a][t0:t1], dtype=T)[:, None]
                if int(bc[a]) == 1:
                    d = d - ln[a] * np.rint(d * inv[a])
                sq = d * d
                d2 = sq if d2 is None else d2 + sq
            assert d2.dtype == pos[0].dtype
            ok = np.ones(d2.shape, dtype=bool)
            if t_index is not None:
                ok = jidx[None, :] != np.asarray(t_index[t0:t1])[:, None]
            # e2 does not descend, so "e2_b <= d2 < e2_{b+1}" picks b = (number of squared edges <= d2) - 1, if that lies
            # in 0 .. NB - 1; a NaN d2 sorts behind every edge and lands in no bin
            with np.errstate(invalid="ignore"):
                b_of = np.searchsorted(e2, d2.ravel(), side="right").reshape(d2.shape) - 1
            m = (b_of >= 0) & (b_of < nb) & ok
            counts += np.bincount(b_of[m], minlength=nb).astype(np.uint64)
            if w64 is not None:
                ti, sj = np.nonzero(m)
                p, pb = tw64[t0 + ti] * w64[sj], b_of[ti, sj]
                for b in np.unique(pb):
                    terms[b].append(p[pb == b])
        self.counts = counts
        self.sums = np.zeros(nb)
        self.abs_sums = np.zeros(nb)
        if w64 is not None:
            for b in range(nb):
                p = np.concatenate(terms[b]) if terms[b] else np.zeros(0)
                self.sums[b] = math.fsum(p.tolist())
                self.abs_sums[b] = math.fsum(np.abs(p).tolist())
        for a in (self.counts, self.sums, self.abs_sums):
            a.flags.writeable = False

    def sum_bound(self):
        n = self.counts.astype(np.float64)
        return 2.0 * (n * U / (1.0 - n * U)) * self.abs_sums


def auto_reference(pos, w, first, last, t_first, t_last, lim, bc, edges):
    tpos = [p[t_first:t_last] for p in pos]
    tw = None if w is None else np.asarray(w)[t_first:t_last]
    return PairCounts(pos, w, first, last, tpos, tw, np.arange(t_first, t_last), lim, bc, edges)


def cross_reference(pos, w, first, last, qc, qw, lim, bc, edges):
    T = pos[0].dtype.type
    qc = np.asarray(qc, dtype=T).reshape(-1, 3)
    return PairCounts(pos, w, first, last, [np.ascontiguousarray(qc[:, a]) for a in range(3)], qw, None, lim, bc, edges)


def xi_natural(counts, edges, n_targets, n_partners, volume):
    """the header's formula in float64, in its order"""
    out = np.empty(len(edges) - 1)
    four_pi_3 = 4.0 * 3.14159265358979323846 / 3.0
    for b in range(out.size):
        e0, e1 = float(edges[b]), float(edges[b + 1])
        shell = four_pi_3 * (e1 * e1 * e1 - e0 * e0 * e0)
        expected = n_targets * n_partners * shell / volume
        out[b] = float(counts[b]) / expected - 1.0 if shell > 0.0 and expected > 0.0 else math.nan
    return out


# ---- the node test of csrc/pair_counts.hip, restated -------------------------------------------------------------------

def abs_margin(lim, T):
    """256 eps L, L the largest of |lo|, |hi|, len over the axes: the absolute term of the kernel's margin"""
    lim = np.asarray(lim, dtype=np.float64)
    L = max(max(abs(lim[2 * a]), abs(lim[2 * a + 1]), lim[2 * a + 1] - lim[2 * a]) for a in range(3))
    return T(256.0 * float(np.finfo(T).eps) * L)


def target_groups(tpos, edges, T):
    """(ranges [(t0, t1)], centre [G, 3], half size [G, 3]) of the groups of targets that share a box and a traversal, as
    the kernel forms them: every 64 consecutive targets are one wave (lanes past the end repeat the last target); the wave
    is cut into aligned groups of gs lanes, gs the largest power of two for which no group's half extent -- the largest
    of (hi - lo) over the axes, halved, in T -- exceeds 2 e_NB; centre and half size are rounded as the kernel rounds
    them"""
    nt = tpos[0].size
    spread = T(2) * T(np.float64(edges[-1]))
    ranges, cen, hs = [], [], []
    for w0 in range(0, nt, 64):
        nv = min(64, nt - w0)
        lanes = np.minimum(np.arange(64), nv - 1) + w0
        v = np.stack([np.asarray(tpos[a], dtype=T)[lanes] for a in range(3)], axis=1)
        gs = 1
        while gs < 64:
            g = v.reshape(64 // (2 * gs), 2 * gs, 3)
            ext = (g.max(axis=1) - g.min(axis=1)).max(axis=1)
            if (ext * T(0.5) > spread).any():
                break
            gs *= 2
        for g0 in range(0, nv, gs):
            g = v[g0:g0 + gs]
            lo, hi = g.min(axis=0), g.max(axis=0)
            h = (hi - lo) * T(0.5)
            ranges.append((w0 + g0, w0 + min(g0 + gs, nv)))
            hs.append(h)
            cen.append(lo + h)
    return ranges, np.array(cen, dtype=T), np.array(hs, dtype=T)


def group_skip_table(case, tpos, edges, absolute=True):
    """skip[group, node]: the kernel's node test prunes node for the group of targets"""
    T = case.x.dtype.type
    lim, bc = case.box.lim, case.box.bc
    _, _, ln, inv = ss.box_arrays(lim, T)
    _, cen, hs = target_groups(tpos, edges, T)
    eps = T(np.finfo(T).eps)
    eN = T(np.float64(edges[-1]))
    thr = eN * (T(1) + T(16) * eps) + (abs_margin(lim, T) if absolute else T(0))
    thr2 = thr * thr
    d2 = None
    for a in range(3):
        d = case.cen[:, a][None, :] - cen[:, a][:, None]
        if int(bc[a]) == 1:
            d = d - ln[a] * np.rint(d * inv[a])
        d = (np.abs(d) - case.siz[:, a][None, :]) - hs[:, a][:, None]
        d = np.where(d > T(0), d, T(0))
        sq = d * d
        d2 = sq if d2 is None else d2 + sq
    assert d2.dtype == case.x.dtype
    return d2 > thr2


def group_hits(pos, tpos, t_index, lim, bc, edges):
    """hit[group, j]: particle j falls into some bin of some target of the group (the pair test alone)"""
    T = pos[0].dtype.type
    e2 = edges2(edges, T)
    _, _, ln, inv = ss.box_arrays(lim, T)
    ranges, _, _ = target_groups(tpos, edges, T)
    hit = np.zeros((len(ranges), pos[0].size), dtype=bool)
    for g, (t0, t1) in enumerate(ranges):
        d2 = None
        for a in range(3):
            d = pos[a][None, :] - np.asarray(tpos[a][t0:t1], dtype=T)[:, None]
            if int(bc[a]) == 1:
                d = d - ln[a] * np.rint(d * inv[a])
            sq = d * d
            d2 = sq if d2 is None else d2 + sq
        m = (e2[0] <= d2) & (d2 < e2[-1])
        if t_index is not None:
            m &= np.arange(pos[0].size)[None, :] != np.asarray(t_index[t0:t1])[:, None]
        hit[g] = m.any(axis=0)
    return hit


# ---- inputs ------------------------------------------------------------------------------------------------------------

def face_waves(T, lim, bc, m=60, level=3, seed=53, background=1000):
    """Waves of 64 targets about cell faces, for an outer edge R = 4 eps of the coordinate type: a few ulps of the
    coordinates (the kernel then walks once per target or per few targets: target_groups).  Group t takes a face lo + k * (len / 2^level) of axis a = t % 3 with 1/2 <= |face| < 4, where R is r = 2,
    4 or 8 ulps of the face coordinate.  Its 64 targets share the coordinate c = face -+ (r - 1) ulps on axis a, one side
    of the face in turn; lane 0 sits at the point p, the others are scattered up to 10^-3 about it in the two other
    directions.  Two particles share p's other coordinates: one ON the face, (r - 1) ulps from the targets' plane and so
    inside R by ONE ulp, and one a further ulp beyond the face, at exactly R: outside, the bins are half-open.  The true
    distance of the targets' box to the cell behind the face is r - 1 ulps; as computed it is all cancellation.  On a
    periodic axis every eighth group sits just below hi with its particles at lo: the face of the BOX.  `background`
    uniform particles make the tree deep.  Returns (x, y, z, targets [64 m, 3], R)."""
    rng = np.random.default_rng(seed)
    cells = 2 ** level
    limT = np.asarray(lim, dtype=np.float64).astype(T)
    lo, hi = limT[0::2], limT[1::2]
    edge = (hi - lo) / T(cells)
    R = T(4.0 * float(np.finfo(T).eps))
    pts, qc = [], np.empty((64 * m, 3), dtype=T)
    for t in range(m):
        a = t % 3
        faces = [T(lo[a] + T(k) * edge[a]) for k in range(1, cells)]
        faces = [f for f in faces if 0.5 <= abs(float(f)) < 4.0]
        face = faces[int(rng.integers(0, len(faces)))]
        sign = 1 if (t // 3) % 2 == 0 else -1  # the side of the particles; the targets lie on the other
        wrap = int(bc[a]) == 1 and t % 8 == 0 and 0.5 <= abs(float(hi[a])) < 4.0
        ulp = T(np.spacing(np.abs(hi[a] if wrap else face)))
        r = int(round(float(R) / float(ulp)))
        assert r in (2, 4, 8)
        p = np.array([lo[d] + (hi[d] - lo[d]) * T(rng.uniform(0.05, 0.95)) for d in range(3)], dtype=T)
        on, beyond = p.copy(), p.copy()
        if wrap:
            c = T(hi[a] - T(r - 1) * ulp)
            on[a], beyond[a] = lo[a], np.nextafter(lo[a], T(np.inf))
        else:
            c = T(face - T(sign) * T(r - 1) * ulp)
            on[a] = face
            beyond[a] = np.nextafter(face, T(np.inf) if sign > 0 else T(-np.inf))
        pts += [on, beyond]
        g = np.tile(p, (64, 1))
        g[1:] += (rng.uniform(-1e-3, 1e-3, (63, 3))).astype(T)
        g[:, a] = c
        qc[64 * t:64 * t + 64] = g
    pts = np.array(pts, dtype=T)
    bg = np.stack([(lo[d] + (hi[d] - lo[d]) * rng.uniform(0.01, 0.99, background)).astype(T) for d in range(3)], axis=1)
    pts = np.concatenate([pts, bg])
    return [np.ascontiguousarray(pts[:, d]) for d in range(3)] + [qc, float(R)]


def lattice(k, a, T):
    """the k^3 points a * (i, j, l), i, j, l = 0 .. k - 1"""
    g = (np.arange(k) * a).astype(T)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    return [np.ascontiguousarray(v.ravel()) for v in (X, Y, Z)]


def pow2_weights(n, seed, T=np.float64):
    return (2.0 ** np.random.default_rng(seed).integers(-1, 3, n)).astype(T)


def weights(n, bits, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, n).astype(np.float32 if bits == 32 else np.float64)
