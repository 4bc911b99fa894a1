"""The plain restatement of the sphere queries (include/cstone_hip.h: cstone_hip_sphere_profiles,
cstone_hip_spherical_overdensity) and the clouds of tests/test_sphere_profiles.py.  Host side only: numpy and plain Python.

Profiles.  Offsets, the fold, d2 and the squared edges are evaluated in the coordinate dtype exactly as the rule says
(d = r_j - c_q; d - len * rint(d * inv) on periodic axes for every particle; d2 = dx*dx + dy*dy + dz*dz left to right; e_b =
T(s_q) * T(edges[b]), e2_b = e_b * e_b).  Bins are found by the comparisons e2_b <= d2 < e2_{b+1} (and e_NB > 0), over ALL
(query, particle) pairs: no tree.  Counts and flags are exact.  The reference sum of a bin is math.fsum, the correctly
rounded exact sum, so the whole of

    sum_bound = (n - 1) u / (1 - (n - 1) u) * sum |w_j|,   u = 2^-53, n = the bin's count

-- the bound for ANY order of adding n doubles (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4) -- belongs
to the order the device chose; nothing measured goes into it.  n <= 2 gives an exact device sum and a bound of 0 or u |w|.

Spherical overdensity.  so_reference restates the finish in float64 in the order of the header.  The device executes the
same IEEE operations (no contraction), so equal bits are expected; the bound that is ASSERTED does not rely on that.  With
eps = 2^-52 and first-order terms, each quantity as computed differs from its exact value for the given sums by at most
    dC_b <= b eps C_b               (b additions of non-negative terms; the weights of the tests are positive)
    dE_b <= eps E_b,  d(rho V_b) <= 6 eps rho V_b      (one product for E; two for E^3, two for 4 pi / 3, one for rho)
    df_b <= dC_b + d(rho V_b) + eps |f_b|
    D = f_{b*-1} - f_{b*} > 0:  dD <= df_{b*-1} + df_{b*} + eps D
    dt <= df_{b*-1} / D + t dD / D + eps t
    dR <= dt (E_{b*} - E_{b*-1}) + 4 eps E_{b*}
    dM <= dt (C_{b*} - C_{b*-1}) + dC_{b*-1} + t (dC_{b*} + dC_{b*-1}) + 4 eps C_{b*}
Two evaluations (the device's and this one) lie within twice that of each other; so_reference returns 2 dR and 2 dM.  In
the NOT_REACHED case R = E_NB and M = C_NB: 2 eps E_NB and 2 NB eps C_NB.

The node test.  node_skip_table restates the kernel's pruning test, with the absolute term of its margin or without: the
cell-face queries must lose particles without it in float32 and none with it."""
import math

import numpy as np

TOO_WIDE, NOT_REACHED, UNRESOLVED = 0x1, 0x2, 0x4
MAX_BINS = 64
U = 2.0 ** -53
EPS = 2.0 ** -52
SENT_COUNT = -0x0123456789ABCDEF  # what the tests fill counts with (int64 storage of the u64 array)
SENT_SUM = -777.25
SENT_FLAG = -1


def box_arrays(lim, T):
    limT = np.asarray(lim, dtype=np.float64).astype(T)
    lo, hi = limT[0::2], limT[1::2]
    ln = hi - lo
    return lo, hi, ln, T(1) / ln


def query_edges(qs, num_queries, edges, T):
    """e[q, b] = T(s_q) * T(edges[b]) in T"""
    s = np.ones(num_queries, dtype=T) if qs is None else np.asarray(qs, dtype=T)
    e = s[:, None] * np.asarray(edges, dtype=np.float64).astype(T)[None, :]
    assert e.dtype == T
    return e


def d2_table(pos, qc, lim, bc):
    """d2[q, j] in the coordinate type"""
    T = pos[0].dtype.type
    _, _, ln, inv = box_arrays(lim, T)
    d2 = None
    for a in range(3):
        d = pos[a][None, :] - qc[:, a][:, None]
        if int(bc[a]) == 1:
            d = d - ln[a] * np.rint(d * inv[a])
        sq = d * d
        d2 = sq if d2 is None else d2 + sq
    assert d2.dtype == pos[0].dtype
    return d2


def too_wide(e, lim, bc, T):
    _, _, ln, _ = box_arrays(lim, T)
    wide = np.zeros(e.shape[0], dtype=bool)
    for a in range(3):
        if int(bc[a]) == 1:
            wide |= e[:, -1] >= T(0.5) * ln[a]
    return wide


class Profiles:
    """counts [Q, NB] uint64, sums [Q, NB] float64 (fsum), abs_sums [Q, NB] = sum |w| per bin, flags [Q] uint32"""

    def __init__(self, pos, w, first, last, lim, bc, qc, qs, edges):
        T = pos[0].dtype.type
        qc = np.asarray(qc, dtype=T).reshape(-1, 3)
        Q, nb = qc.shape[0], len(edges) - 1
        e = query_edges(qs, Q, edges, T)
        with np.errstate(over="ignore", invalid="ignore"):
            e2 = e * e
            d2 = d2_table(pos, qc, lim, bc)
        wide = too_wide(e, lim, bc, T)
        live = ~wide & (e[:, -1] > T(0))
        self.counts = np.zeros((Q, nb), dtype=np.uint64)
        self.sums = np.zeros((Q, nb), dtype=np.float64)
        self.abs_sums = np.zeros((Q, nb), dtype=np.float64)
        self.flags = np.where(wide, TOO_WIDE, 0).astype(np.uint32)
        w64 = None if w is None else np.asarray(w).astype(np.float64)
        in_range = np.zeros(pos[0].size, dtype=bool)
        in_range[first:last] = True
        with np.errstate(invalid="ignore"):
            for q in np.flatnonzero(live):
                m = (e2[q, :-1, None] <= d2[q][None, :]) & (d2[q][None, :] < e2[q, 1:, None]) & in_range[None, :]
                self.counts[q] = m.sum(axis=1)
                if w64 is not None:
                    for b in np.flatnonzero(self.counts[q]):
                        sel = w64[m[b]]
                        self.sums[q, b] = math.fsum(sel.tolist())
                        self.abs_sums[q, b] = math.fsum(np.abs(sel).tolist())
        for a in (self.counts, self.sums, self.abs_sums, self.flags):
            a.flags.writeable = False

    def sum_bound(self):
        n1 = np.maximum(self.counts.astype(np.float64) - 1.0, 0.0)
        return n1 * U / (1.0 - n1 * U) * self.abs_sums


FOUR_PI_3 = 4.0 * 3.14159265358979323846 / 3.0


def so_reference(qs, edges, sums, profile_flags, rho, T):
    """(R, M, flags, bound_R, bound_M) of the finish on the given sums (float64 [Q, NB])"""
    Q, nb = sums.shape
    s = np.ones(Q, dtype=T) if qs is None else np.asarray(qs, dtype=T)
    R, M = np.zeros(Q), np.zeros(Q)
    bR, bM = np.zeros(Q), np.zeros(Q)
    flags = np.zeros(Q, dtype=np.uint32)
    ed = [float(v) for v in edges]
    assert ed[0] == 0.0
    for q in range(Q):
        if profile_flags is not None and int(profile_flags[q]) & TOO_WIDE:
            flags[q] = TOO_WIDE
            continue
        sq = float(s[q])
        Cp, Ep, fp, dfp = 0.0, sq * ed[0], 0.0, 0.0
        C, E, f, df, bstar = 0.0, Ep, 0.0, 0.0, 0
        for b in range(1, nb + 1):
            C = Cp + float(sums[q, b - 1])
            E = sq * ed[b]
            rv = rho * (FOUR_PI_3 * (E * E * E))
            f = C - rv
            df = b * EPS * abs(C) + 6 * EPS * abs(rv) + EPS * abs(f)
            if f < 0.0:
                bstar = b
                break
            Cp, Ep, fp, dfp = C, E, f, df
        if bstar == 0:
            flags[q], R[q], M[q] = NOT_REACHED, E, C
            bR[q], bM[q] = 2 * EPS * abs(E), 2 * nb * EPS * abs(C)
        elif bstar == 1:
            flags[q] = UNRESOLVED
        else:
            D = fp - f
            t = fp / D
            R[q] = Ep + t * (E - Ep)
            M[q] = Cp + t * (C - Cp)
            dD = dfp + df + EPS * D
            dt = dfp / D + t * dD / D + EPS * t
            dCp, dC = (bstar - 1) * EPS * abs(Cp), bstar * EPS * abs(C)
            bR[q] = 2 * (dt * (E - Ep) + 4 * EPS * abs(E))
            bM[q] = 2 * (dt * (C - Cp) + dCp + t * (dC + dCp) + 4 * EPS * abs(C))
    return R, M, flags, bR, bM


# ---- the node test of csrc/sphere.hip, restated ------------------------------------------------------------------------

def abs_margin(lim, T):
    """64 eps L, L the largest of |lo|, |hi|, len over the axes: the absolute term of the kernel's margin"""
    lim = np.asarray(lim, dtype=np.float64)
    L = max(max(abs(lim[2 * a]), abs(lim[2 * a + 1]), lim[2 * a + 1] - lim[2 * a]) for a in range(3))
    return T(64.0 * float(np.finfo(T).eps) * L)


def node_skip_table(case, qc, qs, edges, absolute=True):
    """skip[q, node]: the kernel's node test prunes node for query q -- dist2 > (e_NB * (1 + 16 eps) + 64 eps L)^2 with
    the folded, clamped centre offsets; absolute = False: the margin without its absolute term"""
    T = case.x.dtype.type
    lim, bc = case.box.lim, case.box.bc
    _, _, ln, inv = box_arrays(lim, T)
    qc = np.asarray(qc, dtype=T).reshape(-1, 3)
    e = query_edges(qs, qc.shape[0], edges, T)
    eps = T(np.finfo(T).eps)
    thr = e[:, -1] * (T(1) + T(16) * eps) + (abs_margin(lim, T) if absolute else T(0))
    thr2 = thr * thr
    d2 = None
    for a in range(3):
        d = case.cen[:, a][None, :] - qc[:, a][:, None]
        if int(bc[a]) == 1:
            d = d - ln[a] * np.rint(d * inv[a])
        d = np.abs(d) - case.siz[:, a][None, :]
        d = np.where(d > T(0), d, T(0))
        sq = d * d
        d2 = sq if d2 is None else d2 + sq
    assert d2.dtype == case.x.dtype
    return d2 > thr2[:, None]


def particles_lost(case, skip, hit):
    """number of (query, particle) pairs with hit[q, j] whose leaf, or an ancestor of it, is skipped for q"""
    o = case.o
    nn = o["num_nodes"]
    reach = ~skip[:, :nn]
    if nn > 1:
        parent = np.asarray(o["parents"])[(np.arange(1, nn) - 1) // 8]
        for c in range(1, nn):
            reach[:, c] &= reach[:, parent[c - 1]]
    nodes = np.flatnonzero(o["child_offsets"][:nn] == 0)
    node_of_leaf = np.empty(o["num_leaves"], dtype=np.int64)
    node_of_leaf[o["internal_to_leaf"][nodes]] = nodes
    leaf = np.searchsorted(case.layout, np.arange(case.n), side="right") - 1
    return int((hit & ~reach[:, node_of_leaf[leaf]]).sum())


def in_any_bin(pos, lim, bc, qc, qs, edges):
    """hit[q, j]: particle j falls into some bin of query q (the particle test alone, no range)"""
    T = pos[0].dtype.type
    qc = np.asarray(qc, dtype=T).reshape(-1, 3)
    e = query_edges(qs, qc.shape[0], edges, T)
    e2 = e * e
    d2 = d2_table(pos, qc, lim, bc)
    live = ~too_wide(e, lim, bc, T) & (e[:, -1] > T(0))
    return (e2[:, :1] <= d2) & (d2 < e2[:, -1:]) & live[:, None]


# ---- clouds and queries ------------------------------------------------------------------------------------------------

def log_edges(nb, inner, outer):
    return [inner * (outer / inner) ** (k / nb) for k in range(nb + 1)]


def linear_edges(nb, outer):
    return [outer * k / nb for k in range(nb + 1)]


def mixed_queries(pos, lim, bc, num, seed, T):
    """num query centres: a third at particle positions, a third at random points of the box, a third outside the cloud's
    extent on the open axes (inside the box on periodic ones)"""
    rng = np.random.default_rng(seed)
    lim = np.asarray(lim, dtype=np.float64)
    lo, ln = lim[0::2], lim[1::2] - lim[0::2]
    third = num // 3
    at = rng.choice(pos[0].size, third, replace=False)
    a = np.stack([pos[d][at].astype(np.float64) for d in range(3)], axis=1)
    b = lo + rng.uniform(0, 1, (third, 3)) * ln
    c = lo + rng.uniform(0, 1, (num - 2 * third, 3)) * ln
    for d in range(3):
        if int(bc[d]) != 1:
            out = rng.uniform(0.02, 0.3, c.shape[0]) * ln[d]
            c[:, d] = np.where(rng.uniform(size=c.shape[0]) < 0.5, lo[d] - out, lo[d] + ln[d] + out)
    return np.concatenate([a, b, c]).astype(T)


def face_queries(T, lim, bc, m=200, level=3, seed=41):
    """A cloud of 2 m particles and m queries about cell faces.  Pair t: particle 2t lies ON the face lo + k * (len /
    2^level) of its axis (it belongs to the cell above), particle 2t + 1 lies d_t away from the face on the side opposite
    to the query centre, d_t log-uniform between 4 ulps of the face coordinate and 1e-3; the centre lies one ulp off the
    face, above or below in turn.  The outer radius of query t is, in turn, just above the distance to the far particle
    (it passes the particle test by a few ulps of the RADIUS), just above the distance to the particle on the face (one
    ulp of the coordinate: the node test of that particle's cell is all cancellation), and twice the distance to the far
    particle.  Returns (x, y, z, centres [m, 3], scales [m]); the edges to use are [0, 0.5, 1]."""
    rng = np.random.default_rng(seed)
    cells = 2 ** level
    limT = np.asarray(lim, dtype=np.float64).astype(T)
    lo, hi = limT[0::2], limT[1::2]
    edge = (hi - lo) / T(cells)
    pts = np.empty((2 * m, 3), dtype=T)
    qc = np.empty((m, 3), dtype=T)
    qs = np.empty(m, dtype=T)
    for t in range(m):
        a = t % 3
        p = np.array([lo[d] + (hi[d] - lo[d]) * T(rng.uniform(0.05, 0.95)) for d in range(3)], dtype=T)
        face = T(lo[a] + T(rng.integers(1, cells)) * edge[a])
        sign = 1 if (t // 3) % 2 == 0 else -1  # the side of the centre
        ulp = float(np.spacing(np.abs(face)))
        d = float(np.exp(rng.uniform(np.log(4 * ulp), np.log(1e-3))))
        on, far, c = p.copy(), p.copy(), p.copy()
        on[a] = face
        far[a] = T(face - T(sign) * T(d))
        c[a] = np.nextafter(face, T(np.inf) if sign > 0 else T(-np.inf))
        pts[2 * t], pts[2 * t + 1], qc[t] = on, far, c
        kind = (t // 6) % 3
        dist = abs(float(c[a]) - float(far[a] if kind != 1 else on[a]))
        qs[t] = T(dist * (1.0 + 8 * float(np.finfo(T).eps))) * T(2.0 if kind == 2 else 1.0)
    return [np.ascontiguousarray(pts[:, d]) for d in range(3)] + [qc, qs]


def lattice_ball(R0, spacing, mass):
    """the points of the cubic lattice spacing * (i + 1/2) inside the ball of radius R0 about the origin, equal masses"""
    k = int(math.ceil(R0 / spacing)) + 1
    g = (np.arange(-k, k) + 0.5) * spacing
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    keep = X * X + Y * Y + Z * Z < R0 * R0
    return [X[keep].copy(), Y[keep].copy(), Z[keep].copy()], np.full(int(keep.sum()), mass)
