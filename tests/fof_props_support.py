"""The numpy restatement of the group catalogue's rule (include/cstone_hip.h, cstone_hip_fof_group_properties) and the
derived tolerances, for tests/test_fof_props.py and tests/fof_catalog_mr_worker.py (host side only).

The restatement computes the offsets d = r_j - r_ref and their fold in the coordinate type T exactly as the rule says and
sums in float64 in member order.  Flags are compared with ==.  The tolerances are derived, not measured: with n members,
eps = 2^-53, eps_T the unit roundoff of T and dmax = max_j |d_j| (Euclidean), any order of summation of n products in
float64 differs from the exact sum by at most (n + 1) eps sum |terms| to first order, a quotient adds one eps and the
relative error of M, so
    mass      (n + 2) eps M + eps_T M
    centre    (2 n + 8) eps dmax + 2 eps_T max |lim|          per component
    velocity  (2 n + 8) eps max |v| + eps_T max |v|
    radius^2  (4 n + 32) eps dmax^2 + 2 eps_T radius^2        (compared as a square)
and for the combine across ranks, whose partials are shifted by s = fold(r_p - r_ref), 8 eps (|s| + dmax) more for the
centre and 8 eps (|s| + dmax)^2 more for radius^2.

With float32 coordinates the combine needs one more term.  The rule's offset is d_j = fl_T(r_j - r_ref), one rounding in
T; across ranks a member's offset is e_j + s with e_j = fl_T(r_j - r_p) and s = fl_T(r_p - r_ref), two roundings in T of
quantities up to |s| + dmax: per component the two differ by delta <= eps_T (|e_j| + |s| + |d_j|) <= 2 eps_T (|s| + dmax).
The centre moves by at most delta.  radius^2 is the mean of |d_j - c|^2 with |d_j - c| <= 2 dmax; moving every d_j and c by
up to sqrt(3) delta changes a term by at most 2 (2 dmax) (2 sqrt(3) delta) <= 28 eps_T dmax (|s| + dmax).  So for T =
float32: 2 eps_T (|s| + dmax) more for the centre and 28 eps_T (|s| + dmax)^2 more for radius^2.  (For float64, eps_T = eps
and the terms above stand as they are.)"""
import numpy as np

WIDE, MASSLESS = 0x1, 0x2
EPS = 2.0 ** -53


def eps_of(T):
    return 2.0 ** -24 if np.dtype(T) == np.float32 else 2.0 ** -53


def box_lengths(T, lim):
    """L_a as the library derives it in T: T(hi) - T(lo)"""
    T = np.dtype(T).type
    return [T(lim[2 * a + 1]) - T(lim[2 * a]) for a in range(3)]


def fold(d, L, periodic):
    """d (array of T) folded at most once, in T"""
    if not periodic:
        return d
    T = d.dtype.type
    half = T(0.5) * L
    return np.where(d >= half, d - L, np.where(d < -half, d + L, d)).astype(T)


def seq_sum(a):
    """the sum of a float64 array in index order"""
    return float(np.cumsum(a)[-1]) if a.size else 0.0


class GroupRef:
    """the rule's values of one group in float64 (not yet rounded to T), its flags and what the tolerances need"""


def group_reference(pos, m, vel, members, ref, lim, bc):
    """pos = (x, y, z) arrays of T, m masses, vel = (vx, vy, vz) or None, members: indices in member order, ref: index of
    the reference particle"""
    T = pos[0].dtype.type
    L = box_lengths(T, lim)
    g = GroupRef()
    d = []
    wide = False
    for a in range(3):
        da = fold((pos[a][members] - pos[a][ref]).astype(T), L[a], bc[a] == 1)
        if bc[a] == 1 and (np.abs(da) >= T(0.25) * L[a]).any():
            wide = True
        d.append(da.astype(np.float64))
    mj = m[members].astype(np.float64)
    g.n = len(members)
    g.M = seq_sum(mj)
    S = [seq_sum(mj * d[a]) for a in range(3)]
    g.Q = seq_sum(mj * (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    g.dmax = float(np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2).max())
    g.flags = WIDE if wide else 0
    g.ref = np.array([float(pos[a][ref]) for a in range(3)])
    g.vmax = 0.0
    if g.M == 0.0:
        g.flags |= MASSLESS
        g.center, g.velocity, g.radius2 = g.ref.copy(), np.zeros(3), 0.0
        return g
    cm = np.array([S[a] / g.M for a in range(3)])
    c = g.ref + cm
    for a in range(3):
        if bc[a] == 1:
            lo, hi = float(T(lim[2 * a])), float(T(lim[2 * a + 1]))
            if c[a] < lo:
                c[a] += float(L[a])
            elif c[a] >= hi:
                c[a] -= float(L[a])
    g.center = c
    g.radius2 = max(0.0, g.Q / g.M - float(cm @ cm))
    if vel is not None:
        v = [vel[a][members].astype(np.float64) for a in range(3)]
        g.velocity = np.array([seq_sum(mj * v[a]) / g.M for a in range(3)])
        g.vmax = float(max(np.abs(v[a]).max() for a in range(3)))
    else:
        g.velocity = np.zeros(3)
    return g


def catalogue_reference(pos, m, vel, offsets, members, lim, bc):
    """one GroupRef per group of a catalogue in the form cstone_hip_fof_catalog writes; the reference of a group is its
    first member"""
    out = []
    for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
        mem = members[a:b].astype(np.int64)
        out.append(group_reference(pos, m, vel, mem, int(mem[0]), lim, bc))
    return out


def tolerances(g, T, lim, shift=0.0):
    """(mass, centre component, velocity component, radius^2) bounds of the module's docstring; shift: |s| of the
    combine across ranks"""
    et, n = eps_of(T), g.n
    limmax = float(np.abs(np.asarray(lim, dtype=np.float64)).max())
    extra = 8 * EPS * (shift + g.dmax) if shift else 0.0
    extra2 = 8 * EPS * (shift + g.dmax) ** 2 if shift else 0.0
    if shift and et > EPS:  # the offsets about r_p and the shift are rounded in T
        extra += 2 * et * (shift + g.dmax)
        extra2 += 28 * et * (shift + g.dmax) ** 2
    return ((n + 2) * EPS * abs(g.M) + et * abs(g.M), (2 * n + 8) * EPS * g.dmax + 2 * et * limmax + extra,
            (2 * n + 8) * EPS * g.vmax + et * g.vmax, (4 * n + 32) * EPS * g.dmax ** 2 + 2 * et * g.radius2 + extra2)


def compare(got, refs, T, lim, bc, velocities=True, shifts=None, skip_wide_geometry=False, flags_equal=True):
    """got = dict(mass, center, velocity, radius, flags) of numpy arrays; a list of what is wrong (empty: all is well).
    Centres are compared modulo the box on periodic axes.  skip_wide_geometry: centre and radius of a group whose WIDE
    flag is set in `got` are not compared (the combine across ranks); flags_equal False: the caller compares the flags"""
    bad = []
    L = [float(v) for v in box_lengths(T, lim)]
    worst = dict(mass=0.0, center=0.0, velocity=0.0, radius2=0.0)
    for k, g in enumerate(refs):
        tm, tc, tv, tr = tolerances(g, T, lim, 0.0 if shifts is None else shifts[k])
        if flags_equal and int(got["flags"][k]) != g.flags:
            bad.append(f"group {k}: flags {int(got['flags'][k])}, reference {g.flags}")
        dm = abs(float(got["mass"][k]) - g.M)
        worst["mass"] = max(worst["mass"], dm / tm if tm else 0.0)
        if not dm <= tm:
            bad.append(f"group {k} (n {g.n}): mass off by {dm:.3e}, bound {tm:.3e}")
        if velocities:
            dv = np.abs(got["velocity"][k].astype(np.float64) - g.velocity).max()
            worst["velocity"] = max(worst["velocity"], dv / tv if tv else 0.0)
            if not dv <= tv:
                bad.append(f"group {k} (n {g.n}): velocity off by {dv:.3e}, bound {tv:.3e}")
        if skip_wide_geometry and (int(got["flags"][k]) & WIDE):
            continue
        dc = got["center"][k].astype(np.float64) - g.center
        for a in range(3):
            if bc[a] == 1:
                dc[a] -= L[a] * np.round(dc[a] / L[a])
        worst["center"] = max(worst["center"], float(np.abs(dc).max()) / tc)
        if not np.abs(dc).max() <= tc:
            bad.append(f"group {k} (n {g.n}): centre off by {np.abs(dc).max():.3e}, bound {tc:.3e}")
        dr = abs(float(got["radius"][k]) ** 2 - g.radius2)
        worst["radius2"] = max(worst["radius2"], dr / tr if tr else 0.0)
        if not dr <= tr:
            bad.append(f"group {k} (n {g.n}): radius^2 off by {dr:.3e}, bound {tr:.3e}")
    return bad, worst


# ---- the hand-built partitions -------------------------------------------------------------------------------------------

HAND_N = 2000
HAND_SIZES = [1, 1, 62, 64, 65, 1, 63, 127, 128, 129, 255, 257, 1, 513]  # ... and the rest


def hand_sizes(n=HAND_N):
    return HAND_SIZES + [n - sum(HAND_SIZES)]


def hand_partition(sizes, n=HAND_N, seed=31):
    """(offsets, members): the groups of the given sizes over a random permutation of [0, n): members of a group ascend but
    lie scattered over the array"""
    assert sum(sizes) == n
    perm = np.random.default_rng(seed).permutation(n)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    members = np.concatenate([np.sort(perm[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]).astype(np.uint32)
    return offsets, members


def hand_particles(T, TM=None, n=HAND_N, seed=32):
    """random positions in the unit box, masses in [0.5, 1.5), velocities in [-1, 1)"""
    rng = np.random.default_rng(seed)
    pos = [rng.uniform(0, 1, n).astype(T) for _ in range(3)]
    m = rng.uniform(0.5, 1.5, n).astype(TM or T)
    vel = [rng.uniform(-1, 1, n).astype(T) for _ in range(3)]
    return pos, m, vel


def seeded_fields(index, T, n_cloud):
    """m in [0.5, 1.5) and vx, vy, vz in [-1, 1) of the particles with the given indices into a cloud of n_cloud
    particles: a function of the index"""
    rng = np.random.default_rng(77)
    table = rng.uniform(0, 1, (4, n_cloud))
    m = (0.5 + table[0][index]).astype(T)
    return m, [(2 * table[1 + a][index] - 1).astype(T) for a in range(3)]


# ---- a partition large enough for a wave to walk several chunks ----------------------------------------------------------

LARGE_N = 1300003  # 20 313 chunks of 64 members over the kernel's 8 192 waves: 3 chunks, a span of 192 members, per wave
LARGE_SPAN = 192
_large = {}


def large_cuts(n=LARGE_N, span=LARGE_SPAN):
    """group edges on, one before and one behind: chunk edges inside a wave's span and the edges between spans (which
    leaves singletons either side of every such edge); a group that fills exactly one span beside one that covers five
    whole spans; a group that begins in the first chunk of a span and ends in its third; 250 random edges, so that most
    groups cover many spans and many carries"""
    assert (n + 63) // 64 > 2 * 8192 and -(-((n + 63) // 64) // 8192) == 3 and span == 3 * 64
    cuts = {0, n}
    for w in (1, 10, 11, 500, 3000, 6000, (n // span) - 1, n // span):
        for edge in (span * w, span * w + 64, span * w + 128):
            cuts.update(e for e in (edge - 1, edge, edge + 1) if 0 < e < n)
    cuts.update(np.random.default_rng(35).integers(1, n, 250).tolist())
    whole = [(span * 2000, span * 2001), (span * 2001, span * 2006), (span * 4000 + 10, span * 4000 + 150)]
    for a, b in whole:  # (nothing inside these three groups)
        cuts.difference_update(range(a + 1, b))
        cuts.update([a, b])
    cuts.add(span * 2006 + 1)
    return np.array(sorted(cuts), dtype=np.uint32)


def large_case(T):
    """(pos, m, vel, offsets, members, references with velocities) of the large partition in a periodic unit box: built
    once per coordinate type, shared and never modified"""
    key = np.dtype(T).name
    if key not in _large:
        offsets = large_cuts()
        perm = np.random.default_rng(36).permutation(LARGE_N)
        members = np.concatenate([np.sort(perm[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]).astype(np.uint32)
        pos, m, vel = hand_particles(T, n=LARGE_N, seed=37)
        refs = catalogue_reference(pos, m, vel, offsets, members, [0, 1] * 3, (1, 1, 1))
        for a in (offsets, members, m, *pos, *vel):
            a.flags.writeable = False
        _large[key] = (pos, m, vel, offsets, members, refs)
    return _large[key]
