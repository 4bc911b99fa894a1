"""Gravity with per-particle softening lengths (cstone_hip_compute_gravity_h / _let_h, the domains' _h calls) and the
all-pairs direct sum on the GPU (cstone_hip_direct_gravity).

The pair rule, for target i and source j != i: d = r_j - r_i, r2 = |d|^2 + eps2, H = h_i + h_j, s2 = max(r2, H^2),
rinv = 1 / sqrt(s2), w = r2 < H^2 ? 1.5 - 0.5 r2 rinv^2 : 1; a_i += G m_j rinv^3 d, phi_i -= G m_j rinv w -- the field of a
homogeneous sphere of radius H.  M2P keeps eps2 only, and the walk (MAC, counts) does not know about h.

The references live here: direct_sum_h and walk_reference_h, float64 NumPy restatements that with h = 0 reproduce
test_gravity's direct_sum and walk_reference exactly.

The bound of the direct sum, componentwise: |gpu - ref| <= (n + 16) u sum_j |term_j|, u = 2^-53 | 2^-24 and the sum of
the terms' sizes from the reference: about a dozen roundings per term (three differences, r2, H, H^2, sqrt, division,
three or four products, the conversion of the mass) and a sum of n terms in any order.  Nothing in it is measured.

Figures of the MI355X are in DESIGN.md section 7d."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gravity_mr_worker import let_centers
from test_gravity import (clustered_cloud, direct_sum, grav_domain, groups_of, gpu_gravity, rel_err, tree_state,
                          uniform_cloud, walk_reference)
from test_gravity_mr import REMOTE_MP, let_tree, raw_gravity_let
from test_gravity_walk import (GROUP_LENGTHS, HUGE_MAC, build_tree, centers_of, directions, force_scale, geometric_mac,
                               place_sources, raw_gravity, restatement_state, sources_only, three_level_desc, upload,
                               upsweep)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("cstone_hip_compute_gravity_h", "cstone_hip_compute_gravity_let_h", "cstone_hip_direct_gravity",
               "cstone_hip_domain_compute_gravity_h", "cstone_hip_domain_mr_compute_gravity_h")
TYPES = [(64, 64), (64, 32), (32, 32), (32, 64)]
E_ARG = -1


def np_real(bits):
    return np.float64 if bits == 64 else np.float32


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def soft_pair(r2, H):
    """(rinv, w, inside) of the pair rule for r2 (eps2 included) and H = h_i + h_j; r2 = inf marks the pair to skip"""
    H2 = H * H
    inside = r2 < H2
    with np.errstate(invalid="ignore"):
        rinv = 1.0 / np.sqrt(np.where(inside, H2, r2))
        w = np.where(inside, 1.5 - 0.5 * r2 * (rinv * rinv), 1.0)
    return rinv, w, inside


def direct_sum_h(x, y, z, m, h, targets, G=1.0, eps2=0.0, chunk_elems=1 << 22, sizes=False):
    """direct_sum of test_gravity with the pair rule above (h None: no softening lengths): (a (len(targets), 3), phi),
    float64, the target itself skipped (by index).  sizes: also (sum_j |term_j| of ax, ay, az, phi (len(targets), 4),
    number of pairs with r2 < H^2)"""
    x, y, z, m = [np.asarray(a, dtype=np.float64) for a in (x, y, z, m)]
    h = np.zeros_like(x) if h is None else np.asarray(h, dtype=np.float64)
    targets = np.asarray(targets, dtype=np.int64)
    acc = np.zeros((targets.size, 3))
    phi = np.zeros(targets.size)
    mag = np.zeros((targets.size, 4))
    soft = 0
    step = max(1, chunk_elems // x.size)
    for s in range(0, targets.size, step):
        t = targets[s:s + step]
        dx, dy, dz = x[None, :] - x[t, None], y[None, :] - y[t, None], z[None, :] - z[t, None]
        r2 = dx * dx + dy * dy + dz * dz + eps2
        r2[np.arange(t.size), t] = np.inf  # the target itself
        rinv, w, inside = soft_pair(r2, h[t, None] + h[None, :])
        mr = m[None, :] * rinv
        mr3 = mr * rinv * rinv
        acc[s:s + step] = G * np.stack([(mr3 * dx).sum(1), (mr3 * dy).sum(1), (mr3 * dz).sum(1)], 1)
        phi[s:s + step] = -G * (mr * w).sum(1)
        if sizes:
            mag[s:s + step] = abs(G) * np.stack([np.abs(mr3 * dx).sum(1), np.abs(mr3 * dy).sum(1),
                                                 np.abs(mr3 * dz).sum(1), np.abs(mr * w).sum(1)], 1)
            soft += int(inside.sum())
    return (acc, phi, mag, soft) if sizes else (acc, phi)


def walk_reference_h(t, lo, hi, order, G=1.0, eps2=0.0, h=None, stats=None):
    """walk_reference of test_gravity with the pair rule above in the P2P part (h: one length per particle, indexed like
    x; None: zeros).  The MAC, the M2P part and both counts are those of walk_reference.  stats (a dict): 'pairs' and
    'soft' are incremented by the number of P2P pairs and of those with r2 < H^2"""
    from test_gravity import m2p

    if hi - lo > 64:
        runs = [walk_reference_h(t, s, min(hi, s + 64), order, G, eps2, h, stats) for s in range(lo, hi, 64)]
        return tuple(np.concatenate(parts) for parts in zip(*runs))
    rdt = t["rdt"]
    xs, ys, zs = t["x"], t["y"], t["z"]
    ctr = t["centers"]
    hh = np.zeros(xs.size) if h is None else np.asarray(h, dtype=np.float64)
    lo3 = [a[lo:hi].min() for a in (xs, ys, zs)]
    hi3 = [a[lo:hi].max() for a in (xs, ys, zs)]
    tc = [(a + b) * rdt(0.5) for a, b in zip(lo3, hi3)]
    ts = [(b - a) * rdt(0.5) for a, b in zip(lo3, hi3)]
    d = []
    for k in range(3):
        v = np.abs(tc[k] - ctr[:, k]) - ts[k]
        v = v + np.abs(v)
        d.append(v * rdt(0.5))
    R2 = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])
    opened = R2 < np.abs(ctr[:, 3])
    child, itl, layout = t["child_offsets"], t["internal_to_leaf"], t["layout"]
    m2p_nodes, p2p_leaves = [], []
    stack = [0]
    while stack:
        n = stack.pop()
        if ctr[n, 3] == 0:
            continue
        if not opened[n]:
            m2p_nodes.append(n)
        elif child[n] == 0:
            p2p_leaves.append(itl[n])
        else:
            stack.extend(range(child[n] + 7, child[n] - 1, -1))
    tg = np.arange(lo, hi)
    X = [a.astype(np.float64) for a in (xs, ys, zs)]
    acc = np.zeros((tg.size, 3))
    phi = np.zeros(tg.size)
    if m2p_nodes:
        nodes = np.array(m2p_nodes)
        c64 = ctr[nodes, :3].astype(np.float64)
        dd = [X[k][tg, None] - c64[None, :, k] for k in range(3)]
        a, p = m2p(*dd, t["multipoles"][nodes].astype(np.float64), order, eps2)
        acc += a
        phi += p
    p2p_counts = np.zeros(tg.size, dtype=np.int64)
    if p2p_leaves:
        src = np.concatenate([np.arange(layout[lf], layout[lf + 1]) for lf in p2p_leaves])
        m64 = t["m"].astype(np.float64)[src]
        dd = [X[k][None, src] - X[k][tg, None] for k in range(3)]
        r2 = dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2] + eps2
        self_ = src[None, :] == tg[:, None]
        rinv, w, inside = soft_pair(np.where(self_, 1.0, r2), hh[tg, None] + hh[None, src])
        rinv = np.where(self_, 0.0, rinv)
        mr = m64[None, :] * rinv
        mr3 = mr * rinv * rinv
        acc += np.stack([(mr3 * dd[k]).sum(1) for k in range(3)], 1)
        phi -= (mr * w).sum(1)
        p2p_counts = src.size - self_.sum(1)
        if stats is not None:
            stats["pairs"] = stats.get("pairs", 0) + int((~self_).sum())
            stats["soft"] = stats.get("soft", 0) + int((inside & ~self_).sum())
    return G * acc, G * phi, p2p_counts, np.full(tg.size, len(m2p_nodes))


def walk_reference_let_h(t, lo, hi, order, G=1.0, eps2=0.0, h=None, stats=None):
    """walk_reference_let of gravity_mr_worker extended by h: (a, phi, p2p, m2p, let m2p counts)"""
    if "centers_let" not in t:
        t["centers_let"] = let_centers(t)
    plain = walk_reference_h(t, lo, hi, order, G, eps2, h)
    a, phi, p2p, m2pc = walk_reference_h(dict(t, centers=t["centers_let"]), lo, hi, order, G, eps2, h, stats)
    return a, phi, p2p, m2pc, m2pc - plain[3]


def distinct_h(n, seed, small=(0.004, 0.02), large=(0.08, 0.2)):
    """a distinct length for every particle, neighbours in the arrays differing by an order of magnitude: even indices
    from `small`, odd ones from `large`"""
    rng = np.random.default_rng(seed)
    h = np.where(np.arange(n) % 2 == 0, rng.uniform(*small, n), rng.uniform(*large, n))
    assert np.unique(h).size == n
    return h


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_soft_entry_points_are_exported():
    import cstone_amd

    lib = cstone_amd.load_library()
    for name in NEW_SYMBOLS:
        assert name in cstone_amd.EXPORTS and hasattr(lib, name), name


def test_restatements_with_zero_h_are_the_plain_ones_exactly():
    rng = np.random.default_rng(51)
    n = 300
    x, y, z = rng.uniform(0, 1, (3, n))
    m = rng.uniform(0.5, 1.5, n)
    tg = rng.permutation(n)[:200]
    for h in (None, np.zeros(n)):
        a, phi = direct_sum_h(x, y, z, m, h, tg, G=0.7, eps2=1e-4)
        ra, rphi = direct_sum(x, y, z, m, tg, G=0.7, eps2=1e-4)
        assert np.array_equal(a, ra) and np.array_equal(phi, rphi)
    tr = build_tree(three_level_desc())
    x, y, z, m = place_sources(tr, rng)
    ns, N = tr["n_src"], tr["n_src"] + 90
    x, y, z = [np.concatenate([a, rng.uniform(0, 1, N - ns)]) for a in (x, y, z)]
    m = np.concatenate([m, np.zeros(N - ns)])
    ctr = centers_of(tr, x, y, z, m, geometric_mac(tr, 0.6))
    mp = rng.normal(size=(tr["M"], 8))
    for rdt in (np.float64, np.float32):
        t = restatement_state(tr, x, y, z, m, ctr, mp, rdt)
        for lo, hi in ((0, 64), (17, 80), (100, 330), (ns - 5, N)):
            for h in (None, np.zeros(N)):
                got = walk_reference_h(t, lo, hi, 2, 0.8, 1e-5, h)
                for u, w in zip(got, walk_reference(t, lo, hi, 2, 0.8, 1e-5)):
                    assert np.array_equal(u, w)


def test_restated_rule_is_continuous_and_its_force_is_minus_the_gradient():
    """one source of mass 1.3 at the origin with h = 0.3, a target with h = 0.2 on a ray: H = 0.5.  phi and a are
    continuous across r2 = H^2 (eps2 counted in r2), and a equals the central difference of phi on both sides"""
    G, eps2, H = 0.9, 0.01, 0.5
    u = np.array([0.6, -0.48, 0.64])  # a unit vector
    assert abs(u @ u - 1) < 1e-15
    r_edge = np.sqrt(H * H - eps2)

    def field(r):
        p = np.outer(np.atleast_1d(r), u)
        x, y, z = [np.concatenate([[0.0], p[:, k]]) for k in range(3)]
        m = np.concatenate([[1.3], np.zeros(p.shape[0])])
        h = np.concatenate([[0.3], np.full(p.shape[0], 0.2)])
        # (the targets are massless: only the source at the origin acts)
        a, phi, mag, soft = direct_sum_h(x, y, z, m, h, np.arange(1, x.size), G, eps2, sizes=True)
        return a, phi

    d = 1e-9
    (a_in, a_out), (p_in, p_out) = field([r_edge - d, r_edge + d])
    assert np.abs(a_in - a_out).max() <= 1e-7 * np.abs(a_out).max() and abs(p_in - p_out) <= 1e-7 * abs(p_out)
    # at the edge itself both branches give -G m / H and -G m d / H^3
    assert abs(p_out + G * 1.3 / H) <= 1e-7 and np.allclose(a_out, -G * 1.3 * r_edge * u / H ** 3, rtol=1e-7)
    # inside: phi = -G m (3 H^2 - r2) / (2 H^3)
    _, p = field([0.2])
    assert abs(p[0] + G * 1.3 * (3 * H * H - (0.04 + eps2)) / (2 * H ** 3)) <= 1e-15
    for r in (0.05, 0.3, r_edge - 1e-3, r_edge + 1e-3, 0.8, 3.0):  # inside and outside
        step = 1e-5
        a, _ = field([r])
        _, pp = field([r + step, r - step])
        grad = (pp[0] - pp[1]) / (2 * step)
        assert abs(-grad - a[0] @ u) <= 1e-8 * np.abs(a[0] @ u), r
        assert np.abs(a[0] - (a[0] @ u) * u).max() <= 1e-15  # (radial)


@pytest.mark.parametrize("eps2", [0.0, 1e-3])
def test_restated_direct_sum_conserves_momentum(eps2):
    """the rule is symmetric in i and j: sum_i m_i a_i = 0 to rounding (n times the size of the terms)"""
    rng = np.random.default_rng(52)
    n = 500
    x, y, z = rng.uniform(0, 1, (3, n))
    m = rng.uniform(0.5, 1.5, n)
    h = rng.uniform(0.05, 0.25, n)
    a, phi, mag, soft = direct_sum_h(x, y, z, m, h, np.arange(n), eps2=eps2, sizes=True)
    assert 0.05 < soft / (n * (n - 1)) < 0.5
    total = (m[:, None] * a).sum(0)
    assert (np.abs(total) <= n * 2.0 ** -52 * (m[:, None] * mag[:, :3]).sum(0)).all(), total


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the walk on hand-built trees
# ---------------------------------------------------------------------------------------------------------------------
def raw_h(hip, d, mp, first, last, groups, order=2, G=1.0, eps2=0.0, h=None, let=False):
    """cstone_hip_compute_gravity_h / _let_h called directly, like raw_gravity: (rc, a, phi, p2p, m2p[, let_m2p]); h: a
    host array (uploaded in the coordinates' type) or None for a NULL pointer"""
    import torch

    import cstone_amd
    from cstone_amd import _ptr

    nt = last - first
    dt = d["x"].dtype
    ax, ay, az, phi = [torch.full((nt,), float("nan"), dtype=dt, device="cuda") for _ in range(4)]
    counts = [torch.full((nt,), -1, dtype=torch.int32, device="cuda") for _ in range(3 if let else 2)]
    g = torch.from_numpy(np.asarray(groups, dtype=np.int32)).cuda()
    hd = None if h is None else torch.from_numpy(np.ascontiguousarray(h, dtype=d["rdt"])).cuda()
    box = cstone_amd.make_cbox([-4.0, 4.0] * 3)
    fn = hip.lib.cstone_hip_compute_gravity_let_h if let else hip.lib.cstone_hip_compute_gravity_h
    rc = fn(hip.h, C.c_int(d["rb"]), C.c_int(d["mb"]), _ptr(d["x"]), _ptr(d["y"]), _ptr(d["z"]), _ptr(d["m"]), _ptr(hd),
            C.c_uint32(first), C.c_uint32(last), _ptr(g), C.c_uint32(g.numel() - 1), C.byref(box),
            _ptr(d["child_offsets"]), _ptr(d["internal_to_leaf"]), _ptr(d["layout"]), _ptr(d["centers"]), _ptr(mp),
            C.c_int(order), C.c_double(G), C.c_double(eps2), _ptr(ax), _ptr(ay), _ptr(az), _ptr(phi),
            *[_ptr(c) for c in counts])
    hip.sync()
    a = np.stack([t.cpu().numpy().astype(np.float64) for t in (ax, ay, az)], 1)
    return (rc, a, phi.cpu().numpy().astype(np.float64)) + tuple(c.cpu().numpy().astype(np.int64) for c in counts)


def ragged_setup(rb, mb, seed=9):
    """the tree, particles and groups of test_long_and_ragged_groups_and_sub_ranges: a three-level tree of opened and
    accepted nodes, sources followed by targets in no leaf"""
    tr = build_tree(three_level_desc())
    rng = np.random.default_rng(seed)
    x, y, z, m = place_sources(tr, rng)
    ns, N = tr["n_src"], 555
    x, y, z = [np.concatenate([a, rng.uniform(0, 1, N - ns)]) for a in (x, y, z)]
    rdt, mdt = np_real(rb), np_real(mb)
    m = np.concatenate([m, np.zeros(N - ns)]).astype(mdt).astype(np.float64)
    xr, yr, zr = [a.astype(rdt) for a in (x, y, z)]
    ctr = centers_of(tr, xr.astype(np.float64), yr.astype(np.float64), zr.astype(np.float64), m, geometric_mac(tr, 0.6))
    return tr, xr, yr, zr, m, ctr, ns, N


def same(u, v):
    return np.array_equal(u, v, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("rb,mb", TYPES)
def test_null_and_zero_h_give_the_bits_of_the_old_entry_points(hip, rb, mb):
    """h = NULL and h = 0 everywhere through compute_gravity_h and compute_gravity_let_h: a, phi and both counts (and
    the LET count) bit-equal to compute_gravity and compute_gravity_let, order 0 and 2, on a sub-range with first > 0
    that cuts through groups of 63 .. 200 targets; untouched slots keep their NaN in all of them"""
    import torch

    tr, xr, yr, zr, m, ctr, ns, N = ragged_setup(rb, mb)
    d = upload(hip, tr, xr, yr, zr, m, ctr, rb, mb)
    mp = upsweep(hip, d)
    groups = 12 + np.concatenate([[0], np.cumsum(GROUP_LENGTHS)])
    first, last = 17, N - 9
    for order in (0, 2):
        old = raw_gravity(hip, d, mp, first, last, groups, order, 0.8, 1e-4)
        assert old[0] == 0 and (old[3] > 0).any() and (old[4] > 0).any() and np.isnan(old[1]).any()
        for h in (None, np.zeros(N)):
            new = raw_h(hip, d, mp, first, last, groups, order, 0.8, 1e-4, h)
            assert all(same(u, v) for u, v in zip(old, new)), (order, h is None)
    # the LET rule: the tree with a massive leaf that has no particles
    tl, x, y, z, ml, cl, remote = let_tree(lambda t: geometric_mac(t, 1.0))
    rdt = np_real(rb)
    ml = ml.astype(np_real(mb)).astype(np.float64)
    dl = upload(hip, tl, x.astype(rdt), y.astype(rdt), z.astype(rdt), ml, cl, rb, mb)
    mpl = upsweep(hip, dl)
    mpl[remote] = torch.from_numpy(REMOTE_MP.astype(rdt)).cuda()
    Nl = x.size
    gl = list(range(0, Nl, 16)) + [Nl]
    for order in (0, 2):
        old = raw_gravity_let(hip, dl, mpl, 5, Nl - 2, gl, order, 0.8, 1e-4)
        assert old[0] == 0 and (old[5] > 0).any()
        for h in (None, np.zeros(Nl)):
            new = raw_h(hip, dl, mpl, 5, Nl - 2, gl, order, 0.8, 1e-4, h, let=True)
            assert all(same(u, v) for u, v in zip(old, new)), (order, h is None)


@pytest.mark.gpu
@pytest.mark.parametrize("rb,mb", TYPES)
@pytest.mark.parametrize("cut", ["through", "around"])
def test_softened_walk_of_long_and_ragged_groups(hip, rb, mb, cut):
    """the set-up of test_long_and_ragged_groups_and_sub_ranges (groups of 63, 1, 64, 0, 65, 130 and 200 targets, first
    and last cutting through or lying around the groups, targets after the last source) with a distinct h for every
    particle, neighbours an order of magnitude apart: the counts are those of the h-free call exactly (softening does
    not change the walk) and of the restatement, a and phi agree with walk_reference_h to that test's tolerances.
    Between 5 % and 50 % of the restated P2P pairs have r2 < H^2, so both branches of the rule are taken"""
    tr, xr, yr, zr, m, ctr, ns, N = ragged_setup(rb, mb)
    rdt = np_real(rb)
    h = distinct_h(N, 60, large=(0.15, 0.35)).astype(rdt)
    d = upload(hip, tr, xr, yr, zr, m, ctr, rb, mb)
    mp = upsweep(hip, d)
    t = restatement_state(tr, xr, yr, zr, m, ctr, mp.cpu().numpy(), rdt)
    g0 = 0 if cut == "through" else 12
    groups = g0 + np.concatenate([[0], np.cumsum(GROUP_LENGTHS)])
    first, last = (17, int(groups[-1]) - 40) if cut == "through" else (4, N)
    eps2, G = 1e-4, 0.8
    rc, a, phi, p2p, m2pc = raw_h(hip, d, mp, first, last, groups, 2, G, eps2, h)
    orc, oa, ophi, op2p, om2p = raw_gravity(hip, d, mp, first, last, groups, 2, G, eps2)
    assert rc == 0 and orc == 0
    assert same(p2p, op2p) and same(m2pc, om2p)
    inside = np.zeros(last - first, dtype=bool)
    tol = 1e-10 if rb == 64 else 5e-6
    worst, stats = 0.0, {}
    for lo, hi in zip(groups[:-1], groups[1:]):
        lo, hi = max(first, lo), min(last, hi)
        if hi <= lo:
            continue
        ra, rphi, rp2p, rm2p = walk_reference_h(t, lo, hi, 2, G, eps2, h, stats)
        sl = slice(lo - first, hi - first)
        inside[sl] = True
        assert np.array_equal(p2p[sl], rp2p) and np.array_equal(m2pc[sl], rm2p), (lo, hi)
        scale = G * force_scale(xr, yr, zr, m, ns, np.arange(lo, hi), eps2)
        worst = max(worst, (np.linalg.norm(a[sl] - ra, axis=1) / scale).max(),
                    (np.abs(phi[sl] - rphi) / np.abs(rphi)).max())
    share = stats["soft"] / stats["pairs"]
    print(f"rb={rb} mb={mb} {cut}: worst relative difference to the restatement {worst:.1e}; {share:.1%} of "
          f"{stats['pairs']} P2P pairs softened")
    assert 0.05 <= share <= 0.5
    assert worst <= tol
    assert (m2pc[inside] > 0).any() and (p2p[inside] > 0).any()
    assert inside.sum() == (last - first if cut == "through" else groups[-1] - groups[0])
    assert np.isnan(a[~inside]).all() and np.isnan(phi[~inside]).all()
    # h matters: the softened result is not the plain one
    assert (np.abs(phi[inside] - ophi[inside]) > 1e-3 * np.abs(ophi[inside])).any()


@pytest.mark.gpu
@pytest.mark.parametrize("rb", [64, 32])
def test_softened_leaves_of_more_than_64_particles(hip, rb):
    """every node opened; leaves of 200, 70 and 65 particles (ragged tails of the source tile, the target itself in the
    1st .. 4th pass of its own leaf), groups of 1, 63, 65 and 130 targets, targets after the last source: the softened
    direct sum over the sources, h indexed by the absolute particle index"""
    tr = build_tree([50, 200, 3, 0, 70, 10, 1, 65])
    rng = np.random.default_rng(10)
    x, y, z, m = place_sources(tr, rng)
    ns, ne = tr["n_src"], 30
    x, y, z = [np.concatenate([a, rng.uniform(0, 1, ne)]) for a in (x, y, z)]
    m = np.concatenate([m, np.zeros(ne)])
    rdt = np_real(rb)
    xr, yr, zr = [a.astype(rdt).astype(np.float64) for a in (x, y, z)]
    N = ns + ne
    h = distinct_h(N, 61, large=(0.1, 0.3)).astype(rdt).astype(np.float64)
    ctr = centers_of(tr, xr, yr, zr, m, lambda n: HUGE_MAC)
    d = upload(hip, tr, xr, yr, zr, m, ctr, rb, rb)
    groups = [0, 1, 64, 129, 259, 322, N]
    assert list(np.diff(groups)[:4]) == [1, 63, 65, 130]
    eps2 = 1e-6
    first = 0
    rc, a, phi, p2p, m2pc = raw_h(hip, d, upsweep(hip, d), first, N, groups, 2, 1.0, eps2, h)
    assert rc == 0
    assert (p2p == np.where(np.arange(N) < ns, ns - 1, ns)).all() and (m2pc == 0).all()
    ra, rphi, mag, soft = direct_sum_h(xr, yr, zr, sources_only(m, ns), h, np.arange(N), eps2=eps2, sizes=True)
    assert 0.05 <= soft / (N * ns) <= 0.5
    u = 2.0 ** -53 if rb == 64 else 2.0 ** -24
    bound = (ns + 16) * u * mag
    err = np.abs(np.concatenate([a - ra, (phi - rphi)[:, None]], 1))
    print(f"rb={rb}: worst |error| / bound {np.max(err / bound):.2f}")
    assert (err <= bound).all()
    # a sub-range that starts inside a group, outputs indexed by i - first, h by i
    rc, a2, phi2, _, _ = raw_h(hip, d, upsweep(hip, d), 70, N - 3, groups, 2, 1.0, eps2, h)
    assert rc == 0 and np.array_equal(a2, a[70:N - 3]) and np.array_equal(phi2, phi[70:N - 3])


@pytest.mark.gpu
@pytest.mark.parametrize("rb", [64, 32])
def test_coincident_particles_with_h(hip, rb):
    """two particles at one point and a third elsewhere, eps2 = 0: finite, the coincident partner adds no force and
    -3 G m / (2 H) to phi"""
    tr = build_tree(3)
    x, y, z = np.array([[0.25, 0.5, 0.75], [0.25, 0.5, 0.75], [0.5, 0.125, 0.25]]).T
    m = np.array([1.5, 0.5, 2.0])
    h = np.array([0.0625, 0.03125, 0.015625])
    ctr = centers_of(tr, x, y, z, m, lambda k: HUGE_MAC)
    d = upload(hip, tr, x, y, z, m, ctr, rb, rb)
    G = 2.0
    rc, a, phi, p2p, m2pc = raw_h(hip, d, upsweep(hip, d), 0, 3, [0, 3], 2, G, 0.0, h)
    assert rc == 0 and np.isfinite(a).all() and np.isfinite(phi).all() and (p2p == 2).all()
    # particle 2 alone pulls on 0 and 1, and by the same vector: the coincident partner adds nothing
    far_a, far_phi = direct_sum_h(x, y, z, [0, 0, 2.0], h, [0, 1], G=G)
    tol = 1e-15 if rb == 64 else 1e-6
    assert np.allclose(a[:2], far_a, rtol=tol, atol=0)
    H = h[0] + h[1]
    want = far_phi - 1.5 * G * m[[1, 0]] / H
    assert np.allclose(phi[:2], want, rtol=tol, atol=0), (phi[:2], want)
    ra, rphi = direct_sum_h(x, y, z, m, h, [0, 1, 2], G=G)
    assert np.allclose(a, ra, rtol=tol, atol=0) and np.allclose(phi, rphi, rtol=tol, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("rb", [64, 32])
@pytest.mark.parametrize("mac", ["open", "geometric"])
def test_let_rule_together_with_h(hip, rb, order, mac):
    """the tree of test_gravity_mr.let_tree (a massive leaf with an empty range) through compute_gravity_let_h: the three
    counts equal the restatement with the LET rule exactly and those of the h-free call, a and phi agree with it to the
    tolerance of test_let_walk_of_a_hand_built_tree"""
    import torch

    macf = (lambda tr: (lambda n: HUGE_MAC)) if mac == "open" else (lambda tr: geometric_mac(tr, 1.0))
    tr, x, y, z, m, ctr, remote = let_tree(macf)
    rdt = np_real(rb)
    xr, yr, zr = [a.astype(rdt) for a in (x, y, z)]
    m = m.astype(rdt).astype(np.float64)
    ns, N = tr["n_src"], x.size
    h = distinct_h(N, 62, large=(0.15, 0.35)).astype(rdt)
    d = upload(hip, tr, xr, yr, zr, m, ctr, rb, rb)
    mp = upsweep(hip, d)
    mp[remote] = torch.from_numpy(REMOTE_MP.astype(rdt)).cuda()
    t = restatement_state(tr, xr, yr, zr, m, d["centers"].cpu().numpy(), mp.cpu().numpy(), rdt)
    groups = list(range(0, N, 16)) + [N]
    G, eps2 = 0.8, 1e-4
    rc, a, phi, p2p, m2pc, let = raw_h(hip, d, mp, 0, N, groups, order, G, eps2, h, let=True)
    orc, oa, ophi, op2p, om2p, olet = raw_gravity_let(hip, d, mp, 0, N, groups, order, G, eps2)
    assert rc == 0 and orc == 0
    assert same(p2p, op2p) and same(m2pc, om2p) and same(let, olet)
    tol = 1e-10 if rb == 64 else 5e-6
    worst, stats = 0.0, {}
    for lo, hi in zip(groups[:-1], groups[1:]):
        ra, rphi, rp2p, rm2p, rlet = walk_reference_let_h(t, lo, hi, order, G, eps2, h, stats)
        sl = slice(lo, hi)
        assert np.array_equal(p2p[sl], rp2p) and np.array_equal(m2pc[sl], rm2p) and np.array_equal(let[sl], rlet)
        scale = G * force_scale(xr, yr, zr, m, ns, np.arange(lo, hi), eps2)
        worst = max(worst, (np.linalg.norm(a[sl] - ra, axis=1) / scale).max(), (np.abs(phi[sl] - rphi) / np.abs(rphi)).max())
    share = stats["soft"] / stats["pairs"]
    print(f"rb={rb} order={order} {mac}: worst relative difference to the LET restatement with h {worst:.1e}; "
          f"{share:.1%} of the P2P pairs softened; targets that open the empty leaf {int((let > 0).sum())} of {N}")
    assert 0.05 <= share <= 0.5 and worst <= tol
    assert (let > 0).any() and not np.array_equal(phi, ophi)


def soft_grad_check(hip, tr, x, y, z, m, h, ctr, targets, eps2, rel_step):
    """grad_check of test_gravity_walk with h: -(central differences of phi) against a, every target shifted by
    +- step (rel_step * |target|) along x, y and z.  Returns per target |grad + a| (vector norm) and the counts check"""
    ns, nt = tr["n_src"], len(targets)
    step = rel_step * np.linalg.norm(targets, axis=1)
    groups = np.arange(ns, ns + nt + 1)

    def run(shift):
        pts = targets + shift
        xx, yy, zz = [np.concatenate([s, t]) for s, t in zip((x[:ns], y[:ns], z[:ns]), pts.T)]
        d = upload(hip, tr, xx, yy, zz, m, ctr)
        rc, a, phi, p2p, m2pc = raw_h(hip, d, upsweep(hip, d), ns, ns + nt, groups, 2, 1.0, eps2, h)
        assert rc == 0 and not np.isnan(a).any()
        return a, phi, (p2p, m2pc), pts

    a0, _, counts0, _ = run(np.zeros((nt, 3)))
    g = np.zeros((nt, 3))
    for k in range(3):
        e = np.zeros((nt, 3))
        e[:, k] = step
        _, pp, cp, xp = run(e)
        _, pm, cm, xm = run(-e)
        for c in (cp, cm):
            assert all(np.array_equal(u, v) for u, v in zip(c, counts0))
        g[:, k] = -(pp - pm) / (xp[:, k] - xm[:, k])
    return np.linalg.norm(g - a0, axis=1), a0


@pytest.mark.gpu
@pytest.mark.parametrize("eps2", [0.0, 0.01])
def test_softened_p2p_force_is_minus_the_gradient_of_its_potential(hip, eps2):
    """every node opened, the cloud (edge 1) centred at the origin, 16 targets each: 'inside' -- h = 3, every source
    within H; 'outside' -- at distance 1.5 with h = 0.05, no source within H; 'straddling' -- inside the cloud at
    distance 0.3 with h = 0.45, part of the sources within H.  The error is taken relative to the sum of the sizes of the
    force terms.  Bound: the truncation of the central difference (step / r)^2 = 1e-10 and the rounding of phi, 1e-16 /
    1e-5, as in test_p2p_force_is_minus_the_gradient_of_its_potential; a pair that crosses r2 = H^2 within the step sees
    the jump 3 G m / H^3 of the second derivative, an error of at most step * 3 G m / (2 H^3) against terms that sum to
    about n G m / r^2: with step = 3e-6, H = 0.46, r = 0.5 and n = 415 sources that is 3e-8 per crossing pair; 1e-7 is
    the bound for all three sets.  A wrong factor in the inside branch of the force or of w shows at 1e-2 and more"""
    tr = build_tree(three_level_desc())
    rng = np.random.default_rng(8)
    x, y, z, m = place_sources(tr, rng)
    ns = tr["n_src"]
    x, y, z = x - 0.5, y - 0.5, z - 0.5
    ctr = centers_of(tr, x, y, z, m, lambda n: HUGE_MAC)
    hs = rng.uniform(0.01, 0.04, ns)
    sets = dict(inside=(0.2, 3.0), outside=(1.5, 0.05), straddling=(0.3, 0.45))
    tg = np.concatenate([r * directions(16) for r, _ in sets.values()])
    ht = np.concatenate([np.full(16, v) for _, v in sets.values()])
    mm = np.concatenate([m, np.zeros(len(tg))])
    h = np.concatenate([hs, ht])
    diff, a0 = soft_grad_check(hip, tr, x, y, z, mm, h, ctr, tg, eps2, 1e-5)
    xx, yy, zz = [np.concatenate([s, t]) for s, t in zip((x, y, z), tg.T)]
    ra, rphi, mag, _ = direct_sum_h(xx, yy, zz, mm, h, np.arange(ns, ns + len(tg)), eps2=eps2, sizes=True)
    assert np.allclose(a0, ra, rtol=0, atol=1e-12 * np.linalg.norm(mag[:, :3], axis=1).max())
    r2 = (xx[None, :ns] - tg[:, 0, None]) ** 2 + (yy[None, :ns] - tg[:, 1, None]) ** 2 + \
         (zz[None, :ns] - tg[:, 2, None]) ** 2 + eps2
    within = (r2 < (ht[:, None] + hs[None, :]) ** 2).mean(1).reshape(3, 16)
    assert (within[0] == 1).all() and (within[1] == 0).all() and (within[2] > 0.1).all() and (within[2] < 0.9).all()
    rel = (diff / np.linalg.norm(mag[:, :3], axis=1)).reshape(3, 16)
    for k, name in enumerate(sets):
        print(f"P2P with h, eps2 {eps2}, {name}: worst |grad + a| / sum |terms| {rel[k].max():.1e}")
    assert rel.max() <= 1e-7


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the direct sum
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def direct_case(n, rb, mb):
    """a uniform cube of n particles with h in [0.05, 0.25], rounded to the types of the case, and its references
    (float64, from the rounded values) for all n targets with and without h: computed once per shape and shared"""
    rng = np.random.default_rng(70 + n)
    rdt, mdt = np_real(rb), np_real(mb)
    x, y, z = [a.astype(rdt) for a in rng.uniform(0, 1, (3, n))]
    m = rng.uniform(0.5, 1.5, n).astype(mdt)
    h = rng.uniform(0.05, 0.25, n).astype(rdt)
    G, eps2 = 0.7, 1e-4
    refs = {}
    for key, hh in (("h", h), ("plain", None)):
        a, phi, mag, soft = direct_sum_h(x, y, z, m, hh, np.arange(n), G, eps2, sizes=True)
        refs[key] = (np.concatenate([a, phi[:, None]], 1), mag, soft)
    for v in (x, y, z, m, h):
        v.setflags(write=False)
    return dict(n=n, x=x, y=y, z=z, m=m, h=h, G=G, eps2=eps2, refs=refs)


def gpu_direct(hip, c, dev, use_h, targets=None, first=0, last=None, segs=0, potential=True):
    """(ax, ay, az, phi) of Context.direct_gravity as one (nt, 4) float64 array (phi column NaN without potential)"""
    import torch

    tg = None if targets is None else torch.from_numpy(np.asarray(targets, dtype=np.int32)).cuda()
    out = hip.direct_gravity(dev["x"], dev["y"], dev["z"], dev["m"], dev["h"] if use_h else None, first=first,
                             last=last, targets=tg, num_segments=segs, G=c["G"], eps2=c["eps2"], potential=potential)
    hip.sync()
    cols = [t.cpu().numpy().astype(np.float64) for t in out[:3]]
    cols.append(out[3].cpu().numpy().astype(np.float64) if potential else np.full(cols[0].shape, np.nan))
    return np.stack(cols, 1)


def to_device(c):
    import torch

    return {k: torch.from_numpy(np.array(c[k])).cuda() for k in ("x", "y", "z", "m", "h")}


def unit_roundoff(rb):
    return 2.0 ** -53 if rb == 64 else 2.0 ** -24


@pytest.mark.gpu
@pytest.mark.parametrize("rb,mb", TYPES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 300, 2000])
def test_direct_sum_against_the_restatement(hip, n, rb, mb):
    """every output of cstone_hip_direct_gravity within (n + 16) u sum |term| of direct_sum_h, with and without h, for
    num_segments = 0, 1, 2, 7 and more than ceil(n / 64), for a target range, a sub-range and a shuffled target list
    with a duplicate, with and without phi; two identical calls give the same bits"""
    c = direct_case(n, rb, mb)
    dev = to_device(c)
    u = unit_roundoff(rb)
    rng = np.random.default_rng(n)
    tiles = (n + 63) // 64
    lst = rng.permutation(n)[:max(1, (2 * n) // 3)]
    lst = np.concatenate([lst, lst[:1]])  # a duplicate
    rng.shuffle(lst)
    lo, hi = n // 3, n - n // 5
    worst = 0.0
    for use_h in (True, False):
        ref, mag, soft = c["refs"]["h" if use_h else "plain"]
        if use_h and n >= 300:
            share = soft / (n * (n - 1))
            assert 0.05 <= share <= 0.5, share  # (9 % for the uniform cube with h in [0.05, 0.25])
        bound = (n + 16) * u * mag
        for segs in (0, 1, 2, 7, tiles + 3):
            got = gpu_direct(hip, c, dev, use_h, segs=segs)
            assert got.shape == (n, 4)
            err = np.abs(got - ref)
            assert (err <= bound).all(), (use_h, segs, np.max(err / np.maximum(bound, 1e-300)))
            worst = max(worst, np.max(err[bound > 0] / bound[bound > 0], initial=0.0))
            sub = gpu_direct(hip, c, dev, use_h, first=lo, last=hi, segs=segs)
            assert sub.shape == (hi - lo, 4) and (np.abs(sub - ref[lo:hi]) <= bound[lo:hi]).all()
            pick = gpu_direct(hip, c, dev, use_h, targets=lst, segs=segs)
            assert pick.shape == (lst.size, 4) and (np.abs(pick - ref[lst]) <= bound[lst]).all()
            if segs in (0, 7):
                assert np.array_equal(gpu_direct(hip, c, dev, use_h, targets=lst, segs=segs), pick)
                assert np.array_equal(gpu_direct(hip, c, dev, use_h, segs=segs), got)
                # a range and the list of its indices take the same sums
                assert np.array_equal(gpu_direct(hip, c, dev, use_h, targets=np.arange(lo, hi), segs=segs), sub)
                nophi = gpu_direct(hip, c, dev, use_h, segs=segs, potential=False)
                assert np.array_equal(nophi[:, :3], got[:, :3])
        if n == 1:
            assert (got == 0).all()
    print(f"n={n} rb={rb} mb={mb}: worst |error| / bound {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("rb,mb", [(64, 64), (32, 32)])
@pytest.mark.parametrize("n", [300, 2000])
def test_direct_sum_conserves_momentum(hip, n, rb, mb):
    """|sum_i m_i a_i| over all targets stays within sum_i m_i bound_i, componentwise: the exact sum vanishes because the
    rule is symmetric in i and j"""
    c = direct_case(n, rb, mb)
    dev = to_device(c)
    mag = c["refs"]["h"][1]
    got = gpu_direct(hip, c, dev, True)
    w = c["m"].astype(np.float64)[:, None]
    total = np.abs((w * got[:, :3]).sum(0))
    limit = ((n + 16) * unit_roundoff(rb) * w * mag[:, :3]).sum(0)
    print(f"n={n} rb={rb}: |sum m a| / summed bound {np.max(total / limit):.3f}")
    assert (total <= limit).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rb,mb", TYPES)
def test_walk_with_every_node_opened_agrees_with_the_direct_sum(hip, rb, mb):
    """HUGE_MAC: the walk is the direct sum over the leaves' particles in another order, so compute_gravity_h and
    cstone_hip_direct_gravity differ by at most the sum of both bounds, 2 (n + 16) u sum |term|, with and without h"""
    import torch

    tr = build_tree(three_level_desc())
    rng = np.random.default_rng(80)
    x, y, z, m = place_sources(tr, rng)
    n = tr["n_src"]
    rdt, mdt = np_real(rb), np_real(mb)
    xr, yr, zr = [a.astype(rdt) for a in (x, y, z)]
    m = m.astype(mdt).astype(np.float64)
    h = distinct_h(n, 81, large=(0.1, 0.25)).astype(rdt)
    ctr = centers_of(tr, xr.astype(np.float64), yr.astype(np.float64), zr.astype(np.float64), m, lambda k: HUGE_MAC)
    d = upload(hip, tr, xr, yr, zr, m, ctr, rb, mb)
    mp = upsweep(hip, d)
    groups = list(range(0, n, 64)) + [n]
    G, eps2 = 0.7, 1e-4
    for hh in (h, None):
        rc, a, phi, p2p, m2pc = raw_h(hip, d, mp, 0, n, groups, 2, G, eps2, hh)
        assert rc == 0 and (p2p == n - 1).all() and (m2pc == 0).all()
        hd = None if hh is None else torch.from_numpy(hh).cuda()
        out = hip.direct_gravity(d["x"], d["y"], d["z"], d["m"], hd, G=G, eps2=eps2)
        direct = np.stack([t.cpu().numpy().astype(np.float64) for t in out], 1)
        _, _, mag, soft = direct_sum_h(xr, yr, zr, m, hh, np.arange(n), G, eps2, sizes=True)
        if hh is not None:
            assert 0.05 <= soft / (n * (n - 1)) <= 0.5
        bound = 2 * (n + 16) * unit_roundoff(rb) * mag
        err = np.abs(np.concatenate([a, phi[:, None]], 1) - direct)
        print(f"rb={rb} mb={mb} h={'yes' if hh is not None else 'no'}: worst |walk - direct| / bound "
              f"{np.max(err / bound):.3f}")
        assert (err <= bound).all()


@pytest.mark.gpu
def test_direct_sum_refuses_bad_arguments_and_writes_nothing(hip):
    import torch

    from cstone_amd import _ptr

    c = direct_case(300, 64, 64)
    dev = to_device(c)
    n = 300
    good = dict(rb=64, mb=64, n=n, first=0, last=n, targets=None, nt=0, segs=0)
    tg_bad = torch.tensor([5, 7, n, 2], dtype=torch.int32, device="cuda")
    tg_ok = torch.tensor([5, 7, n - 1, 2], dtype=torch.int32, device="cuda")
    cases = [dict(rb=16), dict(mb=48), dict(first=10, last=9), dict(last=n + 1), dict(targets=tg_bad, nt=4),
             dict(segs=-1), dict(targets=tg_bad, nt=4, segs=3)]

    def call(kw):
        k = dict(good, **kw)
        outs = [torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4)]
        rc = hip.lib.cstone_hip_direct_gravity(
            hip.h, C.c_int(k["rb"]), C.c_int(k["mb"]), _ptr(dev["x"]), _ptr(dev["y"]), _ptr(dev["z"]), _ptr(dev["m"]),
            _ptr(dev["h"]), C.c_uint32(k["n"]), C.c_uint32(k["first"]), C.c_uint32(k["last"]), _ptr(k["targets"]),
            C.c_uint32(k["nt"]), C.c_int(k["segs"]), C.c_double(1.0), C.c_double(0.0), *[_ptr(t) for t in outs])
        hip.sync()
        return rc, torch.stack(outs).cpu().numpy()

    for kw in cases:
        rc, out = call(kw)
        assert rc == E_ARG and np.isnan(out).all(), kw
    rc, out = call(dict(targets=tg_ok, nt=4))
    assert rc == 0 and np.isfinite(out[:, :4]).all() and np.isnan(out[:, 4:]).all()
    rc, out = call(dict(first=7, last=7))  # an empty range is no error
    assert rc == 0 and np.isnan(out).all()
    rc, out = call({})
    assert rc == 0 and np.isfinite(out).all()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: through the Domain
# ---------------------------------------------------------------------------------------------------------------------
def domain_h(xd, seed):
    """a distinct softening length per particle of a synced domain, around the mean spacing of 5 000 particles"""
    import torch

    n = xd.numel()
    h = np.random.default_rng(seed).uniform(0.005, 0.04, n)
    return torch.from_numpy(h).cuda().to(xd.dtype)


@pytest.mark.gpu
def test_domain_gravity_with_h_equals_compute_gravity_h_and_refuses(hip):
    """Domain.gravity(h=...) after sync_grav = compute_gravity(h=...) on the domain's arrays bit for bit, Domain.gravity
    without h = the call of the old entry point; the refusals (before sync_grav, after a plain sync, a periodic box) are
    CSTONE_E_ARG with h as without"""
    import torch

    import cstone_amd
    from cstone_amd import CstoneError
    from cstone_amd.domain import Domain

    x, y, z, m = clustered_cloud(5000, 15)
    for rb in (64, 32):
        dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, rb, 32, bucket_focus=16)
        hd = domain_h(xd, 90)
        s = tree_state(hip, dom, xd, yd, zd, md)
        groups = groups_of(hip, s, xd, yd, zd)
        d = s["dev"]
        n = s["view"].end_index
        for order in (0, 2):
            for h in (hd, None):
                want = hip.compute_gravity(xd, yd, zd, md, 0, n, groups, s["view"].box, d["child_offsets"],
                                           d["internal_to_leaf"], d["layout"], d["centers"], d["multipoles"], order=order,
                                           G=2.0, eps2=1e-4, h=h)
                got = dom.gravity(xd, yd, zd, md, G=2.0, eps=1e-2, order=order, h=h)
                assert all(torch.equal(u, w) for u, w in zip(got, want[:4])), (rb, order, h is None)
            plain = gpu_gravity(hip, s, xd, yd, zd, md, groups, order=order, G=2.0, eps2=1e-4, counts=False)
            assert np.array_equal(got[3].cpu().numpy().astype(np.float64), plain[1])  # (got: the call without h)
            soft = dom.gravity(xd, yd, zd, md, G=2.0, eps=1e-2, order=order, h=hd)
            assert not torch.equal(soft[3], got[3])
        assert dom.gravity(xd, yd, zd, md, potential=False, h=hd)[3] is None
        nn = xd.numel()
        t = [a.clone() for a in (xd, yd, zd)]
        keys = torch.zeros(nn, dtype=torch.int64, device="cuda")
        dom.sync(keys, *t, torch.full_like(t[0], 0.01), [torch.empty_like(t[0]) for _ in range(3)])
        with pytest.raises(CstoneError, match=r"\(-1\)"):
            dom.gravity(*t, md, h=hd)
    fresh = Domain(hip, cstone_amd.HILBERT, 64, 64, 1024, 64, 0.5, cstone_amd.make_cbox([0, 1] * 3))
    xd = torch.from_numpy(x).cuda()
    with pytest.raises(CstoneError, match=r"\(-1\)"):
        fresh.gravity(xd, xd, xd, xd, h=xd)
    pdom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, bc=(1, 1, 1))
    with pytest.raises(CstoneError, match=r"\(-1\)"):
        pdom.gravity(xd, yd, zd, md, h=domain_h(xd, 91))


# Softened walk against the softened direct sum on the GPU (5 000 particles, theta = 0.5, f64, all targets; relative
# |da| and |dphi|, median / p99); the figures of the MI355X are in DESIGN.md section 7d.  The bounds are those of
# check_against_direct_sum in test_gravity_walk.py: M2P is not softened, so h must stay below the distance at which the
# MAC accepts a node, which it does here by an order of magnitude.
@pytest.mark.gpu
@pytest.mark.parametrize("cloud", ["clustered", "uniform"])
def test_accuracy_of_the_softened_walk_against_the_softened_direct_sum(hip, cloud):
    n = 5000
    x, y, z, m = clustered_cloud(n, 93) if cloud == "clustered" else uniform_cloud(n, 93)
    dom, xd, yd, zd, md = grav_domain(hip, x, y, z, m, theta=0.5, bucket_focus=16)
    hd = domain_h(xd, 94) if cloud == "uniform" else domain_h(xd, 94) / 4  # (the blobs are 40 times denser)
    ref = hip.direct_gravity(xd, yd, zd, md, hd, eps2=1e-6)
    plain = hip.direct_gravity(xd, yd, zd, md, None, eps2=1e-6)
    ra = np.stack([t.cpu().numpy() for t in ref[:3]], 1)
    rphi = ref[3].cpu().numpy()
    # the softening is no rounding matter on this cloud
    changed = np.abs(rphi - plain[3].cpu().numpy()) / np.abs(rphi)
    assert np.median(changed) > 1e-4, np.median(changed)
    fig = {}
    for order in (0, 2):
        got = dom.gravity(xd, yd, zd, md, eps=1e-3, order=order, h=hd)
        a = np.stack([t.cpu().numpy() for t in got[:3]], 1)
        e, ep = rel_err(a, ra), np.abs(got[3].cpu().numpy() - rphi) / np.abs(rphi)
        fig[order] = (np.median(e), np.percentile(e, 99), np.median(ep), np.percentile(ep, 99))
        print(f"{cloud}, softened, order {order}: |da| median {fig[order][0]:.1e} p99 {fig[order][1]:.1e}; |dphi| median "
              f"{fig[order][2]:.1e} p99 {fig[order][3]:.1e} (median relative change of phi by h {np.median(changed):.1e})")
    assert fig[2][0] < fig[0][0]
    assert fig[2][0] <= 1e-3 and fig[2][1] <= 1e-2 and fig[2][2] <= 1e-3 and fig[2][3] <= 1e-2


# ---------------------------------------------------------------------------------------------------------------------
# GPU, several ranks
# ---------------------------------------------------------------------------------------------------------------------
def _launch(nproc, port, particles=24000, timeout=900):
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "gravity_soft_mr_worker.py"),
           "--particles", str(particles)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("GRAV_RESULT ")]
    assert lines, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(lines[-1][len("GRAV_RESULT "):])
    print(json.dumps(res))
    assert p.returncode == 0 and res["ok"], str(res["bad"])[:3000] + p.stderr[-2000:]
    assert res["ranks"] == nproc and len(res["figures"]) == nproc
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [1, 2, 3])
def test_softened_gravity_on_several_ranks(nproc):
    """NativeDistributedDomain.gravity(h=...) on 1, 2 and 3 gloo ranks that share the GPU, 24 000 particles: on every
    rank it is compute_gravity_let(h=...) on the domain's arrays bit for bit, sampled groups equal walk_reference_let
    extended by h (counts exactly), the h that the sync returned has its halo ranges filled (they hold the owners'
    values), and the errors against the softened direct sum over the WHOLE cloud (cstone_hip_direct_gravity) are of the
    size of the single-rank domain's on the same cloud: the worst rank within 2 x of it in each of the four figures, as
    the table of DESIGN.md section 7d shows for the unsoftened case.  One rank: bit-equal to the single-rank domain"""
    res = _launch(nproc, 29870 + nproc)
    rows = [f for rank in res["figures"] for f in rank]
    worst = [max(f["direct"][k] for f in rows) for k in range(4)]
    single = res["figures"][0][0]["single_rank"]
    print(f"{nproc} ranks, softened: |da| median {worst[0]:.1e} p99 {worst[1]:.1e}, |dphi| median {worst[2]:.1e} p99 "
          f"{worst[3]:.1e} (worst rank); single-rank domain {['%.1e' % v for v in single['direct']]}")
    for k in range(4):
        assert worst[k] <= 2 * single["direct"][k], (k, worst, single)
    if nproc == 1:
        assert single["bit_equal"]
    else:
        assert all(f["halos"] > 0 for f in rows)
