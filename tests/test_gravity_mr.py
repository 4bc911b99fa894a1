"""Gravity on a locally essential tree and on several ranks: cstone_hip_compute_gravity_let (the walk's LET rule) on
hand-built trees, and cstone_hip_domain_mr_compute_gravity (multipoles of the whole LET through the global and the peer
exchange, then the LET walk) on 1-4 gloo ranks that share the GPU (tests/gravity_mr_worker.py).

The LET rule: a node that fails the MAC, has no children and has an empty particle range is applied as a multipole.

Figures of the multi-rank runs on the MI355X (24000 particles, theta = 0.5, order 2, G = 0.7, eps = 1e-3; relative
error against the direct sum over the whole cloud, worst rank; single rank = Domain.gravity on the same cloud):
see DESIGN.md section 7d."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gravity_mr_worker import walk_reference_let
from test_gravity import direct_sum, walk_reference
from test_gravity_walk import (HUGE_MAC, build_tree, centers_of, cube_of, force_scale, geometric_mac, place_sources,
                               raw_gravity, restatement_state, sources_only, upload, upsweep)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# three leaves hold no particles; the one at octant path (3, 2) is given a mass by hand, the other two stay massless
LET_DESC = [20, 30, 0, [5, 9, 0, 12, 0, 7, 3, 11], 40, 5, 15, 30]
REMOTE_MP = np.array([3.0, 0.020, -0.007, 0.004, -0.012, 0.009, -0.008, 0.0])  # M and a traceless Q (Qxx + Qyy + Qzz = 0)


def let_tree(mac, seed=41, extra=70):
    """the hand-built tree with a massive leaf that has an empty range: (tree, x, y, z, m, centres, remote node); `extra`
    targets that belong to no leaf follow the sources"""
    tr = build_tree(LET_DESC)
    rng = np.random.default_rng(seed)
    x, y, z, m = place_sources(tr, rng)
    x, y, z = [np.concatenate([a, rng.uniform(0, 1, extra)]) for a in (x, y, z)]
    m = np.concatenate([m, np.zeros(extra)])
    ctr = centers_of(tr, x, y, z, m, mac(tr))
    remote = int(tr["leaf_to_internal"][5])
    assert tr["paths"][remote] == (3, 2) and tr["lo"][remote] == tr["hi"][remote] and ctr[remote, 3] == 0
    c, s = cube_of(tr["paths"][remote])
    ctr[remote, :3] = c + s * np.array([0.4, 0.55, 0.6])
    ctr[remote, 3] = mac(tr)(remote)
    return tr, x, y, z, m, ctr, remote


def multipole_term(mp, c, X, G, eps2, order=2):
    """acceleration and potential of ONE multipole at the points X (k, 3), by the formula of include/cstone_hip.h:
    d = r_i - c, r^2 = |d|^2 + eps2, a = G [-M d / r^3 + Q d / r^5 - 5/2 (d.Q.d) d / r^7],
    phi = -G [M / r + 1/2 (d.Q.d) / r^5]; order 0 drops the Q terms"""
    M = mp[0]
    Q = np.array([[mp[1], mp[2], mp[3]], [mp[2], mp[4], mp[5]], [mp[3], mp[5], mp[6]]]) * (order == 2)
    a, phi = np.zeros((len(X), 3)), np.zeros(len(X))
    for i, r_i in enumerate(X):
        d = r_i - c
        r = np.sqrt(d @ d + eps2)
        dQd = d @ Q @ d
        a[i] = G * (-M * d / r ** 3 + Q @ d / r ** 5 - 2.5 * dQd * d / r ** 7)
        phi[i] = -G * (M / r + 0.5 * dQd / r ** 5)
    return a, phi


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement with the LET rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 2])
def test_restated_let_rule_adds_exactly_the_remote_multipole(order):
    """every node forced open: the walk with the rule is the direct sum over the particles that are present plus the
    empty leaf's multipole term by the header's formula; without the rule the same call misses exactly that term"""
    tr, x, y, z, m, ctr, remote = let_tree(lambda tr: (lambda n: HUGE_MAC))
    mp = np.zeros((tr["M"], 8))
    mp[remote] = REMOTE_MP
    t = restatement_state(tr, x, y, z, m, ctr, mp, np.float64)
    ns, N = tr["n_src"], x.size
    G, eps2 = 0.9, 1e-5
    X = np.stack([x, y, z], 1)
    for lo in range(0, N, 64):
        hi = min(N, lo + 64)
        a, phi, p2p, m2pc, let = walk_reference_let(t, lo, hi, order, G, eps2)
        pa, pphi, pp2p, pm2p = walk_reference(t, lo, hi, order, G, eps2)
        tg = np.arange(lo, hi)
        da, dphi = direct_sum(x, y, z, sources_only(m, ns), tg, G=G, eps2=eps2)
        ta, tphi = multipole_term(REMOTE_MP, ctr[remote, :3], X[tg], G, eps2, order)
        assert np.allclose(a, da + ta, rtol=1e-12, atol=0) and np.allclose(phi, dphi + tphi, rtol=1e-12, atol=0)
        assert (m2pc == 1).all() and (let == 1).all() and np.array_equal(p2p, np.where(tg < ns, ns - 1, ns))
        # without the rule: the same sum without the term, the leaf a P2P over nothing
        assert np.allclose(pa, da, rtol=1e-12, atol=0) and np.allclose(pphi, dphi, rtol=1e-12, atol=0)
        assert np.allclose(a - pa, ta, rtol=1e-9, atol=1e-12) and np.allclose(phi - pphi, tphi, rtol=1e-9, atol=1e-12)
        assert (pm2p == 0).all() and np.array_equal(pp2p, p2p)
        assert np.abs(ta).max() > 1e-2  # (the term is no rounding matter)


def test_restated_let_rule_leaves_other_trees_alone():
    """massless empty leaves (macSq = 0) are skipped with and without the rule, and a leaf the MAC accepts is one M2P
    either way: on a tree without a massive empty leaf the two restatements are the same"""
    tr = build_tree(LET_DESC)
    x, y, z, m = place_sources(tr, np.random.default_rng(42))
    ctr = centers_of(tr, x, y, z, m, geometric_mac(tr, 0.6))
    assert (np.diff(tr["layout"]) == 0).any()
    t = restatement_state(tr, x, y, z, m, ctr, np.random.default_rng(43).normal(size=(tr["M"], 8)), np.float64)
    for lo in range(0, tr["n_src"], 64):
        hi = min(tr["n_src"], lo + 64)
        *withrule, let = walk_reference_let(t, lo, hi, 2)
        for u, w in zip(withrule, walk_reference(t, lo, hi, 2)):
            assert np.array_equal(u, w)
        assert (let == 0).all()


def test_let_entry_points_are_exported():
    import cstone_amd

    lib = cstone_amd.load_library()
    for name in ("cstone_hip_compute_gravity_let", "cstone_hip_upsweep_multipoles_nodes",
                 "cstone_hip_domain_mr_compute_gravity", "cstone_hip_domain_mr_multipoles_get"):
        assert name in cstone_amd.EXPORTS and hasattr(lib, name)


# ---------------------------------------------------------------------------------------------------------------------
# GPU, one process: cstone_hip_compute_gravity_let on hand-built trees
# ---------------------------------------------------------------------------------------------------------------------
def raw_gravity_let(hip, d, mp, first, last, groups, order=2, G=1.0, eps2=0.0):
    """cstone_hip_compute_gravity_let called directly, like raw_gravity: (rc, a, phi, p2p, m2p, let_m2p)"""
    import torch

    import cstone_amd
    from cstone_amd import _ptr

    nt = last - first
    dt = d["x"].dtype
    ax, ay, az, phi = [torch.full((nt,), float("nan"), dtype=dt, device="cuda") for _ in range(4)]
    p2p, m2pc, let = [torch.full((nt,), -1, dtype=torch.int32, device="cuda") for _ in range(3)]
    g = torch.from_numpy(np.asarray(groups, dtype=np.int32)).cuda()
    box = cstone_amd.make_cbox([-4.0, 4.0] * 3)
    rc = hip.lib.cstone_hip_compute_gravity_let(
        hip.h, C.c_int(d["rb"]), C.c_int(d["mb"]), _ptr(d["x"]), _ptr(d["y"]), _ptr(d["z"]), _ptr(d["m"]),
        C.c_uint32(first), C.c_uint32(last), _ptr(g), C.c_uint32(g.numel() - 1), C.byref(box), _ptr(d["child_offsets"]),
        _ptr(d["internal_to_leaf"]), _ptr(d["layout"]), _ptr(d["centers"]), _ptr(mp), C.c_int(order), C.c_double(G),
        C.c_double(eps2), _ptr(ax), _ptr(ay), _ptr(az), _ptr(phi), _ptr(p2p), _ptr(m2pc), _ptr(let))
    hip.sync()
    a = np.stack([t.cpu().numpy().astype(np.float64) for t in (ax, ay, az)], 1)
    return (rc, a, phi.cpu().numpy().astype(np.float64), p2p.cpu().numpy().astype(np.int64),
            m2pc.cpu().numpy().astype(np.int64), let.cpu().numpy().astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("rb", [64, 32])
@pytest.mark.parametrize("mac", ["open", "geometric"])
def test_let_walk_of_a_hand_built_tree(hip, rb, order, mac):
    """a massive leaf with an empty range.  'open': every node opened, so every target opens that leaf: let_m2p_counts
    == m2p_counts == 1.  'geometric': near targets open it (the rule), far ones accept it by the MAC.  Counts equal the
    restatement with the rule exactly, a and phi to the tolerance of test_long_and_ragged_groups_and_sub_ranges; the
    old entry point still drops the leaf, as its restatement does"""
    import torch

    macf = (lambda tr: (lambda n: HUGE_MAC)) if mac == "open" else (lambda tr: geometric_mac(tr, 1.0))
    tr, x, y, z, m, ctr, remote = let_tree(macf)
    rdt = np.float64 if rb == 64 else np.float32
    xr, yr, zr = [a.astype(rdt) for a in (x, y, z)]
    m = m.astype(rdt).astype(np.float64)
    d = upload(hip, tr, xr, yr, zr, m, ctr, rb, rb)
    mp = upsweep(hip, d)
    assert float(mp[remote].abs().max()) == 0.0  # (no particles here: the upsweep alone leaves the leaf massless)
    mp[remote] = torch.from_numpy(REMOTE_MP.astype(rdt)).cuda()
    ns, N = tr["n_src"], x.size
    t = restatement_state(tr, xr, yr, zr, m, d["centers"].cpu().numpy(), mp.cpu().numpy(), rdt)
    groups = list(range(0, N, 16)) + [N]
    G, eps2 = 0.8, 1e-4
    rc, a, phi, p2p, m2pc, let = raw_gravity_let(hip, d, mp, 0, N, groups, order, G, eps2)
    orc, oa, ophi, op2p, om2p = raw_gravity(hip, d, mp, 0, N, groups, order, G, eps2)
    assert rc == 0 and orc == 0
    tol = 1e-10 if rb == 64 else 5e-6
    worst = worst_old = 0.0
    for lo, hi in zip(groups[:-1], groups[1:]):
        ra, rphi, rp2p, rm2p, rlet = walk_reference_let(t, lo, hi, order, G, eps2)
        pa, pphi, pp2p, pm2p = walk_reference(t, lo, hi, order, G, eps2)
        sl = slice(lo, hi)
        assert np.array_equal(p2p[sl], rp2p) and np.array_equal(m2pc[sl], rm2p) and np.array_equal(let[sl], rlet)
        assert np.array_equal(op2p[sl], pp2p) and np.array_equal(om2p[sl], pm2p)
        scale = G * force_scale(xr, yr, zr, m, ns, np.arange(lo, hi), eps2)
        worst = max(worst, (np.linalg.norm(a[sl] - ra, axis=1) / scale).max(), (np.abs(phi[sl] - rphi) / np.abs(rphi)).max())
        worst_old = max(worst_old, (np.linalg.norm(oa[sl] - pa, axis=1) / scale).max(),
                        (np.abs(ophi[sl] - pphi) / np.abs(pphi)).max())
    print(f"rb={rb} order={order} {mac}: worst relative difference to the LET restatement {worst:.1e}, of the old entry "
          f"point to the plain one {worst_old:.1e}; targets that open the empty leaf {int((let > 0).sum())} of {N}")
    assert worst <= tol and worst_old <= tol
    assert (let <= 1).all() and (let > 0).any()
    if mac == "open":
        assert (let == 1).all() and (m2pc == 1).all() and (om2p == 0).all()
    else:
        assert (let == 0).any() and (m2pc > let).any()
    # the leaf's mass is in the new result and not in the old one
    assert (np.abs(phi - ophi)[let > 0] > 1e-3 * np.abs(ophi)[let > 0]).all()
    assert np.array_equal(a[let == 0], oa[let == 0]) and np.array_equal(phi[let == 0], ophi[let == 0])


@pytest.mark.gpu
@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("rb", [64, 32])
def test_let_walk_equals_the_plain_walk_without_such_a_leaf(hip, rb, order):
    """on a tree whose empty leaves are all massless the new entry point equals the old one bit for bit in a, phi and
    both counts, and let_m2p_counts is zero everywhere"""
    tr = build_tree(LET_DESC)
    rng = np.random.default_rng(44)
    x, y, z, m = place_sources(tr, rng)
    ns, N = tr["n_src"], tr["n_src"] + 90
    x, y, z = [np.concatenate([a, rng.uniform(0, 1, N - ns)]) for a in (x, y, z)]
    m = np.concatenate([m, np.zeros(N - ns)])
    rdt = np.float64 if rb == 64 else np.float32
    xr, yr, zr = [a.astype(rdt) for a in (x, y, z)]
    ctr = centers_of(tr, xr.astype(np.float64), yr.astype(np.float64), zr.astype(np.float64), m, geometric_mac(tr, 0.6))
    assert (np.diff(tr["layout"]) == 0).any()
    d = upload(hip, tr, xr, yr, zr, m, ctr, rb, rb)
    mp = upsweep(hip, d)
    groups = [0, 50, 114, 115, 200, N]
    rc, a, phi, p2p, m2pc, let = raw_gravity_let(hip, d, mp, 7, N - 3, groups, order, 1.3, 1e-5)
    orc, oa, ophi, op2p, om2p = raw_gravity(hip, d, mp, 7, N - 3, groups, order, 1.3, 1e-5)
    assert rc == 0 and orc == 0
    assert np.array_equal(a, oa) and np.array_equal(phi, ophi) and not np.isnan(a).any()
    assert np.array_equal(p2p, op2p) and np.array_equal(m2pc, om2p) and (let == 0).all()
    assert (m2pc > 0).any() and (p2p > 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# GPU, several ranks
# ---------------------------------------------------------------------------------------------------------------------
def _launch(nproc, port, mode="checks", real_bits=64, cloud="clustered", syncs=1, recentre=0, particles=24000,
            timeout=900):
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "gravity_mr_worker.py"), "--mode", mode,
           "--real-bits", str(real_bits), "--cloud", cloud, "--syncs", str(syncs), "--recentre", str(recentre),
           "--particles", str(particles)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("GRAV_RESULT ")]
    assert lines, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(lines[-1][len("GRAV_RESULT "):])
    print(json.dumps(res))
    assert p.returncode == 0 and res["ok"], str(res["bad"])[:3000] + p.stderr[-2000:]
    assert res["ranks"] == nproc and len(res["figures"]) == nproc
    return res


def _summary(res, what):
    """one line per run: the worst rank's figures, the targets that took the LET rule"""
    rows = [f for rank in res["figures"] for f in rank if "direct" in f]
    worst = [max(f["direct"][k] for f in rows) for k in range(4)]
    let = sum(f.get("let_targets", 0) for f in rows)
    compared = sum(f.get("let_groups_compared", 0) for f in rows)
    single = next((f["single_rank"] for rank in res["figures"] for f in rank if "single_rank" in f), None)
    print(f"{what}: |da| median {worst[0]:.1e} p99 {worst[1]:.1e}, |dphi| median {worst[2]:.1e} p99 {worst[3]:.1e} (worst "
          f"rank); single rank {single['direct'] if single else None}; targets with let_m2p_counts > 0: {let} "
          f"({compared} of their groups compared with the restatement)")
    return let, single


MR_CASES = [
    # ranks, precision, cloud, syncs, update_expansion_centers + the mass-exchange contract
    (2, 64, "uniform", 1, 0),
    (2, 32, "clustered", 1, 1),
    (3, 64, "clustered", 3, 1),
    (4, 64, "clustered", 1, 0),
    (4, 64, "uniform", 1, 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,rb,cloud,syncs,recentre", MR_CASES)
def test_gravity_on_several_ranks(nproc, rb, cloud, syncs, recentre):
    """on every rank and after every sync: the multipoles of EVERY node of the focus tree equal the direct formula over
    the whole cloud (the root's M is the cloud's mass), the walk equals the restatement with the LET rule (counts
    exactly), Domain.gravity is that walk bit for bit, and the accelerations and potentials are within the bounds of
    check_against_direct_sum of the direct sum over the WHOLE cloud.  recentre: the same after moved particles and
    update_expansion_centers without a sync, and NaN masses on the halo ranges are caught unless the wrapper exchanges
    the masses"""
    res = _launch(nproc, 29850 + 10 * nproc + rb // 32 + (5 if cloud == "uniform" else 0), real_bits=rb, cloud=cloud,
                  syncs=syncs, recentre=recentre)
    _summary(res, f"{nproc} ranks f{rb} {cloud}")
    for rank in res["figures"]:
        assert len([f for f in rank if "sync" in f]) == syncs
        assert all(f["halos"] > 0 for f in rank if "sync" in f)
        if recentre:
            assert rank[-1].get("recentred")


@pytest.mark.gpu
def test_gravity_on_one_rank_equals_the_single_rank_domain():
    """a world of one rank: every check of the several-ranks test, and the result agrees with the single-rank
    Domain.gravity on the same cloud to the restatement's tolerance"""
    res = _launch(1, 29810, recentre=1)
    _, single = _summary(res, "1 rank f64 clustered")
    assert single is not None and "against_single_rank" in single
    print(f"one rank against the single-rank domain: worst relative difference {single['against_single_rank']:.1e}, "
          f"bit-equal: {single['bit_equal']}")


@pytest.mark.gpu
def test_gravity_refusals_on_several_ranks():
    """no expansion centres for the current tree, a periodic axis, owner-side halos: CSTONE_E_ARG on every rank before
    any collective, and the next collective call on the same domain works"""
    res = _launch(2, 29815, mode="errors", particles=12000)
    for rank in res["figures"]:
        assert rank == ["after a plain sync", "after sync_grav and a plain sync", "periodic axis", "owner-side halos"]
