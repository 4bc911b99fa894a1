"""One rank of tests/test_gravity_mr.py: gravity on the multi-rank domain (cstone_hip_domain_mr_compute_gravity) checked on
every rank against the direct formula for the multipoles, the NumPy restatement of the walk with the LET rule, and the
direct sum over the whole cloud.  Started by `python -m torch.distributed.run`; the ranks talk over gloo and share the one
GPU.  Rank 0 prints one line `GRAV_RESULT {json}`: ok, the failed checks, and the figures of every rank.

A failed check is recorded and the rank goes on, so that no rank waits in a collective for one that has stopped."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cornerstone-octree_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_gravity import clustered_cloud, direct_sum, grav_domain, rel_err, uniform_cloud, walk_reference  # noqa: E402

MAX_LEVEL = 21  # 64-bit keys
THETA = 0.5


# ---------------------------------------------------------------------------------------------------------------------
# the restatement with the LET rule (tests/test_gravity_mr.py imports it from here)
# ---------------------------------------------------------------------------------------------------------------------
def let_centers(t):
    """the centres of t with the MAC radius^2 of every massive leaf WITHOUT particles replaced by NaN: `R2 < |NaN|` is
    false and `NaN == 0` is false, so walk_reference never opens and never skips such a leaf -- it takes its multipole
    whatever the target box, which is the LET rule of cstone_hip_compute_gravity_let (the nodes the MAC accepts anyway
    are multipoles with and without the rule)"""
    child, itl, layout = t["child_offsets"], t["internal_to_leaf"], np.asarray(t["layout"])
    ctr = np.array(t["centers"], copy=True)
    M = ctr.shape[0]
    leaf_nodes = np.nonzero(child[:M] == 0)[0]
    lf = itl[leaf_nodes]
    empty = layout[lf] == layout[lf + 1]
    massive = ctr[leaf_nodes, 3] != 0
    ctr[leaf_nodes[empty & massive], 3] = np.nan
    return ctr


def walk_reference_let(t, lo, hi, order, G=1.0, eps2=0.0):
    """(a, phi, p2p counts, m2p counts, let m2p counts) of the target group [lo, hi) as cstone_hip_compute_gravity_let
    walks it.  The last count is what the rule adds to the M2P count of the plain walk, in which an opened leaf without
    particles is a P2P over nothing"""
    if "centers_let" not in t:
        t["centers_let"] = let_centers(t)
    plain = walk_reference(t, lo, hi, order, G, eps2)
    a, phi, p2p, m2pc = walk_reference(dict(t, centers=t["centers_let"]), lo, hi, order, G, eps2)
    return a, phi, p2p, m2pc, m2pc - plain[3]


# ---------------------------------------------------------------------------------------------------------------------
# checks of one rank
# ---------------------------------------------------------------------------------------------------------------------
def node_key_ranges(prefixes):
    """[start, end) of the keys of every node from its placeholder-bit prefix (1 followed by 3 * level key bits)"""
    start, end, level = [], [], []
    for p in prefixes:
        p = int(p)
        lv = (p.bit_length() - 1) // 3
        s = (p - (1 << (3 * lv))) << (3 * (MAX_LEVEL - lv))
        start.append(s)
        end.append(s + (1 << (3 * (MAX_LEVEL - lv))))
        level.append(lv)
    return np.array(start, dtype=np.uint64), np.array(end, dtype=object), np.array(level)


def gather_cloud(r, m):
    """the assigned particles of every rank, concatenated in rank order (which is key order): keys, x, y, z, m as
    float64 / uint64 on the host, and the offset of this rank's particles in them"""
    st, en = r["start"], r["end"]
    mine = [r["keys"][st:en].cpu().numpy().view(np.uint64)] + [t[st:en].cpu().numpy().astype(np.float64)
                                                               for t in (r["x"], r["y"], r["z"], m)]
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, mine)
    offset = sum(p[0].size for p in parts[:dist.get_rank()])
    return [np.concatenate([p[k] for p in parts]) for k in range(5)], offset


def check_multipoles(dom, oc, cloud, lim, rb, bad, what):
    """check 3: M and Q of EVERY node of this rank's focus tree against the direct formula over all particles of the
    cloud whose keys lie in the node's key range, about the node's expansion centre; tolerance and scaling of
    test_upsweep_of_a_hand_built_tree.  Returns the worst relative |dQ| and the root's M"""
    keys, x, y, z, m = cloud
    X = np.stack([x, y, z], 1)
    mp = dom.multipoles()
    if mp is None:
        bad.append(f"{what}: no multipoles")
        return None, None
    got = mp.cpu().numpy().astype(np.float64)
    ctr = oc["expansion_centers"].cpu().numpy().astype(np.float64)
    start, end, level = node_key_ranges(oc["prefixes"].cpu().numpy().view(np.uint64))
    lo = np.searchsorted(keys, start)
    hi = np.array([keys.size if e >= (1 << 64) else np.searchsorted(keys, np.uint64(e)) for e in end])
    edge = min(lim[1] - lim[0], lim[3] - lim[2], lim[5] - lim[4])
    tol = 1e-10 if rb == 64 else 3e-4
    worst, fails = 0.0, []
    assert got.shape[0] == ctr.shape[0] == oc["num_nodes"]
    for n in range(oc["num_nodes"]):
        rg = slice(lo[n], hi[n])
        w = m[rg]
        M = w.sum()
        if abs(got[n, 0] - M) > tol * M:
            fails.append((n, "M", got[n, 0], M))
            continue
        if M == 0:
            if (got[n] != 0).any():
                fails.append((n, "massless", got[n].tolist()))
            continue
        d = X[rg] - ctr[n, :3]
        d2 = (d * d).sum(1)
        q = np.array([(w * (3 * d[:, a] * d[:, b] - (d2 if a == b else 0))).sum() for a, b in
                      ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
        scale = max(np.abs(q).max(), 1e-3 * M * (edge * 0.5 ** level[n]) ** 2)
        err = np.abs(got[n, 1:7] - q).max() / scale
        worst = max(worst, err)
        if err > tol or got[n, 7] != 0:
            fails.append((n, "Q", err))
    if fails:
        bad.append(f"{what}: {len(fails)} of {oc['num_nodes']} nodes off, first {fails[:3]}")
    total = m.sum()
    if abs(got[0, 0] - total) > tol * total:
        bad.append(f"{what}: root mass {got[0, 0]} cloud {total}")
    return worst, got[0, 0]


def local_state(dom, oc, r, m, rb):
    """what walk_reference reads, for this rank's arrays (halos included) and its focus tree"""
    rdt = np.float64 if rb == 64 else np.float32
    return dict(rdt=rdt, x=r["x"].cpu().numpy(), y=r["y"].cpu().numpy(), z=r["z"].cpu().numpy(), m=m.cpu().numpy(),
                centers=oc["expansion_centers"].cpu().numpy(), child_offsets=oc["child_offsets"].cpu().numpy(),
                internal_to_leaf=oc["internal_to_leaf"].cpu().numpy(),
                layout=oc["layout"].cpu().numpy().astype(np.int64), multipoles=dom.multipoles().cpu().numpy())


def check_walk(hip, dom, oc, r, m, got, rb, bad, what, G, eps):
    """check 4: the library's walk on this rank's tree against the restatement with the LET rule, for a seeded sample of
    40 groups plus the groups with the largest let_m2p_counts: counts exactly, a / phi to check_against_restatement's
    tolerance.  Also: Domain.gravity IS compute_gravity_let on the domain's arrays.  Returns (targets with
    let_m2p_counts > 0, worst relative difference)"""
    import cstone_amd

    st, en = r["start"], r["end"]
    v = dom.view()
    groups = hip.compute_group_splits(st, en, r["x"], r["y"], r["z"], oc["leaves"], oc["layout"], v.box, 64,
                                      cstone_amd.GRAVITY_GROUP_TOL)
    ax, ay, az, phi, p2p, m2pc, let = hip.compute_gravity_let(
        r["x"], r["y"], r["z"], m, st, en, groups, v.box, oc["child_offsets"], oc["internal_to_leaf"], oc["layout"],
        oc["expansion_centers"], dom.multipoles(), order=2, G=G, eps2=eps * eps, counts=True)
    hip.sync()
    for name, mine, theirs in zip("xyzp", (ax, ay, az, phi), got):
        if not torch.equal(mine, theirs[st:en]):
            bad.append(f"{what}: Domain.gravity differs from compute_gravity_let in {name}")
    a = np.stack([t.cpu().numpy().astype(np.float64) for t in (ax, ay, az)], 1)
    phi, p2p, m2pc, let = [t.cpu().numpy().astype(np.float64 if k == 0 else np.int64)
                           for k, t in enumerate((phi, p2p, m2pc, let))]
    s = local_state(dom, oc, r, m, rb)
    g = groups.cpu().numpy().astype(np.int64)
    if g[0] != st or g[-1] != en:
        bad.append(f"{what}: groups cover [{g[0]}, {g[-1]}), assigned [{st}, {en})")
    per_group = np.array([let[g[k] - st:g[k + 1] - st].max(initial=0) for k in range(g.size - 1)])
    picks = [k for k in np.argsort(-per_group)[:8] if per_group[k] > 0]
    rng = np.random.default_rng(1)
    sample = np.union1d(rng.choice(g.size - 1, min(40, g.size - 1), replace=False), np.asarray(picks, int))
    tol = 1e-10 if rb == 64 else 1e-4
    worst = 0.0
    for k in sample:
        ra, rphi, rp2p, rm2p, rlet = walk_reference_let(s, g[k], g[k + 1], 2, G=G, eps2=eps * eps)
        sl = slice(g[k] - st, g[k + 1] - st)
        if not (np.array_equal(p2p[sl], rp2p) and np.array_equal(m2pc[sl], rm2p) and np.array_equal(let[sl], rlet)):
            bad.append(f"{what}: counts of group {k} differ from the restatement")
            continue
        worst = max(worst, rel_err(a[sl], ra).max(), (np.abs(phi[sl] - rphi) / np.abs(rphi)).max())
    if not worst <= tol:
        bad.append(f"{what}: walk differs from the restatement by {worst:.2e}")
    return int((let > 0).sum()), worst, len(picks)


def errors_against_direct_sum(cloud, offset, a, phi, n_tg, seed, G, eps):
    """relative errors of a (n, 3) / phi (n) of this rank's assigned particles against the direct sum over the whole
    cloud, for a seeded sample of them"""
    _, x, y, z, m = cloud
    n = a.shape[0]
    tg = np.random.default_rng(seed).choice(n, min(n, n_tg), replace=False)
    ra, rphi = direct_sum(x, y, z, m, offset + tg, G=G, eps2=eps * eps)
    return rel_err(a[tg], ra), np.abs(phi[tg] - rphi) / np.abs(rphi)


def check_physics(cloud, offset, r, got, bad, what, G, eps, seed=3):
    """check 5: the bounds of check_against_direct_sum.  Returns [median |da|, p99 |da|, median |dphi|, p99 |dphi|]"""
    st, en = r["start"], r["end"]
    a = np.stack([t[st:en].cpu().numpy().astype(np.float64) for t in got[:3]], 1)
    phi = got[3][st:en].cpu().numpy().astype(np.float64)
    e, ep = errors_against_direct_sum(cloud, offset, a, phi, 256, seed + dist.get_rank(), G, eps)
    fig = [float(np.median(e)), float(np.percentile(e, 99)), float(np.median(ep)), float(np.percentile(ep, 99))]
    if not (fig[0] <= 1e-3 and fig[1] <= 1e-2 and fig[2] <= 1e-3 and fig[3] <= 1e-2):
        bad.append(f"{what}: errors against the direct sum {fig}")
    return fig


def make_domain(hip, rb, N, P, lim, bc=(0, 0, 0), halo_mode=None):
    import cstone_amd
    from cstone_amd.distributed import NativeDistributedDomain

    return NativeDistributedDomain(hip, cstone_amd.HILBERT, 64, rb, max(64, N // (100 * P)), 16, lim, bc,
                                   halo_mode=halo_mode, theta=THETA)


def initial_share(a, hip, rank, P):
    """this rank's random share of the seeded cloud as device tensors: x, y, z, h, m"""
    N = a.particles
    x, y, z, m = clustered_cloud(N, a.seed) if a.cloud == "clustered" else uniform_cloud(N, a.seed)
    mine = np.nonzero(np.random.default_rng(a.seed + 100).integers(0, P, N) == rank)[0]
    tdt = torch.float64 if a.real_bits == 64 else torch.float32
    dev = [torch.from_numpy(c[mine].copy()).cuda().to(tdt) for c in (x, y, z)]
    h = torch.full((mine.size,), 0.01, dtype=tdt, device="cuda")
    return dev + [h, torch.from_numpy(m[mine].copy()).cuda().to(tdt)]


# ---------------------------------------------------------------------------------------------------------------------
def run_checks(a, hip, rank, P):
    rb, N = a.real_bits, a.particles
    G, eps = 0.7, 1e-3
    bad, figs = [], []
    dom = make_domain(hip, rb, N, P, [0.0, 1.0] * 3)
    x, y, z, h, m = initial_share(a, hip, rank, P)
    for s_ in range(a.syncs):
        what = f"rank {rank} sync {s_}"
        r = dom.sync_grav(x, y, z, h, m)
        st, en = r["start"], r["end"]
        mm = r["m"]
        got = dom.gravity(r["x"], r["y"], r["z"], mm, G=G, eps=eps)
        oc = dom.octree()
        cloud, offset = gather_cloud(r, mm)
        worst_q, root_m = check_multipoles(dom, oc, cloud, r["lim"], rb, bad, what)
        let_targets, worst_walk, let_groups = check_walk(hip, dom, oc, r, mm, got, rb, bad, what, G, eps)
        fig = check_physics(cloud, offset, r, got, bad, what, G, eps)
        figs.append(dict(sync=s_, nodes=int(oc["num_nodes"]), targets=int(en - st), halos=int(r["x"].numel() - (en - st)),
                         worst_dq=worst_q, root_mass=root_m, let_targets=let_targets, let_groups_compared=let_groups,
                         worst_walk=worst_walk, direct=fig))
        if s_ == 0 and rank == 0:
            single = single_rank_figures(hip, cloud, rb, N, P, G, eps, got, r, bad)
            figs[-1]["single_rank"] = single
        if s_ + 1 < a.syncs:  # drift; the next sync moves particles between the ranks
            x, y, z, h, m = [r[c][st:en].clone() for c in ("x", "y", "z", "h", "m")]
            for c, k in zip((x, y, z), range(3)):
                c.add_(0.004 * torch.sin(7.0 * (x + k)))
    if a.recentre:
        # check 8: moved particles, update_expansion_centers, gravity, no sync in between: checks 3 and 5 again
        what = f"rank {rank} after update_expansion_centers"
        gen = torch.Generator(device="cuda").manual_seed(50 + rank)
        for c in (r["x"], r["y"], r["z"]):
            c[st:en] += 5e-4 * torch.randn(en - st, dtype=c.dtype, device="cuda", generator=gen)
        for c in (r["x"], r["y"], r["z"]):
            dom.exchange_halos(c)  # (the halo particles have moved on their owners)
        dom.update_expansion_centers(r["x"], r["y"], r["z"], mm)
        if dom.multipoles() is not None:
            bad.append(f"{what}: the multipoles of the old centres are still handed out")
        got = dom.gravity(r["x"], r["y"], r["z"], mm, G=G, eps=eps)
        oc = dom.octree()
        cloud, offset = gather_cloud(r, mm)
        worst_q, root_m = check_multipoles(dom, oc, cloud, r["lim"], rb, bad, what)
        fig = check_physics(cloud, offset, r, got, bad, what, G, eps)
        figs.append(dict(recentred=True, worst_dq=worst_q, root_mass=root_m, direct=fig))
        if P > 1:
            # the call order is a contract: masses whose halo ranges were never exchanged give NaN (or a failed check 5)
            # with the wrapper's mass exchange switched off, and pass with the default
            poisoned = mm.clone()
            poisoned[:st] = float("nan")
            poisoned[en:] = float("nan")
            halos = torch.tensor([poisoned.numel() - (en - st)])
            dist.all_reduce(halos)
            off = dom.gravity(r["x"], r["y"], r["z"], poisoned.clone(), G=G, eps=eps, exchange_masses=False)
            nan_local = torch.tensor([int(sum(int(torch.isnan(t[st:en]).sum()) for t in off))])
            dist.all_reduce(nan_local)
            trial = []
            check_physics(cloud, offset, r, [torch.nan_to_num(t) for t in off], trial, what, G, eps)
            failed = torch.tensor([len(trial)])
            dist.all_reduce(failed)
            if int(halos.item()) == 0:
                bad.append(f"{what}: no halos anywhere, the mass exchange is not exercised")
            elif int(nan_local.item()) == 0 and int(failed.item()) == 0:
                bad.append(f"{what}: NaN masses on the halo ranges went unnoticed without the mass exchange")
            on = dom.gravity(r["x"], r["y"], r["z"], poisoned, G=G, eps=eps)
            if not all(torch.equal(u[st:en], w[st:en]) for u, w in zip(on, got)):
                bad.append(f"{what}: with the default mass exchange the result differs from the one with exchanged masses")
            figs[-1]["nan_outputs_without_exchange"] = int(nan_local.item())
    return bad, figs


def single_rank_figures(hip, cloud, rb, N, P, G, eps, got, r, bad):
    """the single-rank Domain.gravity on the same cloud at the same theta: its errors against the direct sum for a seeded
    sample (figures to put beside the multi-rank ones) and, on one rank (check 6), its agreement with the multi-rank
    result"""
    _, x, y, z, m = cloud
    dom1, xd, yd, zd, md = grav_domain(hip, x, y, z, m, rb, rb, theta=THETA, bucket_focus=16,
                                       bucket=max(64, N // (100 * P)))
    ax, ay, az, phi = dom1.gravity(xd, yd, zd, md, G=G, eps=eps)
    a1 = np.stack([t.cpu().numpy().astype(np.float64) for t in (ax, ay, az)], 1)
    p1 = phi.cpu().numpy().astype(np.float64)
    xs, ys, zs, ms = [t.cpu().numpy().astype(np.float64) for t in (xd, yd, zd, md)]
    tg = np.random.default_rng(3).choice(N, min(N, 1024), replace=False)
    ra, rphi = direct_sum(xs, ys, zs, ms, tg, G=G, eps2=eps * eps)
    e, ep = rel_err(a1[tg], ra), np.abs(p1[tg] - rphi) / np.abs(rphi)
    out = dict(direct=[float(np.median(e)), float(np.percentile(e, 99)), float(np.median(ep)),
                       float(np.percentile(ep, 99))], focus_leaves=int(dom1.view().num_focus_leaves))
    if P == 1:
        st, en = r["start"], r["end"]
        a = np.stack([t[st:en].cpu().numpy().astype(np.float64) for t in got[:3]], 1)
        p = got[3][st:en].cpu().numpy().astype(np.float64)
        same_order = np.array_equal(xs, x) and np.array_equal(ys, y) and np.array_equal(zs, z)
        if not same_order:
            bad.append("one rank: the single-rank domain orders the cloud differently")
            return out
        tol = 1e-10 if rb == 64 else 1e-4
        worst = max(rel_err(a, a1).max(), (np.abs(p - p1) / np.abs(p1)).max())
        out["against_single_rank"] = float(worst)
        out["bit_equal"] = bool(np.array_equal(a, a1) and np.array_equal(p, p1))
        if not worst <= tol:
            bad.append(f"one rank: differs from the single-rank Domain.gravity by {worst:.2e}")
    return out


def run_errors(a, hip, rank, P):
    """check 9: every refusal is CSTONE_E_ARG on every rank, and the next collective call on the same domain works"""
    from cstone_amd import CstoneError
    from cstone_amd.distributed import NativeDistributedDomain

    rb, N = a.real_bits, a.particles
    bad, figs = [], []

    def refused(dom, arrays, what):
        try:
            dom.gravity(*arrays)
            bad.append(f"rank {rank}: {what}: gravity did not refuse")
        except CstoneError as e:
            if "(-1)" not in str(e):
                bad.append(f"rank {rank}: {what}: {e}")
        figs.append(what)

    # no expansion centres for the current tree: a plain sync
    dom = make_domain(hip, rb, N, P, [0.0, 1.0] * 3)
    x, y, z, h, m = initial_share(a, hip, rank, P)
    r = dom.sync(x, y, z, h, props=[m])
    refused(dom, (r["x"], r["y"], r["z"], r["props"][0]), "after a plain sync")
    r = dom.sync_grav(x, y, z, h, m)
    got = dom.gravity(r["x"], r["y"], r["z"], r["m"])
    if not all(bool(torch.isfinite(t[r["start"]:r["end"]]).all()) for t in got):
        bad.append(f"rank {rank}: gravity after the refusal is not finite")
    st, en = r["start"], r["end"]
    r2 = dom.sync(*[r[c][st:en].clone() for c in "xyzh"])  # ... and a plain sync drops the centres again
    refused(dom, (r2["x"], r2["y"], r2["z"], r2["h"]), "after sync_grav and a plain sync")
    # a periodic axis
    pdom = make_domain(hip, rb, N, P, [0.0, 1.0] * 3, bc=(1, 0, 0))
    xp = x.clamp(0.0, 1.0 - 1e-6)
    r = pdom.sync_grav(xp, y, z, h, m)
    refused(pdom, (r["x"], r["y"], r["z"], r["m"]), "periodic axis")
    r = pdom.sync_grav(xp, y, z, h, m)
    pdom.exchange_halos(r["m"])
    # owner-side halos
    odom = make_domain(hip, rb, N, P, [0.0, 1.0] * 3, halo_mode=NativeDistributedDomain.HALOS_OWNER_SIDE)
    r = odom.sync(x, y, z, h, props=[m])
    refused(odom, (r["x"], r["y"], r["z"], r["props"][0]), "owner-side halos")
    r = odom.sync(x, y, z, h, props=[m])
    odom.exchange_halos(r["props"][0])
    return bad, figs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="checks", choices=["checks", "errors"])
    ap.add_argument("--particles", type=int, default=24000)
    ap.add_argument("--real-bits", type=int, default=64)
    ap.add_argument("--cloud", default="clustered", choices=["clustered", "uniform"])
    ap.add_argument("--syncs", type=int, default=1)
    ap.add_argument("--recentre", type=int, default=0)
    ap.add_argument("--seed", type=int, default=31)
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, P = dist.get_rank(), dist.get_world_size()
    import cstone_amd

    torch.cuda.set_device(0)
    hip = cstone_amd.Context(0)
    try:
        bad, figs = (run_checks if a.mode == "checks" else run_errors)(a, hip, rank, P)
    except Exception as e:  # (the other ranks may now wait in a collective: the launcher's timeout ends them)
        import traceback

        traceback.print_exc()
        print("GRAV_RESULT " + json.dumps(dict(ok=False, ranks=P, bad=[f"rank {rank}: {type(e).__name__}: {e}"], figures=[])),
              flush=True)
        os._exit(1)
    allbad, allfigs = [None] * P, [None] * P
    dist.all_gather_object(allbad, bad)
    dist.all_gather_object(allfigs, figs)
    flat = [b for part in allbad for b in part]
    if rank == 0:
        print("GRAV_RESULT " + json.dumps(dict(ok=not flat, ranks=P, bad=flat[:20], figures=allfigs), default=float),
              flush=True)
    dist.destroy_process_group()
    sys.exit(0 if not flat else 1)


if __name__ == "__main__":
    main()
