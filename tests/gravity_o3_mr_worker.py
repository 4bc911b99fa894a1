"""One rank of tests/test_gravity_o3.py::test_order_3_gravity_on_several_ranks: gravity at order 3 on the multi-rank
domain (cstone_hip_domain_mr_compute_gravity with order == 3, FocusLet::updateMultipoles with its doubled exchanges),
checked on every rank against the direct formula for the octupoles over the whole cloud, compute_gravity_o3 with the LET
rule on the domain's arrays, the NumPy restatement, and the direct sum over the whole cloud on the GPU
(cstone_hip_direct_gravity).  Started by `python -m torch.distributed.run`; the ranks talk over gloo and share the one
GPU.  Rank 0 prints one line `GRAV_RESULT {json}`.

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

from gravity_mr_worker import THETA, gather_cloud, local_state, make_domain, node_key_ranges  # noqa: E402
from test_gravity import clustered_cloud, grav_domain, rel_err  # noqa: E402
from test_gravity_o3 import F64_TOL, octupole_tensor, pack, walk_reference_o3  # noqa: E402

G, EPS = 0.7, 1e-3


def figures(e, ep):
    return [float(np.median(e)), float(np.percentile(e, 99)), float(np.median(ep)), float(np.percentile(ep, 99))]


def check_octupoles(dom, oc, cloud, lim, bad, what):
    """the seven components of EVERY node of this rank's focus tree against the direct formula over all particles of the
    cloud whose keys lie in the node's key range, about the node's expansion centre; relative to 15 sum m |d|^3 (floor
    M edge^3 / 1000), slot 7 and massless nodes exactly 0.  Returns the worst value"""
    keys, x, y, z, m = cloud
    X = np.stack([x, y, z], 1)
    got = dom.octupoles()
    if got is None:
        bad.append(f"{what}: no octupoles")
        return None
    got = got.cpu().numpy().astype(np.float64)
    ctr = oc["expansion_centers"].cpu().numpy().astype(np.float64)
    start, end, level = node_key_ranges(oc["prefixes"].cpu().numpy().view(np.uint64))
    lo = np.searchsorted(keys, start)
    hi = np.array([keys.size if e >= (1 << 64) else np.searchsorted(keys, np.uint64(e)) for e in end])
    edge = min(lim[1] - lim[0], lim[3] - lim[2], lim[5] - lim[4])
    worst, fails = 0.0, []
    if got.shape[0] != oc["num_nodes"]:
        bad.append(f"{what}: {got.shape[0]} octupoles for {oc['num_nodes']} nodes")
        return None
    for n in range(oc["num_nodes"]):
        rg = slice(lo[n], hi[n])
        w = m[rg]
        M = w.sum()
        if M == 0:
            if (got[n] != 0).any():
                fails.append((n, "massless", got[n].tolist()))
            continue
        d = X[rg] - ctr[n, :3]
        want = pack(octupole_tensor(d, w))
        scale = max(15.0 * (w * np.linalg.norm(d, axis=1) ** 3).sum(), 1e-3 * M * (edge * 0.5 ** level[n]) ** 3)
        err = np.abs(got[n, :7] - want[:7]).max() / scale
        worst = max(worst, err)
        if err > F64_TOL or got[n, 7] != 0:
            fails.append((n, "O", err))
    if fails:
        bad.append(f"{what}: {len(fails)} of {oc['num_nodes']} octupoles off, first {fails[:3]}")
    return worst


def direct_errors(hip, cloud, targets, a, phi):
    """relative errors of a (k, 3) / phi (k) of the particles `targets` of the gathered cloud against the direct sum over
    the whole cloud on the GPU"""
    _, x, y, z, m = cloud
    dev = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in (x, y, z, m)]
    tg = torch.from_numpy(np.asarray(targets, dtype=np.int32)).cuda()
    out = hip.direct_gravity(*dev, targets=tg, G=G, eps2=EPS * EPS)
    hip.sync()
    ra = np.stack([t.cpu().numpy() for t in out[:3]], 1)
    rphi = out[3].cpu().numpy()
    return rel_err(a, ra), np.abs(phi - rphi) / np.abs(rphi)


def host(got, st, en):
    return (np.stack([t[st:en].cpu().numpy() for t in got[:3]], 1), got[3][st:en].cpu().numpy())


def run(a, hip, rank, P):
    import cstone_amd

    N = a.particles
    bad, figs = [], []
    what = f"rank {rank}"
    x, y, z, m = clustered_cloud(N, a.seed)
    mine = np.nonzero(np.random.default_rng(a.seed + 100).integers(0, P, N) == rank)[0]
    xs, ys, zs, ms = [torch.from_numpy(c[mine].copy()).cuda() for c in (x, y, z, m)]
    hs = torch.full((mine.size,), 0.01, dtype=torch.float64, device="cuda")
    dom = make_domain(hip, 64, N, P, [0.0, 1.0] * 3)
    r = dom.sync_grav(xs, ys, zs, hs, ms)
    st, en = r["start"], r["end"]
    mm = r["m"]
    before = dom.gravity(r["x"], r["y"], r["z"], mm, G=G, eps=EPS, order=2)
    if dom.octupoles() is not None:
        bad.append(f"{what}: octupoles handed out before the first order-3 call")
    got = dom.gravity(r["x"], r["y"], r["z"], mm, G=G, eps=EPS, order=3)
    oc = dom.octree()
    v = dom.view()
    cloud, offset = gather_cloud(r, mm)
    worst_do = check_octupoles(dom, oc, cloud, r["lim"], bad, what)
    if dom.octupoles() is None or dom.multipoles() is None:
        raise RuntimeError("no moments after gravity(order=3)")
    groups = hip.compute_group_splits(st, en, r["x"], r["y"], r["z"], oc["leaves"], oc["layout"], v.box, 64,
                                      cstone_amd.GRAVITY_GROUP_TOL)
    ax, ay, az, phi, p2p, m2pc, let = hip.compute_gravity_o3(
        r["x"], r["y"], r["z"], mm, st, en, groups, v.box, oc["child_offsets"], oc["internal_to_leaf"], oc["layout"],
        oc["expansion_centers"], dom.multipoles(), dom.octupoles(), let=True, G=G, eps2=EPS * EPS, counts=True)
    hip.sync()
    for name, u, w in zip("xyzp", (ax, ay, az, phi), got):
        if not torch.equal(u, w[st:en]):
            bad.append(f"{what}: Domain.gravity(order=3) differs from compute_gravity_o3(let=True) in {name}")
    av = np.stack([t.cpu().numpy() for t in (ax, ay, az)], 1)
    pv, p2p, m2pc, let = [t.cpu().numpy().astype(np.float64 if k == 0 else np.int64)
                          for k, t in enumerate((phi, p2p, m2pc, let))]
    # the order changes no decision: the counts of the order-2 LET walk on the same tree
    _, _, _, _, p2p2, m2p2, let2 = hip.compute_gravity_let(
        r["x"], r["y"], r["z"], mm, st, en, groups, v.box, oc["child_offsets"], oc["internal_to_leaf"], oc["layout"],
        oc["expansion_centers"], dom.multipoles(), order=2, G=G, eps2=EPS * EPS, counts=True)
    hip.sync()
    if not all(np.array_equal(u, w.cpu().numpy()) for u, w in zip((p2p, m2pc, let), (p2p2, m2p2, let2))):
        bad.append(f"{what}: the counts at order 3 differ from those at order 2")
    s = local_state(dom, oc, r, mm, 64)
    s["octupoles"] = dom.octupoles().cpu().numpy()
    g = groups.cpu().numpy().astype(np.int64)
    per_group = np.array([let[g[k] - st:g[k + 1] - st].max(initial=0) for k in range(g.size - 1)])
    picks = [k for k in np.argsort(-per_group)[:6] if per_group[k] > 0]
    sample = np.union1d(np.random.default_rng(1).choice(g.size - 1, min(24, g.size - 1), replace=False),
                        np.asarray(picks, int))
    worst = 0.0
    for k in sample:
        ra, rphi, rp2p, rm2p, rlet = walk_reference_o3(s, g[k], g[k + 1], 3, G, EPS * EPS, True)
        sl = slice(g[k] - st, g[k + 1] - st)
        if not (np.array_equal(p2p[sl], rp2p) and np.array_equal(m2pc[sl], rm2p) and np.array_equal(let[sl], rlet)):
            bad.append(f"{what}: counts of group {k} differ from the restatement")
            continue
        worst = max(worst, rel_err(av[sl], ra).max(), (np.abs(pv[sl] - rphi) / np.abs(rphi)).max())
    if not worst <= F64_TOL:
        bad.append(f"{what}: walk differs from the restatement by {worst:.2e}")
    # the accuracy of both orders against the direct sum over the whole cloud, on the same targets
    tg = np.random.default_rng(3 + rank).choice(en - st, min(en - st, 512), replace=False)
    a2, p2 = host(before, st, en)
    fig3 = figures(*direct_errors(hip, cloud, offset + tg, av[tg], pv[tg]))
    fig2 = figures(*direct_errors(hip, cloud, offset + tg, a2[tg], p2[tg]))
    # order 2 again: the octupoles are gone and the result has the bits it had before any order-3 call
    after = dom.gravity(r["x"], r["y"], r["z"], mm, G=G, eps=EPS, order=2)
    if dom.octupoles() is not None:
        bad.append(f"{what}: octupoles still handed out after gravity(order=2)")
    if not all(torch.equal(u[st:en], w[st:en]) for u, w in zip(after, before)):
        bad.append(f"{what}: the order-2 result changed after an order-3 call")
    figs.append(dict(nodes=int(oc["num_nodes"]), targets=int(en - st), halos=int(r["x"].numel() - (en - st)),
                     worst_do=worst_do, worst_walk=worst, direct_order2=fig2, direct_order3=fig3,
                     let_targets=int((let > 0).sum()), let_groups_compared=len(picks)))
    if rank == 0 and P == 1:
        _, cx, cy, cz, cm = cloud
        dom1, xd, yd, zd, md = grav_domain(hip, cx, cy, cz, cm, 64, 64, theta=THETA, bucket_focus=16,
                                           bucket=max(64, N // (100 * P)))
        if not all(np.array_equal(t.cpu().numpy(), c) for t, c in zip((xd, yd, zd), (cx, cy, cz))):
            bad.append("the single-rank domain orders the cloud differently")
        else:
            a1, p1 = host(dom1.gravity(xd, yd, zd, md, G=G, eps=EPS, order=3), 0, N)
            figs[-1]["single_rank_bit_equal"] = bool(np.array_equal(av, a1) and np.array_equal(pv, p1))
            if not figs[-1]["single_rank_bit_equal"]:
                worst1 = max(rel_err(av, a1).max(), (np.abs(pv - p1) / np.abs(p1)).max())
                bad.append(f"one rank: differs from the single-rank Domain.gravity(order=3) by {worst1:.2e}")
    return bad, figs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=24000)
    ap.add_argument("--seed", type=int, default=31)
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, P = dist.get_rank(), dist.get_world_size()
    import cstone_amd

    torch.cuda.set_device(0)
    hip = cstone_amd.Context(0)
    try:
        bad, figs = run(a, hip, rank, P)
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
