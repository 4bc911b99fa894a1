"""One rank of tests/test_gravity_soft.py::test_softened_gravity_on_several_ranks: gravity with per-particle softening
lengths on the multi-rank domain (cstone_hip_domain_mr_compute_gravity_h), checked on every rank against
compute_gravity_let with h on the domain's arrays, the NumPy restatement with the LET rule and h, and the softened
direct sum over the whole cloud on the GPU (cstone_hip_direct_gravity).  Started by `python -m torch.distributed.run`;
the ranks talk over gloo and share the one GPU.  Rank 0 prints one line `GRAV_RESULT {json}`.

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

from gravity_mr_worker import THETA, gather_cloud, local_state, make_domain  # noqa: E402
from test_gravity import clustered_cloud, grav_domain, rel_err  # noqa: E402
from test_gravity_soft import walk_reference_let_h  # noqa: E402

G, EPS = 0.7, 1e-3
H_RANGE = (0.001, 0.008)  # around the spacing inside a blob of the clustered cloud of 24 000 (about 0.006)


def figures(e, ep):
    return [float(np.median(e)), float(np.percentile(e, 99)), float(np.median(ep)), float(np.percentile(ep, 99))]


def direct_errors(hip, cloud, hc, targets, a, phi):
    """relative errors of a (k, 3) / phi (k) of the particles `targets` of the gathered cloud against the softened direct
    sum over the whole cloud on the GPU"""
    _, x, y, z, m = cloud
    dev = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in (x, y, z, m, hc)]
    tg = torch.from_numpy(np.asarray(targets, dtype=np.int32)).cuda()
    out = hip.direct_gravity(*dev, targets=tg, G=G, eps2=EPS * EPS)
    hip.sync()
    ra = np.stack([t.cpu().numpy() for t in out[:3]], 1)
    rphi = out[3].cpu().numpy()
    return rel_err(a, ra), np.abs(phi - rphi) / np.abs(rphi)


def run(a, hip, rank, P):
    import cstone_amd

    N = a.particles
    bad, figs = [], []
    what = f"rank {rank}"
    x, y, z, m = clustered_cloud(N, a.seed)
    h = np.random.default_rng(a.seed + 7).uniform(*H_RANGE, N)
    mine = np.nonzero(np.random.default_rng(a.seed + 100).integers(0, P, N) == rank)[0]
    xs, ys, zs, hs, ms = [torch.from_numpy(c[mine].copy()).cuda() for c in (x, y, z, h, m)]
    dom = make_domain(hip, 64, N, P, [0.0, 1.0] * 3)
    r = dom.sync_grav(xs, ys, zs, hs, ms)
    st, en = r["start"], r["end"]
    mm, hh = r["m"], r["h"]
    got = dom.gravity(r["x"], r["y"], r["z"], mm, G=G, eps=EPS, h=hh)
    plain = dom.gravity(r["x"], r["y"], r["z"], mm, G=G, eps=EPS)
    if torch.equal(got[3][st:en], plain[3][st:en]):
        bad.append(f"{what}: h changes nothing")
    # the halo ranges of the sync's h hold the owners' values: repeating the exchange for h changes nothing
    hx = hh.clone()
    hx[:st] = float("nan")
    hx[en:] = float("nan")
    dom.exchange_halos(hx)
    if not torch.equal(hx, hh):
        bad.append(f"{what}: the sync left the halo ranges of h unfilled")
    oc = dom.octree()
    v = dom.view()
    groups = hip.compute_group_splits(st, en, r["x"], r["y"], r["z"], oc["leaves"], oc["layout"], v.box, 64,
                                      cstone_amd.GRAVITY_GROUP_TOL)
    ax, ay, az, phi, p2p, m2pc, let = hip.compute_gravity_let(
        r["x"], r["y"], r["z"], mm, st, en, groups, v.box, oc["child_offsets"], oc["internal_to_leaf"], oc["layout"],
        oc["expansion_centers"], dom.multipoles(), order=2, G=G, eps2=EPS * EPS, counts=True, h=hh)
    hip.sync()
    for name, u, w in zip("xyzp", (ax, ay, az, phi), got):
        if not torch.equal(u, w[st:en]):
            bad.append(f"{what}: Domain.gravity(h) differs from compute_gravity_let(h) in {name}")
    av = np.stack([t.cpu().numpy() for t in (ax, ay, az)], 1)
    pv, p2p, m2pc, let = [t.cpu().numpy().astype(np.float64 if k == 0 else np.int64)
                          for k, t in enumerate((phi, p2p, m2pc, let))]
    s = local_state(dom, oc, r, mm, 64)
    hn = hh.cpu().numpy()
    g = groups.cpu().numpy().astype(np.int64)
    stats, worst = {}, 0.0
    for k in np.random.default_rng(1).choice(g.size - 1, min(24, g.size - 1), replace=False):
        ra, rphi, rp2p, rm2p, rlet = walk_reference_let_h(s, g[k], g[k + 1], 2, G, EPS * EPS, hn, stats)
        sl = slice(g[k] - st, g[k + 1] - st)
        if not (np.array_equal(p2p[sl], rp2p) and np.array_equal(m2pc[sl], rm2p) and np.array_equal(let[sl], rlet)):
            bad.append(f"{what}: counts of group {k} differ from the restatement")
            continue
        worst = max(worst, rel_err(av[sl], ra).max(), (np.abs(pv[sl] - rphi) / np.abs(rphi)).max())
    if not worst <= 1e-10:
        bad.append(f"{what}: walk differs from the restatement with h by {worst:.2e}")
    # the whole cloud, in key order, with its h
    cloud, offset = gather_cloud(r, mm)
    parts = [None] * P
    dist.all_gather_object(parts, hn[st:en])
    hc = np.concatenate(parts)
    tg = np.random.default_rng(3 + rank).choice(en - st, min(en - st, 256), replace=False)
    e, ep = direct_errors(hip, cloud, hc, offset + tg, av[tg], pv[tg])
    fig = figures(e, ep)
    if not (fig[0] <= 1e-3 and fig[1] <= 1e-2 and fig[2] <= 1e-3 and fig[3] <= 1e-2):
        bad.append(f"{what}: errors against the softened direct sum {fig}")
    figs.append(dict(targets=int(en - st), halos=int(r["x"].numel() - (en - st)), worst_walk=worst, direct=fig,
                     soft_share=stats.get("soft", 0) / max(1, stats.get("pairs", 0)),
                     let_targets=int((let > 0).sum())))
    if not 0.001 <= figs[-1]["soft_share"] <= 0.5:
        bad.append(f"{what}: {figs[-1]['soft_share']:.2%} of the sampled P2P pairs softened")
    # h is read on the halo ranges: other values there change the result.  (The wrapper has no exchange of h to switch
    # off, the sync fills those ranges; and NaN would not do as a probe: r2 < NaN is false, the pair takes the Plummer
    # branch and the NaN is gone.)
    if P > 1:
        probe = hh.clone()
        probe[:st] = 10.0
        probe[en:] = 10.0
        out = dom.gravity(r["x"], r["y"], r["z"], mm, G=G, eps=EPS, h=probe)
        changed = torch.tensor([int((out[3][st:en] != got[3][st:en]).sum())])
        dist.all_reduce(changed)
        figs[-1]["outputs_changed_by_halo_h"] = int(changed.item())
        if int(changed.item()) == 0:
            bad.append(f"{what}: h on the halo ranges is not read")
    if rank == 0:
        _, cx, cy, cz, cm = cloud
        dom1, xd, yd, zd, md = grav_domain(hip, cx, cy, cz, cm, 64, 64, theta=THETA, bucket_focus=16,
                                           bucket=max(64, N // (100 * P)))
        same_order = all(np.array_equal(t.cpu().numpy(), c) for t, c in zip((xd, yd, zd), (cx, cy, cz)))
        if not same_order:
            bad.append("the single-rank domain orders the cloud differently")
        else:
            hd = torch.from_numpy(hc).cuda()
            one = dom1.gravity(xd, yd, zd, md, G=G, eps=EPS, h=hd)
            a1 = np.stack([t.cpu().numpy() for t in one[:3]], 1)
            p1 = one[3].cpu().numpy()
            t1 = np.random.default_rng(3).choice(N, min(N, 1024), replace=False)
            e, ep = direct_errors(hip, cloud, hc, t1, a1[t1], p1[t1])
            single = dict(direct=figures(e, ep))
            if P == 1:
                single["bit_equal"] = bool(np.array_equal(av, a1) and np.array_equal(pv, p1))
                if not single["bit_equal"]:
                    worst1 = max(rel_err(av, a1).max(), (np.abs(pv - p1) / np.abs(p1)).max())
                    bad.append(f"one rank: differs from the single-rank Domain.gravity(h) by {worst1:.2e}")
            figs[-1]["single_rank"] = single
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
