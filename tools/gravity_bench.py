"""Barnes-Hut gravity (csrc/gravity.hip) on the MI355X: one JSON line per configuration.

For every cloud x precision x size: Domain.sync_grav, then the multipole upsweep (cstone_hip_upsweep_multipoles) and the
group walk (cstone_hip_compute_gravity, order 2, theta 0.5) timed with device events after warm-up, the mean P2P / M2P
interactions per target (from the walk's own counters, in a separate call), interactions/s and FLOP/s.

FLOP per interaction, as the kernel writes them (-ffp-contract=off: no FMA; sqrt and the division count one each):
  P2P  21: d 3, r^2 + eps^2 6, sqrt 1, 1/r 1, m/r 1, m/r^3 2, a 6, phi 1
  M2P  54: d 3, r^2 + eps^2 6, sqrt 1, 1/r 1, 1/r^2 1, M/r^3 2, Q d 15, d.Q.d 5, 1/r^5 2, the d coefficient 4, a 9, phi 5

With --mr the same cloud also goes through the multi-rank route on a world of one rank (NativeDistributedDomain over
gloo: sync_grav, then cstone_hip_domain_mr_compute_gravity): mr_multipoles_ms is the multipole update of the locally
essential tree (with its exchanges, which a single rank skips) and mr_walk_ms the LET walk, both from the library's
stage timers, mr_call_ms the whole call between device events.  The single-rank figures of the same process stand
beside them in the same line.

With --h the walk is also timed with per-particle softening lengths (cstone_hip_compute_gravity_h, h = the smoothing
lengths of the cloud as the sync returned them): walk_h_ms beside walk_ms.  A softened pair costs 29 FLOP by the same
convention (H 1, H^2 1, 1/r^2 1, w 4, phi 1 more than the 21).

With --direct-sample K the all-pairs direct sum (cstone_hip_direct_gravity) of K sampled targets against the whole cloud
is timed (direct_ms, direct_pairs_per_s, direct_flop_per_s and its share of the vector FP peak of the precision, FMA
counted as two operations as in DESIGN section 7d -- this code issues none, so 0.5 is its ceiling), and the walk's
relative errors against it on those targets are printed (median / p99 of |da| and |dphi|, orders 0 and 2); with --h the
same for the softened walk against the softened direct sum.

With --orders 2 3 the octupole upsweep (cstone_hip_upsweep_octupoles, octupole_upsweep_ms) and the order-3 walk
(cstone_hip_compute_gravity_o3, walk_o3_ms) are timed as well, the two walks ALTERNATING repetition by repetition in the
same process (walk_ms is then the order-2 median of that alternation); with --direct-sample the errors of order 3 stand
beside those of orders 0 and 2.  Order 3 is also run at --o3-theta (0.7; a second domain on the same cloud): its walk
time, interactions per target and errors are the line's "o3_theta" entry, to set against the order-2 walk at --theta.
flop_per_s stays the order-2 walk's.  --run TAG puts "run": TAG in front of every line.  The default (--orders 2) prints what
it printed before the option existed.

    python tools/gravity_bench.py [--sizes 1e6 1e7] [--clouds plummer uniform] [--reals 64 32] [--reps 5] [--mr] [--h]
                                  [--direct-sample K] [--orders 2 3] [--o3-theta 0.7] [--run TAG]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "cornerstone-octree_amd"))

P2P_FLOP, M2P_FLOP = 21, 54
P2P_SOFT_FLOP = 29
PEAK_FLOPS = {64: 78.6e12, 32: 157.3e12}  # AMD's specification of the MI355X, vector units, an FMA counted as two


def order3_at(ctx, a, n, rb, lim, x, y, z, h, timed):
    """the order-3 walk of the same cloud on a domain of its own at theta = a.o3_theta: a dict of its time, its
    interactions per target and, with --direct-sample, its errors against the direct sum"""
    import numpy as np
    import torch

    import cstone_amd
    from cstone_amd.domain import Domain

    m = torch.full((n,), 1.0 / n, dtype=x.dtype, device="cuda")
    dom = Domain(ctx, cstone_amd.HILBERT, 64, rb, 4096, 64, a.o3_theta, cstone_amd.make_cbox(lim))
    keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    keys, x, y, z, h, m, _, _ = dom.sync_grav(keys, x, y, z, h, m, [torch.empty_like(x) for _ in range(3)])
    v = dom.view()
    L, M, ne = v.num_focus_leaves, v.num_focus_nodes, v.end_index

    def dev(ptr, count, np_dt):
        return torch.from_numpy(dom.fetch(ptr, count, np_dt)).cuda()

    child, itl = dev(v.child_offsets, M + 1, np.int32), dev(v.internal_to_leaf, M, np.int32)
    lti = dev(v.leaf_to_internal, M, np.int32)[M - L:].contiguous()
    layout, leaves = dev(v.layout, L + 1, np.int32), dev(v.focus_leaves, L + 1, np.int64)
    levels = dom.fetch(v.level_range, 23, np.int32)
    centers = dev(v.expansion_centers, 4 * M, np.float64 if rb == 64 else np.float32)
    groups = ctx.compute_group_splits(0, ne, x, y, z, leaves, layout, v.box, 64, cstone_amd.GRAVITY_GROUP_TOL)
    mp = ctx.upsweep_multipoles(x, y, z, m, lti, layout, levels, child, centers)
    oc = ctx.upsweep_octupoles(x, y, z, m, lti, layout, levels, child, centers, mp)
    args = (x, y, z, m, 0, ne, groups, v.box, child, itl, layout, centers, mp, oc)
    ms, ms_min = timed(lambda: ctx.compute_gravity_o3(*args, potential=True))
    *_, p2p, m2p = ctx.compute_gravity_o3(*args, potential=True, counts=True)
    out = dict(theta=a.o3_theta, leaves=L, walk_o3_ms=round(ms, 3), walk_o3_ms_min=round(ms_min, 3),
               p2p_per_target=round(p2p.double().mean().item(), 1), m2p_per_target=round(m2p.double().mean().item(), 1))
    if a.direct_sample:
        K = min(a.direct_sample, ne)
        tg = torch.randperm(ne, device="cuda", generator=torch.Generator("cuda").manual_seed(5))[:K].int()
        ref = ctx.direct_gravity(x, y, z, m, None, targets=tg)
        ra = torch.stack(ref[:3], 1)
        got = ctx.compute_gravity_o3(*args, potential=True)
        e = (torch.stack(got[:3], 1)[tg.long()] - ra).norm(dim=1) / ra.norm(dim=1)
        ep = (got[3][tg.long()] - ref[3]).abs() / ref[3].abs()
        out["walk_vs_direct"] = dict(order3=[float(f"{t.double().quantile(q).item():.3g}") for t in (e, ep)
                                             for q in (0.5, 0.99)])
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", nargs="+", type=float, default=[1e6, 1e7])
    p.add_argument("--clouds", nargs="+", default=["plummer", "uniform"])
    p.add_argument("--reals", nargs="+", type=int, default=[64, 32])
    p.add_argument("--theta", type=float, default=0.5)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--mr", action="store_true", help="also time the multi-rank route on a world of one rank")
    p.add_argument("--h", action="store_true", help="also time the walk with per-particle softening lengths")
    p.add_argument("--direct-sample", type=int, default=0, metavar="K",
                   help="time the direct sum of K sampled targets and print the walk's error against it")
    p.add_argument("--orders", nargs="+", type=int, default=[2], choices=[2, 3],
                   help="the orders of the walk to time: 2 (the default), or 2 3 for the octupoles as well")
    p.add_argument("--o3-theta", type=float, default=0.7, help="the second theta of the order-3 walk (0: none)")
    p.add_argument("--run", default=None, help="a tag put in front of every line")
    a = p.parse_args()
    o3 = 3 in a.orders

    import numpy as np
    import torch

    import cstone_amd
    from cstone_amd.clouds import make_cloud
    from cstone_amd.domain import Domain

    ctx = cstone_amd.Context(0)
    if a.mr:
        import torch.distributed as dist

        from cstone_amd.distributed import NativeDistributedDomain

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29830")
        dist.init_process_group("gloo", rank=0, world_size=1)
    for n in [int(s) for s in a.sizes]:
        for cloud in a.clouds:
            for rb in a.reals:
                dt = torch.float64 if rb == 64 else torch.float32
                x, y, z, h, lim = make_cloud(cloud, n, n, "cuda", dt, 7)
                m = torch.full((n,), 1.0 / n, dtype=dt, device="cuda")
                x0, y0, z0, h0 = (x.clone(), y.clone(), z.clone(), h.clone()) if o3 and a.o3_theta else (None,) * 4
                dom = Domain(ctx, cstone_amd.HILBERT, 64, rb, 4096, 64, a.theta, cstone_amd.make_cbox(lim))
                keys = torch.zeros(n, dtype=torch.int64, device="cuda")
                scratch = [torch.empty_like(x) for _ in range(3)]
                keys, x, y, z, h, m, scratch, _ = dom.sync_grav(keys, x, y, z, h, m, scratch)
                v = dom.view()
                L, M, ne = v.num_focus_leaves, v.num_focus_nodes, v.end_index

                def dev(ptr, count, np_dt):
                    return torch.from_numpy(dom.fetch(ptr, count, np_dt)).cuda()

                child = dev(v.child_offsets, M + 1, np.int32)
                itl = dev(v.internal_to_leaf, M, np.int32)
                lti = dev(v.leaf_to_internal, M, np.int32)[M - L:].contiguous()
                layout = dev(v.layout, L + 1, np.int32)
                leaves = dev(v.focus_leaves, L + 1, np.int64)
                levels = dom.fetch(v.level_range, 23, np.int32)
                centers = dev(v.expansion_centers, 4 * M, np.float64 if rb == 64 else np.float32)
                groups = ctx.compute_group_splits(0, ne, x, y, z, leaves, layout, v.box, 64,
                                                  cstone_amd.GRAVITY_GROUP_TOL)
                mp = ctx.upsweep_multipoles(x, y, z, m, lti, layout, levels, child, centers)

                def timed(fn):
                    for _ in range(a.warmup):
                        fn()
                    ts = []
                    for _ in range(a.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        ts.append(e0.elapsed_time(e1))
                    return float(np.median(ts)), float(min(ts))

                up_ms, up_min = timed(lambda: ctx.upsweep_multipoles(x, y, z, m, lti, layout, levels, child, centers,
                                                                     multipoles=mp))
                walk = lambda: ctx.compute_gravity(x, y, z, m, 0, ne, groups, v.box, child, itl, layout, centers, mp,
                                                   order=2, potential=True)  # noqa: E731
                third = {}
                if o3:
                    oc = ctx.upsweep_octupoles(x, y, z, m, lti, layout, levels, child, centers, mp)
                    ou_ms, ou_min = timed(lambda: ctx.upsweep_octupoles(x, y, z, m, lti, layout, levels, child, centers,
                                                                        mp, octupoles=oc))
                    walk3 = lambda: ctx.compute_gravity_o3(x, y, z, m, 0, ne, groups, v.box, child, itl, layout, centers,
                                                           mp, oc, potential=True)  # noqa: E731
                    for _ in range(a.warmup):
                        walk(), walk3()
                    ts = {2: [], 3: []}
                    for _ in range(a.reps):  # the two orders alternate
                        for order, fn in ((2, walk), (3, walk3)):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            fn()
                            e1.record()
                            e1.synchronize()
                            ts[order].append(e0.elapsed_time(e1))
                    walk_ms, walk_min = float(np.median(ts[2])), float(min(ts[2]))
                    third = dict(octupole_upsweep_ms=round(ou_ms, 4), walk_o3_ms=round(float(np.median(ts[3])), 3),
                                 walk_o3_ms_min=round(float(min(ts[3])), 3),
                                 walk_o3_over_walk=round(float(np.median(ts[3])) / walk_ms, 3))
                else:
                    walk_ms, walk_min = timed(walk)
                *_, p2p, m2p = ctx.compute_gravity(x, y, z, m, 0, ne, groups, v.box, child, itl, layout, centers, mp,
                                                   order=2, potential=True, counts=True)
                p2p_mean, m2p_mean = p2p.double().mean().item(), m2p.double().mean().item()
                inter = (p2p_mean + m2p_mean) * ne
                flop = (p2p_mean * P2P_FLOP + m2p_mean * M2P_FLOP) * ne
                soft = {}
                if a.h:
                    walk_h = lambda: ctx.compute_gravity(x, y, z, m, 0, ne, groups, v.box, child, itl, layout, centers,
                                                         mp, order=2, potential=True, h=h)  # noqa: E731
                    walk_h_ms, walk_h_min = timed(walk_h)
                    soft = dict(walk_h_ms=round(walk_h_ms, 3), walk_h_ms_min=round(walk_h_min, 3),
                                walk_h_over_walk=round(walk_h_ms / walk_ms, 3))
                if a.direct_sample:
                    K = min(a.direct_sample, ne)
                    tg = torch.randperm(ne, device="cuda", generator=torch.Generator("cuda").manual_seed(5))[:K].int()
                    pick = tg.long()

                    def errors(hh):
                        ref = ctx.direct_gravity(x, y, z, m, hh, targets=tg)
                        ra = torch.stack(ref[:3], 1)
                        out = {}
                        for order in (0, 2):
                            got = ctx.compute_gravity(x, y, z, m, 0, ne, groups, v.box, child, itl, layout, centers, mp,
                                                      order=order, potential=True, h=hh)
                            e = (torch.stack(got[:3], 1)[pick] - ra).norm(dim=1) / ra.norm(dim=1)
                            ep = (got[3][pick] - ref[3]).abs() / ref[3].abs()
                            out[f"order{order}"] = [float(f"{t.double().quantile(q).item():.3g}") for t in (e, ep)
                                                    for q in (0.5, 0.99)]
                        if o3:
                            got = ctx.compute_gravity_o3(x, y, z, m, 0, ne, groups, v.box, child, itl, layout, centers, mp,
                                                         oc, potential=True, h=hh)
                            e = (torch.stack(got[:3], 1)[pick] - ra).norm(dim=1) / ra.norm(dim=1)
                            ep = (got[3][pick] - ref[3]).abs() / ref[3].abs()
                            out["order3"] = [float(f"{t.double().quantile(q).item():.3g}") for t in (e, ep)
                                             for q in (0.5, 0.99)]
                        return out

                    for key, hh, per_pair in (("direct", None, P2P_FLOP),) + ((("direct_h", h, P2P_SOFT_FLOP),) if a.h else ()):
                        d_ms, d_min = timed(lambda: ctx.direct_gravity(x, y, z, m, hh, targets=tg))
                        pairs = float(K) * float(ne)
                        soft.update({f"{key}_targets": K, f"{key}_ms": round(d_ms, 3), f"{key}_ms_min": round(d_min, 3),
                                     f"{key}_pairs_per_s": float(f"{pairs / (d_ms * 1e-3):.4g}"),
                                     f"{key}_flop_per_s": float(f"{pairs * per_pair / (d_ms * 1e-3):.4g}"),
                                     f"{key}_share_of_fp_peak": round(pairs * per_pair / (d_ms * 1e-3) / PEAK_FLOPS[rb], 4),
                                     f"walk_vs_{key}": errors(hh)})
                if o3 and a.o3_theta:
                    third["o3_theta"] = order3_at(ctx, a, n, rb, lim, x0, y0, z0, h0, timed)
                    del x0, y0, z0, h0
                mr = {}
                if a.mr:
                    x0, y0, z0, h0, _ = make_cloud(cloud, n, n, "cuda", dt, 7)
                    m0 = torch.full((n,), 1.0 / n, dtype=dt, device="cuda")
                    mdom = NativeDistributedDomain(ctx, cstone_amd.HILBERT, 64, rb, 4096, 64, lim, theta=a.theta)
                    r = mdom.sync_grav(x0, y0, z0, h0, m0)
                    call = lambda: mdom.gravity(r["x"], r["y"], r["z"], r["m"], exchange_masses=False)  # noqa: E731
                    call_ms, _ = timed(call)
                    ctx.profile_enable(True)
                    ctx.profile_reset()
                    for _ in range(a.reps):
                        call()
                    ctx.sync()
                    (mp_ms, mp_cnt), (wk_ms, wk_cnt) = ctx.profile_get("multipoles"), ctx.profile_get("gravity")
                    ctx.profile_enable(False)
                    mr = dict(mr_leaves=int(mdom.view().num_focus_leaves), mr_call_ms=round(call_ms, 3),
                              mr_multipoles_ms=round(mp_ms / a.reps, 4), mr_walk_ms=round(wk_ms / max(wk_cnt, 1), 3))
                    del mdom, r, x0, y0, z0, h0, m0
                tag = dict(run=a.run) if a.run is not None else {}
                print(json.dumps(dict(
                    **tag, n=n, cloud=cloud, real_bits=rb, theta=a.theta, leaves=L, groups=int(groups.numel() - 1), **mr,
                    **soft, **third,
                    upsweep_ms=round(up_ms, 4), walk_ms=round(walk_ms, 3), walk_ms_min=round(walk_min, 3),
                    p2p_per_target=round(p2p_mean, 1), m2p_per_target=round(m2p_mean, 1),
                    interactions_per_s=float(f"{inter / (walk_ms * 1e-3):.4g}"),
                    flop_per_s=float(f"{flop / (walk_ms * 1e-3):.4g}"))), flush=True)
                del dom, x, y, z, h, m, keys, scratch, mp, groups
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
