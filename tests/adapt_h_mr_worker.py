"""One rank of tests/test_adapt_h.py::test_hip_adapt_h_on_several_ranks: NativeDistributedDomain.adapt_h
(cstone_hip_domain_mr_adapt_h) with a halo factor of 1.5, checked per particle against the restatement of the rule on the
WHOLE cloud with grow_limit = 1.5 (tests/adapt_h_support.py).  Started by `python -m torch.distributed.run`; the ranks
talk over gloo and share the one GPU.  A global id travels with every particle as a property.  Rank 0 prints one line
`ADAPT_RESULT {json}`.

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

import adapt_h_support as ah  # noqa: E402
import neighbors_support as ns  # noqa: E402
from helpers import Box  # noqa: E402

N, NG0, TOL, MAX_ITER, HALO_FACTOR = 6000, 30, 3, 10, 1.5


def cloud(pbc):
    """6 000 uniform particles in the unit box, h0 = the h of NG0 neighbours at the mean density times U(0.6, 1.4)"""
    rng = np.random.default_rng(77)
    x, y, z = rng.uniform(0, 1, (3, N))
    h_mean = 0.5 * (3 * NG0 / (4 * np.pi * N)) ** (1 / 3)
    h = h_mean * rng.uniform(0.6, 1.4, N)
    return x, y, z, h, ((1, 1, 1) if pbc else (0, 0, 0))


def run(pbc, hip, rank, P):
    import cstone_amd
    from cstone_amd.distributed import NativeDistributedDomain

    bad, what = [], f"rank {rank}"
    x, y, z, h, bc = cloud(pbc)
    mine = np.nonzero(np.random.default_rng(78).integers(0, P, N) == rank)[0]
    xs, ys, zs, hs = [torch.from_numpy(c[mine].copy()).cuda() for c in (x, y, z, h)]
    gid = torch.from_numpy(mine.astype(np.int64)).cuda()
    dom = NativeDistributedDomain(hip, cstone_amd.HILBERT, 64, 64, 64, 16, [0.0, 1.0] * 3, bc)
    dom.set_halo_factor(HALO_FACTOR)

    def refused(call, why):
        try:
            call()
        except cstone_amd.CstoneError:
            return
        bad.append(f"{what}: {why} was not refused")

    def synced():
        r = dom.sync(xs, ys, zs, hs, props=[gid])
        g = r["props"][0].clone()
        dom.exchange_halos(g)  # the halo ranges of a property are filled on request
        return r, g

    # ---- first sync: refusals, exchange=False
    r, g = synced()
    st, en = r["start"], r["end"]
    hh = r["h"]
    before = hh.clone()
    args = (r["x"], r["y"], r["z"], hh, NG0, TOL, MAX_ITER)
    refused(lambda: dom.adapt_h(*args, grow_limit=2.0), "a grow_limit above the halo factor")
    refused(lambda: dom.adapt_h(*args, grow_limit=0.5), "a grow_limit below 1")
    if not torch.equal(hh, before):
        bad.append(f"{what}: a refused call changed h")
    cnt, status = dom.adapt_h(*args, exchange=False)  # grow_limit 0: the halo factor
    hip.sync()
    keep = torch.ones_like(hh, dtype=torch.bool)
    keep[st:en] = False
    if not torch.equal(hh[keep], before[keep]):
        bad.append(f"{what}: exchange=False touched the halo ranges of h")
    refused(lambda: dom.adapt_h(*args, exchange=False), "a second call before the next sync")
    first = [t.cpu().numpy() for t in (g[st:en], hh[st:en], cnt, status)]

    # ---- second sync of the same input: the flag is cleared, exchange=True fills the halo ranges
    r, g = synced()
    st, en = r["start"], r["end"]
    hh = r["h"]
    cnt, status = dom.adapt_h(r["x"], r["y"], r["z"], hh, NG0, TOL, MAX_ITER, grow_limit=HALO_FACTOR, exchange=True)
    hip.sync()
    second = [t.cpu().numpy() for t in (g[st:en], hh[st:en], cnt, status)]
    # (the assignment may shift from one sync to the next: the two calls are compared per global id)
    both = [None] * P
    dist.all_gather_object(both, (first, second))
    for k, name in ((1, "h"), (2, "counts"), (3, "status")):
        a, b = np.empty(N, dtype=first[k].dtype), np.empty(N, dtype=first[k].dtype)
        a[np.concatenate([f[0] for f, _ in both])] = np.concatenate([f[k] for f, _ in both])
        b[np.concatenate([s[0] for _, s in both])] = np.concatenate([s[k] for _, s in both])
        if rank == 0 and not np.array_equal(a, b):
            bad.append(f"{name} after the second sync of the same input differs from the first call")
    parts = [None] * P
    dist.all_gather_object(parts, second + [np.stack([t[st:en].cpu().numpy() for t in (r["x"], r["y"], r["z"])])])
    ids = np.concatenate([p[0] for p in parts])
    h_new = np.empty(N)
    h_new[ids] = np.concatenate([p[1] for p in parts])
    halo_ids = g[keep].cpu().numpy()
    if not np.array_equal(hh[keep].cpu().numpy(), h_new[halo_ids]):
        bad.append(f"{what}: exchange=True left halo values of h that are not the owners' new ones")
    if np.array_equal(hh[keep].cpu().numpy(), h[halo_ids]):
        bad.append(f"{what}: no halo value of h changed")
    figs = dict(halos=int(keep.sum()))

    # ---- rank 0: the restatement on the whole cloud in the domain's box
    if rank == 0:
        if not np.array_equal(np.sort(ids), np.arange(N)):
            bad.append("the ranks do not hold every particle once")
        cnt_all, st_all = np.empty(N, dtype=np.int64), np.empty(N, dtype=np.int64)
        cnt_all[ids] = np.concatenate([p[2] for p in parts]).view(np.uint32)
        st_all[ids] = np.concatenate([p[3] for p in parts]).view(np.uint32)
        pos = np.empty((3, N))
        pos[:, ids] = np.concatenate([p[4] for p in parts], 1)
        if not np.array_equal(pos, np.stack([x, y, z])):
            bad.append("the global ids do not lead back to the coordinates")
        oracle = ah.the_oracle()
        box = Box(list(r["lim"]), bc)
        order = ah.sfc_order(oracle, x, y, z, box)
        case = ns.Case(oracle, x, y, z, h, box, 16)
        ref = ah.adapt(case, 0, N, ah.Params(NG0, TOL, MAX_ITER, HALO_FACTOR))
        for name, got, want in (("h", h_new[order], ref.h), ("counts", cnt_all[order], ref.counts),
                                ("status", st_all[order], ref.status)):
            wrong = np.flatnonzero(got != want)
            if wrong.size:
                bad.append(f"{name} differs from the restatement for {wrong.size} particles, first {wrong[:5].tolist()}: "
                           f"{got[wrong[:5]].tolist()} / {want[wrong[:5]].tolist()}")
        figs.update(particles=N, capped=int((ref.status & ah.CAPPED != 0).sum()),
                    converged=int((ref.status & ah.FLAGS == 0).sum()), max_walks=int((ref.status & ah.WALKS).max()))
    return bad, figs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pbc", action="store_true")
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, P = dist.get_rank(), dist.get_world_size()
    import cstone_amd

    torch.cuda.set_device(0)
    hip = cstone_amd.Context(0)
    try:
        bad, figs = run(a.pbc, hip, rank, P)
    except Exception as e:  # (the other ranks may now wait in a collective: the launcher's timeout ends them)
        import traceback

        traceback.print_exc()
        print("ADAPT_RESULT " + json.dumps(dict(ok=False, ranks=P, bad=[f"rank {rank}: {type(e).__name__}: {e}"])),
              flush=True)
        os._exit(1)
    allbad, allfigs = [None] * P, [None] * P
    dist.all_gather_object(allbad, bad)
    dist.all_gather_object(allfigs, figs)
    flat = [b for part in allbad for b in part]
    if rank == 0:
        res = dict(allfigs[0], ok=not flat, ranks=P, bad=flat[:20], halos=[f["halos"] for f in allfigs])
        print("ADAPT_RESULT " + json.dumps(res, default=float), flush=True)
    dist.destroy_process_group()
    sys.exit(0 if not flat else 1)


if __name__ == "__main__":
    main()
