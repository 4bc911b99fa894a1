"""One rank of tests/test_pair_counts_mr.py: NativeDistributedDomain.pair_counts and pair_counts_cross
(cstone_hip_domain_mr_pair_counts, cstone_hip_domain_mr_pair_counts_cross).  Started by `python -m torch.distributed.run`;
the ranks talk over gloo and share the one GPU.  After the sync the ranks gather their assigned coordinates in rank order:
that is the whole cloud.  Every rank compares what it received with the brute force over that cloud
(tests/pair_counts_support.py): counts with ==, sums within the bound derived there; rank 0 prints one line
`PAIR_MR_RESULT {json}` with the counts, which the launcher compares with the brute force over the cloud as generated --
the same for every number of ranks.

Every particle carries the same smoothing length H, so the kept halo radius of every leaf is float32(2 H) and the outer edge
is exactly that: the cover rule holds with equality.  One float32 ulp more and the call must be refused on every rank of a
communicator of several, and be taken on one rank.  A particle's weight is 0.5 + x: it follows from the synced arrays,
halos included, without an exchange.

A failed check is recorded and the rank goes on, so that no rank waits in a collective for one that has stopped.  After
every refused call the ranks gather their return codes: that every rank came back, and with what, is part of the result."""
import ctypes as C
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

import pair_counts_support as ps  # noqa: E402

E_ARG, E_INTERNAL = -1, -4
N, Q, NB, PAD = 6000, 500, 8, 3
H = 0.03
CLOUDS = ("uniform-pbc-f64", "blobs-open-f32")


def make_cloud(name):
    """(coordinates, boundary conditions): N particles in the unit box, uniform or in five Gaussian blobs"""
    kind, bc, rb = name.split("-")
    T = np.float32 if rb == "f32" else np.float64
    bcs = (1, 1, 1) if bc == "pbc" else (0, 0, 0)
    rng = np.random.default_rng(302)
    if kind == "uniform":
        pts = rng.uniform(0, 1, (N, 3))
    else:
        centers = rng.uniform(0.2, 0.8, (5, 3))
        pts = np.clip(centers[rng.integers(0, 5, N)] + rng.normal(0, 0.03, (N, 3)), 0.0, np.nextafter(1.0, 0.0))
    return [np.ascontiguousarray(pts[:, a]).astype(T) for a in range(3)], bcs


def outer_edge(T):
    """the kept halo radius of every leaf: float32(T(H) * 2), as the sync computes it with the halo factor 1"""
    return float(np.float32(T(H) * T(2)))


def make_edges(T):
    R = outer_edge(T)
    return [R * (k / NB) ** (1.0 / 3.0) for k in range(NB)] + [R]


def make_queries(T):
    """Q centres, the same on every rank: in the box, a few outside it"""
    rng = np.random.default_rng(303)
    qc = rng.uniform(0, 1, (Q, 3))
    qc[-20:] += rng.choice([-1.0, 1.0], (20, 3)) * rng.uniform(0.0, 0.05, (20, 3))
    return qc.astype(T), rng.uniform(0.5, 1.5, Q)


def weights_of(x):
    return 0.5 + np.asarray(x).astype(np.float64)


class Run:
    def __init__(self, hip, rank, P):
        self.hip, self.rank, self.P, self.bad = hip, rank, P, []
        self.culprit = P - 1

    def fail(self, what, text):
        self.bad.append(f"rank {self.rank}, {what}: {text}")

    def raw(self, dom, r, w, edges, cross=None, null=(), with_w=True):
        """the C entry on sentinel-filled outputs with PAD more entries: (return code, outputs as numpy arrays, stats)"""
        import cstone_amd

        e, nb = cstone_amd.sphere_edges(edges)
        out = dict(counts=torch.full((max(nb, 1) + PAD,), ps.SENT_COUNT, dtype=torch.int64, device="cuda"),
                   sums=torch.full((max(nb, 1) + PAD,), ps.SENT_SUM, dtype=torch.float64, device="cuda"))
        a = {name: (r[name].data_ptr() if r is not None and r[name].numel() else None) for name in ("x", "y", "z")}
        for name in null:
            a[name] = None
        wp = w.data_ptr() if (w is not None and with_w) else None
        st = (C.c_uint64 * 2)(7, 7)
        torch.cuda.synchronize()
        if cross is None:
            rc = self.hip.lib.cstone_hip_domain_mr_pair_counts(dom.h, a["x"], a["y"], a["z"], wp, 64, e, nb, out["counts"].data_ptr(),
                                                               out["sums"].data_ptr(), st)
        else:
            qc, qw = cross
            rc = self.hip.lib.cstone_hip_domain_mr_pair_counts_cross(dom.h, a["x"], a["y"], a["z"], wp, 64, qc.data_ptr(),
                                                                     qw.data_ptr() if (qw is not None and wp) else None,
                                                                     qc.shape[0], e, nb, out["counts"].data_ptr(),
                                                                     out["sums"].data_ptr(), st)
        dom.coll.error = None
        self.hip.sync()
        return rc, {name: t.cpu().numpy() for name, t in out.items()}, (int(st[0]), int(st[1]))

    @staticmethod
    def clean(got, start=0):
        return (got["counts"][start:] == ps.SENT_COUNT).all() and (got["sums"][start:] == ps.SENT_SUM).all()

    def refused(self, what, rc, got, mine, others):
        """every rank came back: the return codes of all ranks are gathered and checked on every rank"""
        codes = [None] * self.P
        dist.all_gather_object(codes, rc)
        want = [mine if p == self.culprit else others for p in range(self.P)]
        if codes != want or not self.clean(got):
            self.fail(what, f"return codes {codes}, expected {want}, or something was written")
        return codes

    def compare(self, what, rc, got, ref):
        if rc != 0:
            self.fail(what, f"returned {rc}")
            return
        if not self.clean(got, start=NB):
            self.fail(what, "something behind the bins was written")
        if not (ref.counts[0] > 0 and ref.counts[-1] > 0):
            self.fail(what, "the reference's first or last bin is empty")
        if not np.array_equal(got["counts"][:NB].view(np.uint64), ref.counts):
            self.fail(what, f"counts {got['counts'][:NB].tolist()} differ from the brute force over the whole cloud "
                            f"{ref.counts.tolist()}")
        if not (np.abs(got["sums"][:NB] - ref.sums) <= ref.sum_bound()).all():
            self.fail(what, "sums beyond the bound")
        everyone = [None] * self.P
        dist.all_gather_object(everyone, {key: got[key].tobytes() for key in got})
        if any(e != everyone[0] for e in everyone):
            self.fail(what, "the ranks do not hold the same bits")

    def cloud(self, name):
        import cstone_amd
        from cstone_amd.distributed import NativeDistributedDomain

        coords, bc = make_cloud(name)
        T = coords[0].dtype.type
        tdt = torch.float32 if T is np.float32 else torch.float64
        edges = make_edges(T)
        qc_h, qw_h = make_queries(T)
        qc, qw = torch.from_numpy(qc_h).cuda(), torch.from_numpy(qw_h).cuda()
        statuses = {}

        dom = NativeDistributedDomain(self.hip, cstone_amd.HILBERT, 64, coords[0].itemsize * 8, 64, 16, [0.0, 1.0] * 3, bc)
        rc, got, _ = self.raw(dom, None, None, edges)
        statuses["no sync"] = self.refused(f"{name}, before the first sync", rc, got, E_ARG, E_ARG)
        rc, got, _ = self.raw(dom, None, None, edges, cross=(qc, qw))
        statuses["no sync, cross"] = self.refused(f"{name}, cross counts before the first sync", rc, got, E_ARG, E_ARG)

        mine = np.nonzero(np.random.default_rng(78).integers(0, self.P, N) == self.rank)[0]
        dev = [torch.from_numpy(c[mine].copy()).cuda() for c in coords]
        h = torch.full((mine.size,), H, dtype=tdt, device="cuda")
        r = dom.sync(*dev, h)
        self.hip.sync()
        start, end = int(r["start"]), int(r["end"])
        w = (0.5 + r["x"].double()).contiguous()

        # the whole cloud: the assigned ranges in rank order
        parts = [None] * self.P
        dist.all_gather_object(parts, [r[a][start:end].cpu().numpy() for a in "xyz"])
        whole = [np.concatenate([p[a] for p in parts]) for a in range(3)]
        assigned = [int(p[0].size) for p in parts]
        if whole[0].size != N:
            self.fail(name, f"the assigned ranges hold {whole[0].size} particles of {N}")
        lim = list(r["lim"])
        w_whole = weights_of(whole[0])

        ref = ps.auto_reference(whole, w_whole, 0, N, 0, N, lim, bc, edges)
        rc, got, stats = self.raw(dom, r, w, edges)
        self.compare(f"{name}, auto counts", rc, got, ref)
        all_stats = [None] * self.P
        dist.all_gather_object(all_stats, stats)
        if sum(s[1] for s in all_stats) != int(ref.counts.sum()):
            self.fail(name, f"the ranks binned {[s[1] for s in all_stats]} pairs, the brute force {int(ref.counts.sum())}")
        ref_x = ps.cross_reference(whole, w_whole, 0, N, qc_h, qw_h, lim, bc, edges)
        rc, got_x, _ = self.raw(dom, r, w, edges, cross=(qc, qw))
        self.compare(f"{name}, cross counts", rc, got_x, ref_x)
        # without weights: the same counts, sums untouched
        rc, bare, _ = self.raw(dom, r, None, edges)
        if rc != 0 or bare["counts"].tobytes() != got["counts"].tobytes() or (bare["sums"] != ps.SENT_SUM).any():
            self.fail(name, "the call without weights differs in its counts or wrote sums")

        # the bindings
        have = end > start
        args = [r[a] if have else None for a in "xyz"]
        c3, s3, _ = dom.pair_counts(*args, w if have else None, edges)
        c4, s4, _ = dom.pair_counts_cross(*args, w if have else None, qc, edges, query_w=qw)
        self.hip.sync()
        if c3.cpu().numpy().tobytes() != got["counts"][:NB].tobytes() or s3.cpu().numpy().tobytes() != got["sums"][:NB].tobytes():
            self.fail(name, "NativeDistributedDomain.pair_counts differs from the C entry")
        if c4.cpu().numpy().tobytes() != got_x["counts"][:NB].tobytes() or s4.cpu().numpy().tobytes() != got_x["sums"][:NB].tobytes():
            self.fail(name, "NativeDistributedDomain.pair_counts_cross differs from the C entry")

        # refusals: the same on every rank
        for label, bad in (("bad edges", [0.0, 0.01, 0.01]), ("no bins", [0.01])):
            rc, g, _ = self.raw(dom, r, w, bad)
            statuses[label] = self.refused(f"{name}, {label}", rc, g, E_ARG, E_ARG)
            rc, g, _ = self.raw(dom, r, w, bad, cross=(qc, qw))
            statuses[label + ", cross"] = self.refused(f"{name}, {label}, cross", rc, g, E_ARG, E_ARG)
        last = self.rank == self.culprit
        if self.P > 1:
            fewer = make_edges(T)[1:]
            rc, g, _ = self.raw(dom, r, w, fewer if last else edges)
            statuses["NB differs"] = self.refused(f"{name}, another NB on the last rank", rc, g, E_ARG, E_ARG)
            rc, g, _ = self.raw(dom, r, w, fewer if last else edges, cross=(qc, qw))
            statuses["NB differs, cross"] = self.refused(f"{name}, another NB on the last rank, cross", rc, g, E_ARG, E_ARG)
            rc, g, _ = self.raw(dom, r, w, edges, with_w=not last)
            statuses["w differs"] = self.refused(f"{name}, no w on the last rank", rc, g, E_ARG, E_ARG)
            rc, g, _ = self.raw(dom, r, w, edges, cross=(qc, qw), with_w=not last)
            statuses["w differs, cross"] = self.refused(f"{name}, no w on the last rank, cross", rc, g, E_ARG, E_ARG)
        rc, g, _ = self.raw(dom, r, w, edges, null=("x",) if last else ())
        statuses["null x"] = self.refused(f"{name}, a null x on the last rank", rc, g, E_ARG, E_INTERNAL)
        rc, g, _ = self.raw(dom, r, w, edges, cross=(qc, qw), null=("x",) if last else ())
        statuses["null x, cross"] = self.refused(f"{name}, a null x on the last rank, cross", rc, g, E_ARG, E_INTERNAL)
        # the cover rule: one float32 ulp above the kept halo radius
        beyond = edges[:-1] + [float(np.nextafter(np.float32(edges[-1]), np.float32(np.inf)))]
        rc, g, _ = self.raw(dom, r, w, beyond)
        if self.P > 1:
            statuses["cover"] = self.refused(f"{name}, the outer edge an ulp above the halo radius", rc, g, E_ARG, E_ARG)
        else:
            statuses["cover"] = [rc]
            self.compare(f"{name}, one rank takes an outer edge above the halo radius", rc, g,
                         ps.auto_reference(whole, w_whole, 0, N, 0, N, lim, bc, beyond))
        # the cross counts need no reach: the same edge is taken on any number of ranks
        rc, g, _ = self.raw(dom, r, w, beyond, cross=(qc, qw))
        self.compare(f"{name}, cross counts with an outer edge above the halo radius", rc, g,
                     ps.cross_reference(whole, w_whole, 0, N, qc_h, qw_h, lim, bc, beyond))
        # and the domain is still usable
        rc, again, _ = self.raw(dom, r, w, edges)
        if rc != 0 or again["counts"].tobytes() != got["counts"].tobytes():
            self.fail(name, "the call after the refusals differs from the one before")
        dom.close()
        return dict(statuses=statuses, assigned=assigned, auto=got["counts"][:NB].tolist(), cross=got_x["counts"][:NB].tolist(),
                    halos=int(r["x"].numel() - (end - start)))


def main():
    dist.init_process_group("gloo")
    rank, P = dist.get_rank(), dist.get_world_size()
    import cstone_amd

    torch.cuda.set_device(0)
    run = Run(cstone_amd.Context(0), rank, P)
    names = sys.argv[1:] or list(CLOUDS)
    figs = {}
    try:
        for name in names:
            figs[name] = run.cloud(name)
    except Exception as e:  # (the other ranks may now wait in a collective: the launcher's timeout ends them)
        import traceback

        traceback.print_exc()
        print("PAIR_MR_RESULT " + json.dumps(dict(ok=False, ranks=P, bad=run.bad + [f"rank {rank}: {type(e).__name__}: {e}"])),
              flush=True)
        os._exit(1)
    allbad = [None] * P
    dist.all_gather_object(allbad, run.bad)
    flat = [b for part in allbad for b in part]
    if rank == 0:
        print("PAIR_MR_RESULT " + json.dumps(dict(ok=not flat, ranks=P, bad=flat[:20], clouds=figs), default=float), flush=True)
    dist.destroy_process_group()
    sys.exit(0 if not flat else 1)


if __name__ == "__main__":
    main()
