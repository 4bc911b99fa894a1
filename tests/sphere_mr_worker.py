"""One rank of tests/test_sphere_profiles_mr.py: NativeDistributedDomain.sphere_profiles
(cstone_hip_domain_mr_sphere_profiles) on the clouds of tests/fof_mr_support.py.  Started by `python -m
torch.distributed.run`; the ranks talk over gloo and share the one GPU.  Every particle carries its index in the generated
cloud and a weight that is a function of that index through the sync.  Every rank compares what it received with the brute
force over the WHOLE cloud (tests/sphere_support.py); rank 0 prints one line `SPHERE_MR_RESULT {json}`.

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

import fof_mr_support as ms  # noqa: E402
import sphere_support as ss  # noqa: E402

E_ARG, E_INTERNAL = -1, -4
Q, PAD = 64, 3


def seeded_weights(index, mass_bits):
    """a weight in [1/6, 1/2) that depends on the particle's index in the generated cloud alone (thirds: sums of them round)"""
    w = (0.5 + ((index.astype(np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 20)).astype(np.float64) / float(1 << 20)) / 3.0
    return w.astype(np.float32 if mass_bits == 32 else np.float64)


class Run:
    def __init__(self, hip, rank, P):
        self.hip, self.rank, self.P, self.bad = hip, rank, P, []

    def fail(self, what, text):
        self.bad.append(f"rank {self.rank}, {what}: {text}")

    def raw(self, dom, r, qc, qs, edges, num_queries=None, null=(), with_w=True):
        """the C entry on sentinel-filled outputs with PAD more rows: (return code, outputs as numpy arrays)"""
        import cstone_amd

        nq = qc.shape[0] if num_queries is None else num_queries
        nb = len(edges) - 1
        out = dict(counts=torch.full((Q + PAD, max(nb, 1)), ss.SENT_COUNT, dtype=torch.int64, device="cuda"),
                   sums=torch.full((Q + PAD, max(nb, 1)), ss.SENT_SUM, dtype=torch.float64, device="cuda"),
                   flags=torch.full((Q + PAD,), ss.SENT_FLAG, dtype=torch.int32, device="cuda"))
        n = r["x"].numel() if r is not None else 0
        ptr = (lambda t: t.data_ptr() if (n and t is not None) else None)
        a = dict(x=ptr(r["x"]), y=ptr(r["y"]), z=ptr(r["z"]), w=ptr(r["w"]) if with_w else None) if r is not None else dict(
            x=None, y=None, z=None, w=None)
        for k in null:
            a[k] = None
        e, _ = cstone_amd.sphere_edges(edges)
        torch.cuda.synchronize()
        rc = self.hip.lib.cstone_hip_domain_mr_sphere_profiles(
            dom.h, a["x"], a["y"], a["z"], a["w"], (r["w"].element_size() * 8) if r is not None else 64, qc.data_ptr(),
            qs.data_ptr(), nq, e, nb, out["counts"].data_ptr(), out["sums"].data_ptr(), out["flags"].data_ptr())
        dom.coll.error = None
        self.hip.sync()
        return rc, {k: t.cpu().numpy() for k, t in out.items()}

    @staticmethod
    def clean(got, first_row=0):
        return ((got["counts"][first_row:] == ss.SENT_COUNT).all() and (got["sums"][first_row:] == ss.SENT_SUM).all() and
                (got["flags"][first_row:] == ss.SENT_FLAG).all())

    def refused(self, what, rc, got, mine, others):
        """every rank came back: the return codes of all ranks are gathered and checked on every rank"""
        codes = [None] * self.P
        dist.all_gather_object(codes, rc)
        want = [mine if p == self.culprit else others for p in range(self.P)]
        if codes != want or not self.clean(got):
            self.fail(what, f"return codes {codes}, expected {want}, or something was written")
        return codes

    def cloud(self, name, mass_bits):
        import cstone_amd
        from cstone_amd.distributed import NativeDistributedDomain

        coords, _, bc = ms.cloud(name)
        T = coords[0].dtype.type
        n = coords[0].size
        tdt = torch.float32 if T is np.float32 else torch.float64
        rng = np.random.default_rng(211)
        qc_h = rng.uniform(0, 1, (Q, 3)).astype(T)
        qc_h[:8] = np.stack([c[:8] for c in coords], axis=1)  # eight of them at particles
        qs_h = (0.45 * 10.0 ** rng.uniform(-1.5, 0, Q)).astype(T)
        if any(bc):
            qs_h[-1] = T(0.5)  # TOO_WIDE in a periodic box
        edges = ss.linear_edges(8, 1.0)
        qc, qs = torch.from_numpy(qc_h).cuda(), torch.from_numpy(qs_h).cuda()
        self.culprit = self.P - 1
        statuses = {}

        dom = NativeDistributedDomain(self.hip, cstone_amd.HILBERT, 64, coords[0].itemsize * 8, 64, 16, [0.0, 1.0] * 3, bc)
        rc, got = self.raw(dom, None, qc, qs, edges)
        statuses["no sync"] = self.refused(f"{name}, before the first sync", rc, got, E_ARG, E_ARG)

        mine = np.nonzero(np.random.default_rng(78).integers(0, self.P, n) == self.rank)[0]
        dev = [torch.from_numpy(c[mine].copy()).cuda() for c in coords]
        h = torch.full((mine.size,), 0.02, dtype=tdt, device="cuda")
        props = [torch.from_numpy(mine.astype(np.int64)).cuda(), torch.from_numpy(seeded_weights(mine, mass_bits)).cuda()]
        r = dom.sync(*dev, h, props=props)
        r["w"] = r["props"][1].clone()

        for label, bad in (("descending", [0.0, 0.6, 0.5]), ("negative", [-0.1, 1.0]), ("nan", [0.0, float("nan")]),
                           ("too many", ss.linear_edges(65, 1.0))):
            rc, got = self.raw(dom, r, qc, qs, bad)
            statuses[f"edges {label}"] = self.refused(f"{name}, edges {label}", rc, got, E_ARG, E_ARG)
        if self.P > 1:
            rc, got = self.raw(dom, r, qc, qs, edges, num_queries=Q - 1 if self.rank == self.culprit else Q)
            statuses["Q differs"] = self.refused(f"{name}, another Q on the last rank", rc, got, E_ARG, E_ARG)
        rc, got = self.raw(dom, r, qc, qs, edges, null=("x",) if self.rank == self.culprit else ())
        statuses["null x"] = self.refused(f"{name}, a null x on the last rank", rc, got, E_ARG, E_INTERNAL)

        # the correct call afterwards
        rc, got = self.raw(dom, r, qc, qs, edges)
        rc2, again = self.raw(dom, r, qc, qs, edges)
        if rc != 0 or rc2 != 0:
            self.fail(name, f"returned {rc}, {rc2}")
            dom.close()
            return dict(statuses=statuses)
        if not self.clean(got, first_row=Q):
            self.fail(name, "rows behind the last query were written")
        lim = list(r["lim"])
        ref = ss.Profiles(list(coords), seeded_weights(np.arange(n), mass_bits), 0, n, lim, bc, qc_h, qs_h, edges)
        counts, sums, flags = got["counts"][:Q].view(np.uint64), got["sums"][:Q], got["flags"][:Q].view(np.uint32)
        if not np.array_equal(counts, ref.counts):
            self.fail(name, f"counts differ from the brute force over the whole cloud in {int((counts != ref.counts).sum())} bins")
        if not np.array_equal(flags, ref.flags):
            self.fail(name, "flags differ")
        err, bound = np.abs(sums - ref.sums), ref.sum_bound()
        if not (err <= bound).all():
            k = np.unravel_index(np.argmax(err - bound), err.shape)
            self.fail(name, f"a sum is off by {err[k]:.3e}, bound {bound[k]:.3e}, count {int(ref.counts[k])}")
        if any(got[k].tobytes() != again[k].tobytes() for k in got):
            self.fail(name, "two calls do not give identical results")
        everyone = [None] * self.P
        dist.all_gather_object(everyone, {k: got[k].tobytes() for k in got})
        if any(e != everyone[0] for e in everyone):
            self.fail(name, "the ranks do not hold the same bits")
        c3, s3, f3 = dom.sphere_profiles(r["x"], r["y"], r["z"], r["w"], qc, edges, query_scale=qs)
        self.hip.sync()
        if (c3.cpu().numpy().tobytes() != got["counts"][:Q].tobytes() or s3.cpu().numpy().tobytes() != got["sums"][:Q].tobytes()
                or f3.cpu().numpy().tobytes() != got["flags"][:Q].tobytes()):
            self.fail(name, "NativeDistributedDomain.sphere_profiles differs from the C entry")
        # without weights: counts as before, sums untouched
        rc4, now = self.raw(dom, r, qc, qs, edges, with_w=False)
        if rc4 != 0 or now["counts"].tobytes() != got["counts"].tobytes() or (now["sums"] != ss.SENT_SUM).any():
            self.fail(name, "the call without weights differs in its counts or wrote sums")
        if self.P == 1:
            o = dom.octree()
            c5, s5, f5 = self.hip.sphere_profiles(r["x"], r["y"], r["z"], r["w"], r["start"], r["end"], dom.view().box, o,
                                                  o["layout"], o["centers"], o["sizes"], qc, edges, query_scale=qs)
            self.hip.sync()
            if (c5.cpu().numpy().tobytes() != got["counts"][:Q].tobytes() or s5.cpu().numpy().tobytes() != got["sums"][:Q].tobytes()
                    or f5.cpu().numpy().tobytes() != got["flags"][:Q].tobytes()):
                self.fail(name, "one rank: the bits differ from cstone_hip_sphere_profiles on the same arrays")
        dom.close()
        return dict(statuses=statuses, binned=int(ref.counts.sum()), wide=int((ref.flags != 0).sum()),
                    worst_sum_error=float(err.max()), assigned=int(r["end"] - r["start"]))


def main():
    dist.init_process_group("gloo")
    rank, P = dist.get_rank(), dist.get_world_size()
    import cstone_amd

    torch.cuda.set_device(0)
    run = Run(cstone_amd.Context(0), rank, P)
    figs = {}
    try:
        for k, name in enumerate(ms.CLOUDS):
            figs[name] = run.cloud(name, 32 if k % 2 else 64)
    except Exception as e:  # (the other ranks may now wait in a collective: the launcher's timeout ends them)
        import traceback

        traceback.print_exc()
        print("SPHERE_MR_RESULT " + json.dumps(dict(ok=False, ranks=P, bad=run.bad + [f"rank {rank}: {type(e).__name__}: {e}"])),
              flush=True)
        os._exit(1)
    allbad = [None] * P
    dist.all_gather_object(allbad, run.bad)
    flat = [b for part in allbad for b in part]
    if rank == 0:
        print("SPHERE_MR_RESULT " + json.dumps(dict(ok=not flat, ranks=P, bad=flat[:20], clouds=figs), default=float), flush=True)
    dist.destroy_process_group()
    sys.exit(0 if not flat else 1)


if __name__ == "__main__":
    main()
