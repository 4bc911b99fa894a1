"""One rank of tests/test_knn_mr.py: NativeDistributedDomain.knn (cstone_hip_domain_mr_knn).  Started by `python -m
torch.distributed.run`; the ranks talk over gloo and share the one GPU.  After the sync the ranks gather their assigned
coordinates in rank order: that is the whole cloud in global SFC order, and a global id is a position in it.  Every rank
compares what it received with the brute force over that cloud (tests/knn_support.py) with ==; rank 0 prints one line
`KNN_MR_RESULT {json}`.

A failed check is recorded and the rank goes on, so that no rank waits in a collective for one that has stopped.  After
every refused call the ranks gather their return codes: that every rank came back, and with what, is part of the result."""
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
import knn_support as ks  # noqa: E402

E_ARG, E_INTERNAL = -1, -4
Q, PAD = 40, 3
KS = (8, 100)
SENT_ID = 0x5A5A5A5A5A5A5A5A
CAP_ENV = "CSTONE_KNN_MR_GATHER_BYTES"
SMALL_CAP = 16384  # a few KiB: 3 queries per all_gather with k = 100 on 3 ranks, 40 with k = 8 on 3 ranks


def blobs_cloud(T):
    """6 000 particles in five Gaussian blobs of the unit box, clipped to it"""
    rng = np.random.default_rng(102)
    centers = rng.uniform(0.2, 0.8, (5, 3))
    pts = centers[rng.integers(0, 5, 6000)] + rng.normal(0, 0.03, (6000, 3))
    pts = np.clip(pts, 0.0, np.nextafter(1.0, 0.0))
    return [np.ascontiguousarray(pts[:, a]).astype(T) for a in range(3)]


def make_cloud(name):
    """(coordinates, boundary conditions)"""
    kind, bc, rb = name.split("-")
    T = np.float32 if rb == "f32" else np.float64
    bcs = (1, 1, 1) if bc == "pbc" else (0, 0, 0)
    if kind == "uniform":
        return ms.uniform_cloud(T)[0], bcs
    if kind == "blobs":
        return blobs_cloud(T), bcs
    assert kind == "sparse"  # 150 particles: k = 100 exceeds a rank's share, k = 256 the cloud
    n = 150
    return [a.astype(T) for a in np.random.default_rng(103).uniform(0, 1, (3, n))], bcs


CLOUDS = ("uniform-open-f64", "uniform-pbc-f32", "blobs-open-f32", "blobs-pbc-f64", "sparse-pbc-f64")


def make_queries(coords, bc, T):
    """Q centres: 30 in the box, 5 at particles, 5 far away (up to two box lengths on periodic axes, far more on open ones)"""
    rng = np.random.default_rng(211)
    qc = rng.uniform(0, 1, (Q, 3))
    n = coords[0].size
    at = rng.choice(n, 5, replace=False)
    qc[30:35] = np.stack([c[at].astype(np.float64) for c in coords], axis=1)
    reach = 2.0 if any(bc) else 40.0
    qc[35:] += rng.choice([-1.0, 1.0], (5, 3)) * rng.uniform(0.5, reach, (5, 3))
    return qc.astype(T)


class Run:
    def __init__(self, hip, rank, P):
        self.hip, self.rank, self.P, self.bad = hip, rank, P, []
        self.culprit = P - 1

    def fail(self, what, text):
        self.bad.append(f"rank {self.rank}, {what}: {text}")

    def raw(self, dom, r, qc, rmax, k, num_queries=None, null=(), with_rmax=True):
        """the C entry on sentinel-filled outputs with PAD more rows: (return code, outputs as numpy arrays)"""
        nq = qc.shape[0] if num_queries is None else num_queries
        cols = min(max(k, 1), 300)
        out = dict(ids=torch.full((Q + PAD, cols), SENT_ID, dtype=torch.int64, device="cuda"),
                   dist2=torch.full((Q + PAD, cols), ks.SENT_DIST, dtype=qc.dtype, device="cuda"),
                   counts=torch.full((Q + PAD,), ks.SENT_COUNT, dtype=torch.int32, device="cuda"))
        n = r["x"].numel() if r is not None else 0
        a = {name: (r[name].data_ptr() if n else None) for name in ("x", "y", "z")} if r is not None else dict(x=None, y=None, z=None)
        for name in null:
            a[name] = None
        torch.cuda.synchronize()
        rc = self.hip.lib.cstone_hip_domain_mr_knn(dom.h, a["x"], a["y"], a["z"], qc.data_ptr(),
                                                   rmax.data_ptr() if (with_rmax and rmax is not None) else None, nq, k,
                                                   out["ids"].data_ptr(), out["dist2"].data_ptr(), out["counts"].data_ptr())
        dom.coll.error = None
        self.hip.sync()
        return rc, {name: t.cpu().numpy() for name, t in out.items()}

    @staticmethod
    def clean(got, first_row=0):
        return ((got["ids"][first_row:] == SENT_ID).all() and (got["dist2"][first_row:] == ks.SENT_DIST).all() and
                (got["counts"][first_row:] == ks.SENT_COUNT).all())

    def refused(self, what, rc, got, mine, others):
        """every rank came back: the return codes of all ranks are gathered and checked on every rank"""
        codes = [None] * self.P
        dist.all_gather_object(codes, rc)
        want = [mine if p == self.culprit else others for p in range(self.P)]
        if codes != want or not self.clean(got):
            self.fail(what, f"return codes {codes}, expected {want}, or something was written")
        return codes

    def compare(self, what, got, ref, k):
        if not self.clean(got, first_row=Q) or (got["ids"][:Q, k:] != SENT_ID).any():
            self.fail(what, "something behind the rows was written")
        ids = got["ids"][:Q, :k].view(np.uint64)
        want = np.where(ref.neighbors == ks.NONE, np.uint64(0xFFFFFFFFFFFFFFFF), ref.neighbors.astype(np.uint64))
        if not np.array_equal(ids, want):
            rows = np.flatnonzero((ids != want).any(axis=1))
            self.fail(what, f"ids differ from the brute force over the whole cloud in queries {rows[:6].tolist()}")
        if got["dist2"][:Q, :k].tobytes() != ref.dist2.tobytes():
            self.fail(what, "dist2 differs in its bits")
        if not np.array_equal(got["counts"][:Q].view(np.uint32), ref.counts):
            self.fail(what, "counts differ")

    def cloud(self, name, ks_of_cloud=KS):
        import cstone_amd
        from cstone_amd.distributed import NativeDistributedDomain

        coords, bc = make_cloud(name)
        T = coords[0].dtype.type
        n = coords[0].size
        tdt = torch.float32 if T is np.float32 else torch.float64
        qc_h = make_queries(coords, bc, T)
        qc = torch.from_numpy(qc_h).cuda()
        statuses = {}

        dom = NativeDistributedDomain(self.hip, cstone_amd.HILBERT, 64, coords[0].itemsize * 8, 64, 16, [0.0, 1.0] * 3, bc)
        rc, got = self.raw(dom, None, qc, None, 8)
        statuses["no sync"] = self.refused(f"{name}, before the first sync", rc, got, E_ARG, E_ARG)

        mine = np.nonzero(np.random.default_rng(78).integers(0, self.P, n) == self.rank)[0]
        dev = [torch.from_numpy(c[mine].copy()).cuda() for c in coords]
        h = torch.full((mine.size,), 0.02, dtype=tdt, device="cuda")
        r = dom.sync(*dev, h)
        self.hip.sync()
        start, end = int(r["start"]), int(r["end"])

        # the whole cloud in global SFC order: the assigned ranges in rank order
        parts = [None] * self.P
        dist.all_gather_object(parts, [r[a][start:end].cpu().numpy() for a in "xyz"])
        whole = [np.concatenate([p[a] for p in parts]) for a in range(3)]
        assigned = [int(p[0].size) for p in parts]
        if whole[0].size != n:
            self.fail(name, f"the assigned ranges hold {whole[0].size} particles of {n}")
        lim = list(r["lim"])

        free = ks.Knn(whole, 0, n, lim, bc, qc_h, 6)
        with np.errstate(invalid="ignore"):
            d5 = np.sqrt(free.dist2[:, min(5, n - 1)].astype(np.float64))
        rmax_h = (d5 * 10.0 ** np.random.default_rng(212).uniform(-0.5, 1.5, Q)).astype(T)
        rmax_h[:4] = [0.0, np.nan, -float(d5[2]) * 3.0, np.inf]
        rmax = torch.from_numpy(rmax_h).cuda()

        for k in (0, 257):
            rc, got = self.raw(dom, r, qc, rmax, k)
            statuses[f"k {k}"] = self.refused(f"{name}, k = {k}", rc, got, E_ARG, E_ARG)
        if self.P > 1:
            last = self.rank == self.culprit
            rc, got = self.raw(dom, r, qc, rmax, 9 if last else 8)
            statuses["k differs"] = self.refused(f"{name}, another k on the last rank", rc, got, E_ARG, E_ARG)
            rc, got = self.raw(dom, r, qc, rmax, 8, num_queries=Q - 1 if last else Q)
            statuses["Q differs"] = self.refused(f"{name}, another Q on the last rank", rc, got, E_ARG, E_ARG)
            rc, got = self.raw(dom, r, qc, rmax, 8, with_rmax=not last)
            statuses["rmax differs"] = self.refused(f"{name}, no query_rmax on the last rank", rc, got, E_ARG, E_ARG)
        if min(assigned) > 0:  # (the same decision on every rank: what follows is collective)
            rc, got = self.raw(dom, r, qc, rmax, 8, null=("x",) if self.rank == self.culprit else ())
            statuses["null x"] = self.refused(f"{name}, a null x on the last rank", rc, got, E_ARG, E_INTERNAL)

        chunking = {}
        d2 = None
        for k in ks_of_cloud:
            for label, lim_h, lim_d in (("free", None, None), ("rmax", rmax_h, rmax)):
                what = f"{name}, k = {k}, {label}"
                ref = ks.Knn(whole, 0, n, lim, bc, qc_h, k, lim_h, d2=d2)
                d2 = ref.d2_table
                os.environ.pop(CAP_ENV, None)
                rc, got = self.raw(dom, r, qc, lim_d, k)
                if rc != 0:
                    self.fail(what, f"returned {rc}")
                    continue
                self.compare(what, got, ref, k)
                chunks, nbytes = dom.knn_last()
                if chunks != 1 or nbytes != (self.P * Q * k * 16 if self.P > 1 else 0) or nbytes > cstone_amd.KNN_MR_GATHER_BYTES:
                    self.fail(what, f"{chunks} chunks, {nbytes} bytes received under the default cap")
                everyone = [None] * self.P
                dist.all_gather_object(everyone, {key: got[key].tobytes() for key in got})
                if any(e != everyone[0] for e in everyone):
                    self.fail(what, "the ranks do not hold the same bits")
                # the chunked gather: a cap of a few KiB through the documented override; the same bits
                os.environ[CAP_ENV] = str(SMALL_CAP)
                rc, capped = self.raw(dom, r, qc, lim_d, k)
                os.environ.pop(CAP_ENV, None)
                chunks, nbytes = dom.knn_last()
                per = self.hip.lib.cstone_hip_knn_mr_chunk_queries(Q, k, self.P, SMALL_CAP)
                want_chunks = -(-Q // per)
                if rc != 0 or any(capped[key].tobytes() != got[key].tobytes() for key in got):
                    self.fail(what, "the capped call differs from the uncapped one")
                if per != max(1, min(Q, SMALL_CAP // (16 * k * self.P))) or chunks != want_chunks:
                    self.fail(what, f"{chunks} chunks of {per} queries, expected {want_chunks}")
                if self.P > 1 and (nbytes != self.P * per * k * 16 or nbytes > SMALL_CAP):
                    self.fail(what, f"the receive buffer took {nbytes} bytes under a cap of {SMALL_CAP}")
                chunking[f"{k} {label}"] = [int(chunks), int(nbytes)]
            ids3, d3, c3 = dom.knn(r["x"] if end > start else None, r["y"] if end > start else None,
                                   r["z"] if end > start else None, qc, k, query_rmax=rmax)
            self.hip.sync()
            if (ids3.cpu().numpy().tobytes() != got["ids"][:Q, :k].tobytes() or d3.cpu().numpy().tobytes() != got["dist2"][:Q, :k].tobytes()
                    or c3.cpu().numpy().tobytes() != got["counts"][:Q].tobytes()):
                self.fail(name, f"k = {k}: NativeDistributedDomain.knn differs from the C entry")
            if self.P == 1:
                o = dom.octree()
                nb5, d5_, c5 = self.hip.knn(r["x"], r["y"], r["z"], start, end, dom.view().box, o, o["layout"], o["centers"],
                                            o["sizes"], qc, k, query_rmax=rmax)
                self.hip.sync()
                nb5 = nb5.cpu().numpy().view(np.uint32)
                as_ids = np.where(nb5 == ks.NONE, np.uint64(0xFFFFFFFFFFFFFFFF), nb5.astype(np.uint64) - np.uint64(start))
                if (not np.array_equal(as_ids, got["ids"][:Q, :k].view(np.uint64)) or d5_.cpu().numpy().tobytes() != got["dist2"][:Q, :k].tobytes()
                        or c5.cpu().numpy().tobytes() != got["counts"][:Q].tobytes()):
                    self.fail(name, f"k = {k}: one rank: the output differs from cstone_hip_knn with indices turned into ids")
        dom.close()
        return dict(statuses=statuses, assigned=assigned, chunking=chunking, full_rows=int((ref.counts == ks_of_cloud[-1]).sum()))


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
            figs[name] = run.cloud(name, (8, 100, 256) if name.startswith("sparse") else KS)
    except Exception as e:  # (the other ranks may now wait in a collective: the launcher's timeout ends them)
        import traceback

        traceback.print_exc()
        print("KNN_MR_RESULT " + json.dumps(dict(ok=False, ranks=P, bad=run.bad + [f"rank {rank}: {type(e).__name__}: {e}"])),
              flush=True)
        os._exit(1)
    allbad = [None] * P
    dist.all_gather_object(allbad, run.bad)
    flat = [b for part in allbad for b in part]
    if rank == 0:
        print("KNN_MR_RESULT " + json.dumps(dict(ok=not flat, ranks=P, bad=flat[:20], clouds=figs), default=float), flush=True)
    dist.destroy_process_group()
    sys.exit(0 if not flat else 1)


if __name__ == "__main__":
    main()
