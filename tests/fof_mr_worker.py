"""One rank of tests/test_fof_mr.py: NativeDistributedDomain.fof (cstone_hip_domain_mr_fof) on the clouds of
tests/fof_mr_support.py, checked on rank 0 against the brute force over the WHOLE cloud and the numpy restatement of the
rounds.  Started by `python -m torch.distributed.run`; the ranks talk over gloo and share the one GPU.  Every particle
carries its index in the generated cloud as a property; the sync uses h = 0.6 b and a halo factor of 1, so the halos
reach 1.2 b.  Rank 0 prints one line `FOF_MR_RESULT {json}`.  Cloud names on the command line replace the default set
(tests/test_face_pairs.py runs "faces" that way).

A failed check is recorded and the rank goes on, so that no rank waits in a collective for one that has stopped."""
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
from helpers import Box  # noqa: E402

SENT = -0x0123456789ABCDF  # what the outputs hold before a call that must write nothing
E_ARG, E_INTERNAL = -1, -4
OWNER_SIDE = "uniform-open, owner-side halos"


def u64(t):
    return t.cpu().numpy().view(np.uint64)


class Run:
    def __init__(self, hip, rank, P):
        self.hip, self.rank, self.P, self.bad = hip, rank, P, []

    def fail(self, what, text):
        self.bad.append(f"rank {self.rank}, {what}: {text}")

    def domain(self, rb, bc, owner_side, lim=None):
        import cstone_amd
        from cstone_amd.distributed import NativeDistributedDomain

        mode = NativeDistributedDomain.HALOS_OWNER_SIDE if owner_side else None  # (None: the locally essential tree)
        return NativeDistributedDomain(self.hip, cstone_amd.HILBERT, 64, rb, 64, 16, lim or [0.0, 1.0] * 3, bc, halo_mode=mode)

    def sync(self, dom, coords, h_value):
        """this rank's share of the cloud (drawn at random) through a sync; the cloud index follows as a property"""
        n = coords[0].size
        mine = np.nonzero(np.random.default_rng(78).integers(0, self.P, n) == self.rank)[0]
        dev = [torch.from_numpy(c[mine].copy()).cuda() for c in coords]
        h = torch.full((mine.size,), h_value, dtype=dev[0].dtype, device="cuda")
        r = dom.sync(*dev, h, props=[torch.from_numpy(mine.astype(np.int64)).cuda()])
        r["index"] = r["props"][0].clone()
        dom.exchange_halos(r["index"])
        return r

    def raw_call(self, dom, r, b, max_rounds=0, null=()):
        """the C entry on arrays filled with a sentinel: (return code, labels and sizes still hold the sentinel)"""
        n = r["x"].numel() if r is not None else 0
        labels = torch.full((n,), SENT, dtype=torch.int64, device="cuda")
        sizes = torch.full((n,), SENT, dtype=torch.int64, device="cuda")
        ptr = (lambda t: t.data_ptr() if n else None)
        ng, rounds = C.c_uint64(12345), C.c_uint32(54321)
        xyz = [ptr(r[c]) if c not in null else None for c in "xyz"] if r is not None else [None] * 3
        rc = self.hip.lib.cstone_hip_domain_mr_fof(dom.h, *xyz, b, max_rounds, ptr(labels), ptr(sizes), C.byref(ng),
                                                   C.byref(rounds))
        dom.coll.error = None
        self.hip.sync()
        clean = bool((labels == SENT).all()) and bool((sizes == SENT).all()) and (ng.value, rounds.value) == (12345, 54321)
        return rc, clean

    def refused(self, dom, r, b, what, code=E_ARG, max_rounds=0, null=()):
        rc, clean = self.raw_call(dom, r, b, max_rounds, null)
        if rc != code:
            self.fail(what, f"returned {rc}, {code} was expected")
        if not clean:
            self.fail(what, "the refused call wrote to its outputs")

    def gather(self, r, res):
        labels, sizes, ng, rounds = res
        st, en = r["start"], r["end"]
        mine = dict(x=r["x"].cpu().numpy(), y=r["y"].cpu().numpy(), z=r["z"].cpu().numpy(), index=r["index"].cpu().numpy(),
                    start=st, end=en, labels=u64(labels), sizes=u64(sizes), ng=ng, rounds=rounds, lim=r["lim"])
        parts = [None] * self.P
        dist.all_gather_object(parts, mine)
        return parts

    def check(self, name, coords, b, bc, parts):
        """rank 0: everything the ranks report against the brute force over the whole cloud and the restated rounds"""
        what, n = name, coords[0].size
        order = np.concatenate([p["index"][p["start"]:p["end"]] for p in parts])  # global id -> cloud index
        if not np.array_equal(np.sort(order), np.arange(n)):
            self.fail(what, "the ranks do not hold every particle once")
            return {}
        gid = np.empty(n, dtype=np.int64)
        gid[order] = np.arange(n)
        box = Box(list(parts[0]["lim"]), bc)
        ref_labels, ref_sizes, ref_ng = ms.groups_of(*[c[order] for c in coords], b, box)
        model = []
        for q, p in enumerate(parts):
            ids = gid[p["index"]]
            st, en = p["start"], p["end"]
            for c, axis in zip(coords, "xyz"):
                if not np.array_equal(p[axis], c[p["index"]]):
                    self.fail(what, f"rank {q}: the cloud index does not lead back to {axis}")
            halo = np.ones(ids.size, dtype=bool)
            halo[st:en] = False
            for key, ref in (("labels", ref_labels), ("sizes", ref_sizes)):
                for rng_name, sel in (("assigned", ~halo), ("halo", halo)):
                    wrong = np.flatnonzero((p[key] != ref[ids].astype(np.uint64)) & sel)
                    if wrong.size:
                        self.fail(what, f"rank {q}: {wrong.size} {rng_name} {key} differ from the brute force, first "
                                        f"{wrong[:4].tolist()}: {p[key][wrong[:4]].tolist()} / {ref[ids][wrong[:4]].tolist()}")
            if p["ng"] != ref_ng:
                self.fail(what, f"rank {q}: {p['ng']} groups, the brute force has {ref_ng}")
            model.append(ms.RankPart(p["x"], p["y"], p["z"], ids, st, en))
        model_labels, model_rounds = ms.model_rounds(model, b, box)
        for q, (p, lab) in enumerate(zip(parts, model_labels)):
            if not np.array_equal(lab, ref_labels[model[q].ids.astype(np.int64)].astype(np.uint64)):
                self.fail(what, f"rank {q}: the restated rounds do not end at the brute force's labels")
            if p["rounds"] != model_rounds:
                self.fail(what, f"rank {q}: {p['rounds']} rounds, the restatement makes {model_rounds}")
        figs = dict(groups=ref_ng, largest=int(ref_sizes.max()), rounds=int(parts[0]["rounds"]), model_rounds=model_rounds,
                    halos=[int(p["x"].size - (p["end"] - p["start"])) for p in parts])
        if name == "faces":
            # the fitted limits are the box's (the faces are faces of the domain's cells); the pairs 2p, 2p + 1 that the
            # brute force puts into one group, and those of them whose two particles belong to different ranks
            if not np.array_equal(np.asarray(parts[0]["lim"]), np.asarray(ms.cloud_limits(name))):
                self.fail(what, f"the domain's limits {list(parts[0]['lim'])} are not the box's")
            owner = np.empty(n, dtype=np.int64)
            for q, p in enumerate(parts):
                owner[p["index"][p["start"]:p["end"]]] = q
            even = np.arange(0, ms.FACES_N, 2)
            joined = ref_labels[gid[even]] == ref_labels[gid[even + 1]]
            figs.update(pairs=int(even.size), pairs_joined=int(joined.sum()),
                        joined_across_ranks=int((joined & (owner[even] != owner[even + 1])).sum()))
        return figs

    def one_rank_equals_the_single_rank_call(self, name, dom, r, b, res):
        """world of one rank: labels - start_index == cstone_hip_friends_of_friends on the assigned range of the same arrays"""
        st, en = r["start"], r["end"]
        o, v = dom.octree(), dom.view()
        l1, s1, n1 = self.hip.friends_of_friends(r["x"], r["y"], r["z"], st, en, v.box, o, o["layout"], o["centers"],
                                                 o["sizes"], b)
        self.hip.sync()
        labels, sizes, ng, rounds = res
        if not np.array_equal(u64(labels)[st:en] + np.uint64(st), l1.cpu().numpy().view(np.uint32).astype(np.uint64)):
            self.fail(name, "labels differ from the single-rank call's")
        if not np.array_equal(u64(sizes)[st:en], s1.cpu().numpy().view(np.uint32).astype(np.uint64)) or ng != n1:
            self.fail(name, "sizes or the number of groups differ from the single-rank call's")
        if rounds != 2:
            self.fail(name, f"{rounds} rounds on one rank, 2 were expected")

    def cloud(self, name, owner_side=False):
        coords, b, bc = ms.cloud(name)
        T = coords[0].dtype.type
        what = name + (", owner-side halos" if owner_side else "")
        dom = self.domain(coords[0].itemsize * 8, bc, owner_side, ms.cloud_limits(name))
        self.refused(dom, None, b, f"{what}, a call before the first sync")

        # ---- a sync whose halos do not reach b: h = 0.4 b
        r = self.sync(dom, coords, T(0.4 * b))
        if self.P > 1:
            self.refused(dom, r, b, f"{what}, b beyond the halo radius (h = 0.4 b)")
        else:  # (one rank: every particle is on the rank, there is nothing to cover)
            short = dom.fof(r["x"], r["y"], r["z"], b)

        # ---- the sync of the set-up: h = 0.6 b
        r = self.sync(dom, coords, T(0.6 * b))
        if bc[0] == 1:
            self.refused(dom, r, 0.5, f"{what}, b of half the periodic edge")
        self.refused(dom, r, float("nan"), f"{what}, a NaN")
        self.refused(dom, r, 0.0, f"{what}, b = 0")
        # a null x on the last rank only: that rank's own refusal, the others learn of it; nothing is written
        last = self.rank == self.P - 1
        self.refused(dom, r, b, f"{what}, a null x on the last rank", code=E_ARG if last else E_INTERNAL,
                     null=("x",) if last else ())
        if name == "serpentine" and self.P > 1:
            self.refused(dom, r, b, f"{what}, max_rounds = 1", code=E_INTERNAL, max_rounds=1)
        res = dom.fof(r["x"], r["y"], r["z"], b)
        again = dom.fof(r["x"], r["y"], r["z"], b)
        self.hip.sync()
        if not (torch.equal(res[0], again[0]) and torch.equal(res[1], again[1]) and res[2:] == again[2:]):
            self.fail(what, "two calls do not give identical results")
        without = dom.fof(r["x"], r["y"], r["z"], b, want_sizes=False)
        if without[1] is not None or not torch.equal(without[0], res[0]) or without[2:] != res[2:]:
            self.fail(what, "the call without sizes differs")
        if self.P == 1:
            self.one_rank_equals_the_single_rank_call(what, dom, r, b, res)
            if not (torch.equal(short[0], res[0]) and torch.equal(short[1], res[1])):
                self.fail(what, "one rank: the labels depend on the h of the sync")
        parts = self.gather(r, res)
        figs = self.check(what, coords, b, bc, parts) if self.rank == 0 else {}
        if name == "serpentine" and self.P > 1 and res[3] < 8:
            self.fail(what, f"only {res[3]} rounds: the loop hardly iterates")
        dom.close()
        return figs


def main():
    dist.init_process_group("gloo")
    rank, P = dist.get_rank(), dist.get_world_size()
    import cstone_amd

    torch.cuda.set_device(0)
    run = Run(cstone_amd.Context(0), rank, P)
    figs = {}
    try:
        if len(sys.argv) > 1:  # the clouds named on the command line only
            for name in sys.argv[1:]:
                figs[name] = run.cloud(name)
        else:
            for name in ms.CLOUDS:
                figs[name] = run.cloud(name)
            # the other way of finding halos keeps its radii elsewhere and exchanges halos along other routes
            figs[OWNER_SIDE] = run.cloud("uniform-open", owner_side=True)
    except Exception as e:  # (the other ranks may now wait in a collective: the launcher's timeout ends them)
        import traceback

        traceback.print_exc()
        print("FOF_MR_RESULT " + json.dumps(dict(ok=False, ranks=P, bad=run.bad + [f"rank {rank}: {type(e).__name__}: {e}"])),
              flush=True)
        os._exit(1)
    allbad = [None] * P
    dist.all_gather_object(allbad, run.bad)
    flat = [b for part in allbad for b in part]
    if rank == 0:
        print("FOF_MR_RESULT " + json.dumps(dict(ok=not flat, ranks=P, bad=flat[:20], clouds=figs), default=float), flush=True)
    dist.destroy_process_group()
    sys.exit(0 if not flat else 1)


if __name__ == "__main__":
    main()
