"""One rank of tests/test_fof_catalog_mr.py: NativeDistributedDomain.fof_catalog (cstone_hip_domain_mr_fof_catalog) on the
clouds of tests/fof_mr_support.py.  Started by `python -m torch.distributed.run`; the ranks talk over gloo and share the
one GPU.  Every particle carries its index in the generated cloud and m, vx, vy, vz -- functions of that index
(fof_props_support.seeded_fields) -- through the sync as properties.  Rank 0 compares the union of the ranks' tables with
the brute force over the WHOLE cloud (fof_mr_support.groups_of) and the numpy rule (fof_props_support) about every group's
lowest global id, and prints one line `FOF_CATALOG_MR_RESULT {json}`.

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
import fof_props_support as ps  # noqa: E402
import fof_support as fs  # noqa: E402
from helpers import Box  # noqa: E402

E_ARG, E_CAPACITY, E_INTERNAL = -1, -2, -4
SENT = -777.25
KEYS = ("labels", "sizes", "mass", "center", "velocity", "radius", "flags")


def u64(t):
    return t.cpu().numpy().view(np.uint64)


class Run:
    def __init__(self, hip, rank, P):
        self.hip, self.rank, self.P, self.bad = hip, rank, P, []

    def fail(self, what, text):
        self.bad.append(f"rank {self.rank}, {what}: {text}")

    def sync(self, dom, coords, h_value):
        n = coords[0].size
        T = coords[0].dtype.type
        mine = np.nonzero(np.random.default_rng(78).integers(0, self.P, n) == self.rank)[0]
        dev = [torch.from_numpy(c[mine].copy()).cuda() for c in coords]
        h = torch.full((mine.size,), h_value, dtype=dev[0].dtype, device="cuda")
        m, vel = ps.seeded_fields(mine, T, n)
        props = [torch.from_numpy(mine.astype(np.int64)).cuda()] + [torch.from_numpy(a).cuda() for a in (m, *vel)]
        r = dom.sync(*dev, h, props=props)
        r["index"], r["m"] = r["props"][0].clone(), r["props"][1].clone()
        r["vel"] = [p.clone() for p in r["props"][2:5]]
        return r

    def raw(self, dom, r, labels, min_members=1, capacity=None, null=(), velocities=True):
        """the C entry on sentinel-filled outputs: (return code, number of groups, outputs as numpy arrays)"""
        n = r["x"].numel() if r is not None else 0
        tdt = r["x"].dtype if r is not None else torch.float64
        na = (r["end"] - r["start"]) if r is not None else 0
        cap = max(na, 1) if capacity is None else capacity
        rows = cap + 3
        out = dict(labels=torch.full((rows,), -7, dtype=torch.int64, device="cuda"),
                   sizes=torch.full((rows,), -7, dtype=torch.int64, device="cuda"),
                   mass=torch.full((rows,), SENT, dtype=tdt, device="cuda"),
                   center=torch.full((rows, 3), SENT, dtype=tdt, device="cuda"),
                   velocity=torch.full((rows, 3), SENT, dtype=tdt, device="cuda"),
                   radius=torch.full((rows,), SENT, dtype=tdt, device="cuda"),
                   flags=torch.full((rows,), -1, dtype=torch.int32, device="cuda"))
        ptr = (lambda t: t.data_ptr() if (n and t is not None) else None)
        a = dict(x=ptr(r["x"]), y=ptr(r["y"]), z=ptr(r["z"]), m=ptr(r["m"])) if r is not None else dict(x=None, y=None, z=None, m=None)
        v = [ptr(t) for t in r["vel"]] if (r is not None and velocities) else [None] * 3
        for k in null:
            a[k] = None
        ng = C.c_uint32(4242)
        rc = self.hip.lib.cstone_hip_domain_mr_fof_catalog(
            dom.h, a["x"], a["y"], a["z"], a["m"], (r["m"].element_size() * 8) if r is not None else 64, *v, ptr(labels),
            min_members, cap, *[out[k].data_ptr() for k in KEYS], C.byref(ng))
        dom.coll.error = None
        self.hip.sync()
        got = {k: t.cpu().numpy() for k, t in out.items()}
        for k in ("labels", "sizes"):
            got[k] = got[k].view(np.uint64)
        got["flags"] = got["flags"].view(np.uint32)
        return rc, ng.value, got

    @staticmethod
    def clean(got, first_row=0):
        return all((got[k][first_row:] == (np.uint64(-7 & (2 ** 64 - 1)) if k in ("labels", "sizes") else
                                           np.uint32(0xFFFFFFFF) if k == "flags" else SENT)).all() for k in KEYS)

    def check(self, what, name, coords, b, bc, min_members, parts, all_clear=False):
        """rank 0: the union of the tables against the brute force over the whole cloud and the numpy rule; all_clear: no
        group may be WIDE, so that centre and radius of EVERY group are compared"""
        n = coords[0].size
        T = coords[0].dtype.type
        order = np.concatenate([p["index"][p["start"]:p["end"]] for p in parts])  # global id -> cloud index
        if not np.array_equal(np.sort(order), np.arange(n)):
            self.fail(what, "the ranks do not hold every particle once")
            return {}
        lim = list(parts[0]["lim"])
        pos = [c[order] for c in coords]
        ref_labels, ref_sizes, _ = ms.groups_of(*pos, b, Box(lim, bc))
        off, mem = fs.catalog_of(ref_labels, 0, min_members)
        m, vel = ps.seeded_fields(order, T, n)
        refs = ps.catalogue_reference(pos, m, vel, off, mem, lim, bc)
        want = mem[off[:-1]].astype(np.uint64)  # the groups' labels, ascending
        bounds = np.concatenate([[0], np.cumsum([p["end"] - p["start"] for p in parts])]).astype(np.uint64)
        for q, p in enumerate(parts):
            lab = p["table"]["labels"]
            if not ((lab >= bounds[q]) & (lab < bounds[q + 1])).all():
                self.fail(what, f"rank {q} lists a group whose label it does not own")
            if not (np.diff(lab.astype(np.int64)) > 0).all():
                self.fail(what, f"the table of rank {q} does not ascend")
        got = {k: np.concatenate([p["table"][k] for p in parts]) for k in KEYS}
        if not np.array_equal(got["labels"], want):  # (owners hold ascending id ranges: the union ascends too)
            self.fail(what, f"the tables list {got['labels'].size} groups, not the {want.size} of the brute force, or other labels")
            return {}
        if not np.array_equal(got["sizes"], np.diff(off.astype(np.int64)).astype(np.uint64)):
            self.fail(what, "group sizes differ from the brute force")
        shifts = [g.dmax if self.P > 1 else 0.0 for g in refs]  # (r_p is a member: |s| <= dmax)
        bad, worst = ps.compare(got, refs, T, lim, bc, shifts=shifts, skip_wide_geometry=True, flags_equal=False)
        for text in bad[:6]:
            self.fail(what, text)
        # the flags.  MASSLESS: with ==.  WIDE is conservative across ranks: never missing where the rule sets it, and set
        # only where some member is at least an eighth of the box from the reference (closer than that, every two members
        # are within a quarter: no partial and no shift can be wide).  This caps what the geometry comparison leaves out
        L = min(float(v) for v, c in zip(ps.box_lengths(T, lim), bc) if c == 1) if any(c == 1 for c in bc) else np.inf
        wide = (got["flags"] & ps.WIDE) != 0
        ref_wide = np.array([bool(g.flags & ps.WIDE) for g in refs])
        far = np.array([g.dmax >= 0.125 * L for g in refs])
        if ((got["flags"] & ps.MASSLESS) != 0).any() or (ref_wide & ~wide).any() or (wide & ~far).any():
            self.fail(what, "flags: MASSLESS set, WIDE missing where the rule sets it, or WIDE set on a compact group")
        if self.P == 1 and not np.array_equal(wide, ref_wide):
            self.fail(what, "one rank: WIDE differs from the rule's")
        if name == "uniform-open" and wide.any():
            self.fail(what, "WIDE in an open box")
        if all_clear and (wide.any() or far.any()):
            self.fail(what, "a group is WIDE, or has a member an eighth of the box away: geometry was left out")
        if name == "serpentine" and not wide.all():
            self.fail(what, "the serpentine is not flagged")
        return dict(groups=int(want.size), largest=int(got["sizes"].max(initial=0)), wide=int(wide.sum()),
                    rule_wide=int(ref_wide.sum()), geometry_compared=int((~wide).sum()), worst=worst,
                    per_rank=[int(p["table"]["labels"].size) for p in parts])

    def cloud(self, name):
        import cstone_amd
        from cstone_amd.distributed import NativeDistributedDomain

        coords, b, bc = ms.cloud(name)
        T = coords[0].dtype.type
        dom = NativeDistributedDomain(self.hip, cstone_amd.HILBERT, 64, coords[0].itemsize * 8, 64, 16, [0.0, 1.0] * 3, bc)
        rc, ng, got = self.raw(dom, None, None)
        if rc != E_ARG or ng != 4242 or not self.clean(got):
            self.fail(name, f"a call before the first sync returned {rc} or wrote something")
        r = self.sync(dom, coords, T(0.6 * b))
        rc, ng, got = self.raw(dom, r, torch.zeros(r["x"].numel(), dtype=torch.int64, device="cuda"))
        if rc != E_ARG or ng != 4242 or not self.clean(got):
            self.fail(name, f"a call without domain_mr_fof since the sync returned {rc} or wrote something")
        labels, _, _, _ = dom.fof(r["x"], r["y"], r["z"], b, want_sizes=False)

        # a null x on the last rank only: every rank fails, nothing is written, the domain stays usable
        rc, ng, got = self.raw(dom, r, labels, null=("x",) if self.rank == self.P - 1 else ())
        if rc != (E_ARG if self.rank == self.P - 1 else E_INTERNAL) or ng != 4242 or not self.clean(got):
            self.fail(name, f"a null x on the last rank: returned {rc} or wrote something")
        bad_labels = labels.clone()
        if self.rank == 0:
            bad_labels[r["start"]] = 2 ** 40
        rc, ng, got = self.raw(dom, r, bad_labels)
        if rc != (E_ARG if self.rank == 0 else E_INTERNAL) or not self.clean(got):
            self.fail(name, f"a label outside [0, total) on rank 0: returned {rc} or wrote something")

        figs = {}
        for mm in (1, 3):
            what = f"{name}, min_members {mm}"
            rc, ng, got = self.raw(dom, r, labels, mm)
            rc2, ng2, again = self.raw(dom, r, labels, mm)
            if rc != 0 or rc2 != 0:
                self.fail(what, f"returned {rc}, {rc2}")
                continue
            if ng != ng2 or any(got[k].tobytes() != again[k].tobytes() for k in KEYS):
                self.fail(what, "two calls do not give identical results")
            if not self.clean(got, first_row=ng):
                self.fail(what, "rows behind the last group were written")
            t = dom.fof_catalog(r["x"], r["y"], r["z"], r["m"], labels, vel=r["vel"], min_members=mm)
            self.hip.sync()
            if any(t[i].cpu().numpy().tobytes() != got[k][:ng].tobytes() for i, k in enumerate(KEYS)):
                self.fail(what, "NativeDistributedDomain.fof_catalog differs from the C entry")
            # without velocities: the velocity rows stay untouched, the rest is the same
            rc3, ng3, nov = self.raw(dom, r, labels, mm, velocities=False)
            if rc3 != 0 or ng3 != ng or (nov["velocity"] != SENT).any() or any(
                    nov[k].tobytes() != got[k].tobytes() for k in KEYS if k != "velocity"):
                self.fail(what, "the call without velocities differs or wrote velocities")
            # a capacity one too small on the rank with the most groups: that rank alone is refused, with the count set
            counts = [None] * self.P
            dist.all_gather_object(counts, ng)
            most = int(np.argmax(counts))
            short = self.rank == most and ng > 0
            rc4, ng4, small = self.raw(dom, r, labels, mm, capacity=ng - 1 if short else None)
            if rc4 != (E_CAPACITY if short else 0) or ng4 != ng or (short and not self.clean(small)):
                self.fail(what, f"capacity one short on rank {most}: returned {rc4}, count {ng4} of {ng}, or wrote something")
            if self.P == 1 and mm == 1:
                self.one_rank_bits(what, dom, r, labels, got, ng)
            table = {k: got[k][:ng] for k in KEYS}
            mine = dict(index=r["index"].cpu().numpy(), start=r["start"], end=r["end"], lim=r["lim"], table=table)
            parts = [None] * self.P
            dist.all_gather_object(parts, mine)
            if self.rank == 0:
                figs[f"min{mm}"] = self.check(what, name, coords, b, bc, mm, parts)
        if name.startswith("uniform"):
            # the same sync at HALF the mean separation (its halos reach further than that): thousands of groups of at most
            # ten members, none near an eighth of the box wide -- no WIDE flag, centre and radius of every group compared
            what, b2 = f"{name}, b of half the mean separation", 0.5 * coords[0].size ** (-1.0 / 3.0)
            labels2, _, _, _ = dom.fof(r["x"], r["y"], r["z"], b2, want_sizes=False)
            rc, ng, got = self.raw(dom, r, labels2, 1)
            if rc != 0:
                self.fail(what, f"returned {rc}")
            mine = dict(index=r["index"].cpu().numpy(), start=r["start"], end=r["end"], lim=r["lim"],
                        table={k: got[k][:ng] for k in KEYS})
            parts = [None] * self.P
            dist.all_gather_object(parts, mine)
            if self.rank == 0:
                figs["half"] = self.check(what, name, coords, b2, bc, 1, parts, all_clear=True)
        dom.close()
        return figs

    def one_rank_bits(self, what, dom, r, labels, got, ng):
        """a communicator of one rank: the bits of cstone_hip_fof_group_properties on the catalogue of the same labels"""
        st, en = r["start"], r["end"]
        lab32 = (labels[st:en] + st).to(torch.int32)
        off, mem = self.hip.fof_catalog(lab32, st, en, 1)
        single = self.hip.fof_group_properties(r["x"], r["y"], r["z"], r["m"], off, mem, dom.view().box, vel=r["vel"])
        self.hip.sync()
        if off.numel() - 1 != ng:
            self.fail(what, "one rank: the single-rank catalogue has another number of groups")
            return
        for t, k in zip(single, ("mass", "center", "velocity", "radius", "flags")):
            if t.cpu().numpy().tobytes() != got[k][:ng].tobytes():
                self.fail(what, f"one rank: {k} differs in its bits from cstone_hip_fof_group_properties")
        if not np.array_equal(got["labels"][:ng], mem.cpu().numpy().view(np.uint32)[off.cpu().numpy()[:-1]] - np.uint32(st)):
            self.fail(what, "one rank: the labels are not the first members of the single-rank catalogue")


def main():
    dist.init_process_group("gloo")
    rank, P = dist.get_rank(), dist.get_world_size()
    import cstone_amd

    torch.cuda.set_device(0)
    run = Run(cstone_amd.Context(0), rank, P)
    figs = {}
    try:
        for name in ms.CLOUDS:
            figs[name] = run.cloud(name)
    except Exception as e:  # (the other ranks may now wait in a collective: the launcher's timeout ends them)
        import traceback

        traceback.print_exc()
        print("FOF_CATALOG_MR_RESULT " + json.dumps(dict(ok=False, ranks=P, bad=run.bad + [f"rank {rank}: {type(e).__name__}: {e}"])),
              flush=True)
        os._exit(1)
    allbad = [None] * P
    dist.all_gather_object(allbad, run.bad)
    flat = [b for part in allbad for b in part]
    if rank == 0:
        print("FOF_CATALOG_MR_RESULT " + json.dumps(dict(ok=not flat, ranks=P, bad=flat[:20], clouds=figs), default=float),
              flush=True)
    dist.destroy_process_group()
    sys.exit(0 if not flat else 1)


if __name__ == "__main__":
    main()
