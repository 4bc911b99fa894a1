"""The friends-of-friends group catalogue across ranks (cstone_hip_domain_mr_fof_catalog, NativeDistributedDomain.fof_catalog):
on 1 to 4 ranks the union of the ranks' tables against the brute force over the whole cloud and the numpy rule of
tests/fof_props_support.py (tests/fof_catalog_mr_worker.py), the refusals, the capacity, and one rank == the single-rank call.

Every group is listed by exactly one rank, the owner of its lowest global id; labels, sizes and the MASSLESS bit are
compared with ==, mass and velocity within the derived bounds for every group, centre and radius for every group whose
WIDE flag is clear in the result.  What that condition may leave out is capped: WIDE must be set wherever the rule sets
it and ONLY on groups with a member at least an eighth of the box from the reference -- closer than that every two
members are within a quarter, and neither a partial nor a shift can be wide.

The clouds are those of tests/fof_mr_support.py.  At their b of 0.9 mean separations the periodic uniform clouds are not
the handful of small groups one might expect: the numpy rule finds 554 groups, one of 4 219 members that percolates, and
sets WIDE on two of them (test_premises_of_the_clouds pins this).  So "no group is WIDE" is asserted for the open uniform
cloud only, where it holds; for the periodic ones the cap above is asserted instead, and the test prints how many groups
had their geometry compared (all but a few of the 554).  And the three uniform clouds run a second time on the same sync at
a linking length of HALF the mean separation, where the premise does hold (test_premises_at_half_the_mean_separation:
some 4 600 groups of at most ten members, none with a member an eighth of the box from its reference): there WIDE must be
clear on every group and centre and radius of every group are compared across ranks, nothing left out.  The serpentine -- one chain through the whole box -- must be
flagged, with mass, size and velocity still compared."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fof_mr_support as ms
import fof_props_support as ps
import fof_support as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_premises = {}


def premises(name):
    """(reference groups, labels) of a cloud in the order it is generated in, min_members 1: once per session"""
    if name not in _premises:
        from helpers import Box

        (x, y, z), b, bc = ms.cloud(name)
        lim = [0.0, 1.0] * 3
        labels, sizes, ng = ms.groups_of(x, y, z, b, Box(lim, bc))
        off, mem = fs.catalog_of(labels, 0, 1)
        m, vel = ps.seeded_fields(np.arange(x.size), x.dtype.type, x.size)
        _premises[name] = (ps.catalogue_reference([x, y, z], m, vel, off, mem, lim, bc), ng)
    return _premises[name]


def test_header_declares_and_the_bindings_export_the_call():
    import cstone_amd

    text = open(os.path.join(ROOT, "include", "cstone_hip.h")).read()
    assert re.search(r"\bint cstone_hip_domain_mr_fof_catalog\(", text)
    assert "cstone_hip_domain_mr_fof_catalog" in cstone_amd.EXPORTS
    assert hasattr(cstone_amd.load_library(), "cstone_hip_domain_mr_fof_catalog")
    from cstone_amd.distributed import NativeDistributedDomain

    assert callable(NativeDistributedDomain.fof_catalog)


@pytest.mark.parametrize("name", list(ms.CLOUDS))
def test_premises_of_the_clouds(name):
    """what the worker's flag assertions rest on, from the numpy rule alone"""
    refs, ng = premises(name)
    wide = sum(1 for g in refs if g.flags & ps.WIDE)
    far = sum(1 for g in refs if g.dmax >= 0.125)
    print(f"{name}: {ng} groups, largest {max(g.n for g in refs)}, WIDE by the rule {wide}, with a member an eighth of the "
          f"box away {far}")
    assert not any(g.flags & ps.MASSLESS for g in refs)
    if name == "uniform-open":
        assert wide == 0 and ng > 100
    elif name.startswith("uniform-pbc"):
        assert ng == 554 and max(g.n for g in refs) == 4219 and wide == 2 and far == 24  # (not "a few particles")
    else:
        assert ng == 1 and wide == 1


@pytest.mark.parametrize("name", [n for n in ms.CLOUDS if n.startswith("uniform")])
def test_premises_at_half_the_mean_separation(name):
    """the second pass of the uniform clouds: small groups only, so that not even the conservative flag can be set"""
    from helpers import Box

    (x, y, z), _, bc = ms.cloud(name)
    lim, b2 = [0.0, 1.0] * 3, 0.5 * x.size ** (-1.0 / 3.0)
    labels, sizes, ng = ms.groups_of(x, y, z, b2, Box(lim, bc))
    off, mem = fs.catalog_of(labels, 0, 1)
    m, vel = ps.seeded_fields(np.arange(x.size), x.dtype.type, x.size)
    refs = ps.catalogue_reference([x, y, z], m, vel, off, mem, lim, bc)
    assert ng > 4000 and 2 < sizes.max() <= 10 and (np.diff(off.astype(np.int64)) > 1).sum() > 900
    assert not any(g.flags for g in refs) and max(g.dmax for g in refs) < 0.125


def _launch(nproc, port, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "fof_catalog_mr_worker.py")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("FOF_CATALOG_MR_RESULT ")]
    assert lines, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(lines[-1][len("FOF_CATALOG_MR_RESULT "):])
    print(json.dumps(res))
    assert p.returncode == 0 and res["ok"], str(res["bad"])[:3000] + p.stderr[-2000:]
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [1, 2, 3, 4])
def test_hip_fof_catalogue_across_ranks(nproc):
    """every cloud of fof_mr_support.CLOUDS on nproc gloo ranks that share the GPU, min_members 1 and 3: the comparison of
    the module's docstring; tables ascend and list only labels their rank owns; two calls identical; the Python method ==
    the C entry; without velocities the velocity rows stay untouched; a capacity one too small on the rank with the most
    groups is CSTONE_E_CAPACITY there alone, with the count set and nothing written; a call before the first sync, a null x
    on one rank and a label outside [0, total) on one rank are refused on every rank, write nothing and leave the domain
    usable; on one rank the bits == cstone_hip_fof_group_properties on the catalogue of the same labels; the uniform clouds
    once more at half the mean separation, no group WIDE and the geometry of every group compared"""
    res = _launch(nproc, 29970 + nproc)
    assert res["ranks"] == nproc and set(res["clouds"]) == set(ms.CLOUDS)
    for name, figs in res["clouds"].items():
        ng = premises(name)[1]
        uniform = name.startswith("uniform")
        assert set(figs) == {"min1", "min3"} | ({"half"} if uniform else set())
        assert figs["min1"]["groups"] == ng and 0 < figs["min3"]["groups"] <= ng
        if uniform:
            half = figs.pop("half")
            assert half["groups"] > 4000 and half["largest"] <= 10 and half["wide"] == 0
            assert half["geometry_compared"] == half["groups"] == sum(half["per_rank"])
        for f in figs.values():
            assert sum(f["per_rank"]) == f["groups"] and f["wide"] >= f["rule_wide"]
            assert f["geometry_compared"] == f["groups"] - f["wide"]
            if name.startswith("uniform-pbc"):
                # (the worker lets WIDE stand only on groups with a member an eighth of the box away: 24 of the 554)
                assert f["wide"] <= sum(1 for g in premises(name)[0] if g.dmax >= 0.125)
            if name == "uniform-open":
                assert f["wide"] == 0
