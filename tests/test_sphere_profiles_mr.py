"""Sphere profiles across ranks (cstone_hip_domain_mr_sphere_profiles, NativeDistributedDomain.sphere_profiles): on 1, 2
and 3 ranks every rank's rows against the brute force over the whole cloud (tests/sphere_mr_worker.py, on the clouds of
tests/fof_mr_support.py), and the refusals.

Sixty-four seeded centres, identical on all ranks.  Counts and flags on every rank == the brute force; sums within the
bound of an arbitrary order of addition (tests/sphere_support.py), which covers the collective's order too; every rank
holds the same bits; on one rank the bits are those of cstone_hip_sphere_profiles on the same arrays.  A call before the
first sync, bad edges, a num_queries that differs on one rank and a null x on one rank are refused on EVERY rank, write
nothing and leave the domain usable: after each of them the worker's ranks gather their return codes, so a rank left
waiting in a collective shows as a missing result, not as this test's timeout."""
import json
import os
import re
import subprocess
import sys

import pytest

import fof_mr_support as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_INTERNAL = -1, -4


def test_header_declares_and_the_bindings_export_the_call():
    import cstone_amd
    from cstone_amd.distributed import NativeDistributedDomain

    text = open(os.path.join(ROOT, "include", "cstone_hip.h")).read()
    assert re.search(r"\bint cstone_hip_domain_mr_sphere_profiles\(", text)
    assert "cstone_hip_domain_mr_sphere_profiles" in cstone_amd.EXPORTS
    assert hasattr(cstone_amd.load_library(), "cstone_hip_domain_mr_sphere_profiles")
    assert callable(NativeDistributedDomain.sphere_profiles)


def _launch(nproc, port, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "sphere_mr_worker.py")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("SPHERE_MR_RESULT ")]
    assert lines, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(lines[-1][len("SPHERE_MR_RESULT "):])
    print(json.dumps(res))
    assert p.returncode == 0 and res["ok"], str(res["bad"])[:3000] + p.stderr[-2000:]
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [1, 2, 3])
def test_hip_sphere_profiles_across_ranks(nproc):
    """the comparison and the refusals of the module's docstring on nproc gloo ranks that share the GPU, every cloud of
    fof_mr_support.CLOUDS, 32- and 64-bit weights in turn"""
    res = _launch(nproc, 29980 + nproc)
    assert res["ranks"] == nproc and set(res["clouds"]) == set(ms.CLOUDS)
    for name, figs in res["clouds"].items():
        periodic = any(ms.CLOUDS[name][1])
        assert figs["binned"] > 1000 and figs["wide"] == (1 if periodic else 0)
        st = figs["statuses"]
        assert set(st) == {"no sync", "edges descending", "edges negative", "edges nan", "edges too many", "null x"} | (
            {"Q differs"} if nproc > 1 else set())
        for what, codes in st.items():
            want = [E_ARG] * nproc
            if what == "null x":
                want = [E_INTERNAL] * (nproc - 1) + [E_ARG]
            assert codes == want, (name, what, codes)
