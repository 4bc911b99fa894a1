"""k nearest neighbours across ranks (cstone_hip_domain_mr_knn, NativeDistributedDomain.knn): on 1, 2 and 3 ranks every
rank's rows against the brute force over the whole cloud in global SFC order (tests/knn_mr_worker.py), and the refusals.

Clouds of 6 000 particles, uniform and in blobs, open and periodic, and one of 150 particles where k = 100 exceeds a rank's
share and k = 256 the cloud; 40 seeded centres, identical on all ranks, five of them far away; k = 8 and 100, with and
without radius limits.  ids, dist2 and counts on every rank == the restatement (tests/knn_support.py); every rank holds the
same bits; on one rank the output is that of cstone_hip_knn with indices turned into ids.  Every correct call is repeated
with the cap on the gather's receive buffer set to 16 KiB through the documented environment override: the same bits, the
number of all_gather rounds the chunk rule gives, and a receive buffer under the cap.  A call before the first sync and a
k out of range are refused on every rank before any collective; a k, a num_queries or a presence of query_rmax that
differs on one rank, and a null x on one rank, are refused on EVERY rank together, write nothing and leave the domain
usable: after each of them the worker's ranks gather their return codes, so a rank left waiting in a collective shows as
a missing result, not as this test's timeout.

Not covered: a rank WITHOUT assigned particles.  The multi-rank sync refuses a decomposition that leaves a rank without
particles ("rank 1 is left without particles": ten particles on three ranks), so no domain can be brought into that
state; the call treats such a rank like cstone_hip_domain_mr_sphere_profiles does (an empty range, null arrays allowed)."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_INTERNAL = -1, -4
NEW_SYMBOLS = ("cstone_hip_domain_mr_knn", "cstone_hip_knn_mr_chunk_queries", "cstone_hip_domain_mr_knn_last")


def test_header_declares_and_the_bindings_export_the_calls_and_the_cap():
    import cstone_amd
    from cstone_amd.distributed import NativeDistributedDomain

    text = open(os.path.join(ROOT, "include", "cstone_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = cstone_amd.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", code) and name in cstone_amd.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define CSTONE_KNN_MR_GATHER_BYTES \(256ull << 20\)", code) and cstone_amd.KNN_MR_GATHER_BYTES == 256 << 20
    assert callable(NativeDistributedDomain.knn) and callable(NativeDistributedDomain.knn_last)


def test_chunk_rule_keeps_the_receive_buffer_under_the_cap():
    """queries per all_gather = floor(cap / (16 k P)), at least 1, at most Q: P * chunk * k * 16 bytes never exceed the cap
    unless a single query's records do"""
    import cstone_amd

    rule = cstone_amd.load_library().cstone_hip_knn_mr_chunk_queries
    cap = cstone_amd.KNN_MR_GATHER_BYTES
    assert rule(0, 8, 2, cap) == 0 and rule(40, 8, 3, cap) == 40 and rule(40, 100, 3, 16384) == 3 and rule(40, 8, 3, 16384) == 40
    assert rule(40, 256, 3, 4096) == 1 and rule(40, 256, 1, 4096) == 1 and rule(40, 1, 1, 16) == 1 and rule(40, 1, 1, 47) == 2
    assert rule(10 ** 8, 256, 8, cap) == cap // (16 * 256 * 8) == 8192
    for Q, k, P, c in ((10 ** 6, 64, 4, cap), (1000, 256, 64, 1 << 20), (77, 33, 5, 12345), (2 ** 32 - 1, 1, 1, 2 ** 40)):
        per = rule(Q, k, P, c)
        assert 1 <= per <= Q and (per * 16 * k * P <= c or per == 1) and (per == Q or (per + 1) * 16 * k * P > c)


def _launch(nproc, port, names=(), timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    env.pop("CSTONE_KNN_MR_GATHER_BYTES", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "knn_mr_worker.py")] + list(names)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("KNN_MR_RESULT ")]
    assert lines, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(lines[-1][len("KNN_MR_RESULT "):])
    print(json.dumps(res))
    assert p.returncode == 0 and res["ok"], str(res["bad"])[:3000] + p.stderr[-2000:]
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [1, 2, 3])
def test_hip_knn_across_ranks(nproc):
    """the comparison, the chunked gather and the refusals of the module's docstring on nproc gloo ranks that share the GPU"""
    import knn_mr_worker as w

    res = _launch(nproc, 29960 + nproc)
    assert res["ranks"] == nproc and set(res["clouds"]) == set(w.CLOUDS)
    for name, figs in res["clouds"].items():
        assert len(figs["assigned"]) == nproc and min(figs["assigned"]) > 0
        if name.startswith("sparse"):
            assert sum(figs["assigned"]) == 150 and (nproc == 1 or max(figs["assigned"]) < 100)  # k = 100 exceeds every share
        st = figs["statuses"]
        assert set(st) == {"no sync", "k 0", "k 257", "null x"} | ({"k differs", "Q differs", "rmax differs"} if nproc > 1 else set())
        for what, codes in st.items():
            want = [E_ARG] * nproc
            if what == "null x":
                want = [E_INTERNAL] * (nproc - 1) + [E_ARG]
            assert codes == want, (name, what, codes)
        # the cap really applied: more than one all_gather round with k = 100, the receive buffer under the 16 KiB
        chunks, nbytes = figs["chunking"]["100 free"]
        assert chunks == -(-w.Q // max(1, w.SMALL_CAP // (1600 * nproc))) > 1 and nbytes <= w.SMALL_CAP
        assert (nbytes > 0) == (nproc > 1)

