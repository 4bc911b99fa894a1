"""Pair counts across ranks (cstone_hip_domain_mr_pair_counts, cstone_hip_domain_mr_pair_counts_cross;
NativeDistributedDomain.pair_counts, pair_counts_cross): on 1, 2 and 3 ranks every rank's counts against the brute force
over the whole cloud (tests/pair_counts_mr_worker.py), and the refusals.

Clouds of 6 000 particles, uniform in a periodic box (float64) and in blobs in an open one (float32); every particle has
the smoothing length 0.03, so the halos reach exactly the outer edge float32(0.06) of the 8 bins; weights 0.5 + x; 500 seeded
query centres with weights, identical on all ranks, a few of them outside the box.  Auto and cross counts on every rank ==
the restatement (tests/pair_counts_support.py) over the GLOBAL cloud, sums within the bound derived there, every rank holds
the same bits, and the pairs the ranks say they binned add up to the total.  The launcher computes the brute force once
more over the cloud AS GENERATED, in no rank's order: the counts of every number of ranks must equal it, hence each other.

A call before the first sync and bad edges are refused on every rank before any collective; an NB that differs on one
rank, a w on all ranks but one, a null x on one rank and -- auto counts only -- an outer edge one float32 ulp above the kept
halo radius are refused on EVERY rank together, write nothing and leave the domain usable: after each of them the worker's
ranks gather their return codes, so a rank left waiting in a collective shows as a missing result, not as this test's
timeout.  On one rank the outer edge above the halo radius is taken (every particle is on the rank), and the cross counts
take it on any number of ranks: they need no reach.

Not covered: a rank WITHOUT assigned particles.  The multi-rank sync refuses a decomposition that leaves a rank without
particles, so no domain can be brought into that state; the calls treat such a rank like
cstone_hip_domain_mr_sphere_profiles does (an empty range, null arrays allowed, it goes along in both collectives)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_INTERNAL = -1, -4

_expected = {}


def expected_counts(name):
    """(auto, cross) counts of the brute force over the cloud as generated; the box is the unit box (an open box is never
    folded, whatever limits the domain fits)"""
    import pair_counts_mr_worker as w
    import pair_counts_support as ps

    if name not in _expected:
        coords, bc = w.make_cloud(name)
        T = coords[0].dtype.type
        edges = w.make_edges(T)
        qc, _ = w.make_queries(T)
        auto = ps.auto_reference(coords, None, 0, w.N, 0, w.N, [0, 1] * 3, bc, edges)
        cross = ps.cross_reference(coords, None, 0, w.N, qc, None, [0, 1] * 3, bc, edges)
        _expected[name] = (auto.counts.tolist(), cross.counts.tolist())
    return _expected[name]


def test_cover_rule_edge_is_the_kept_halo_radius():
    """the outer edge of the worker's bins is float32(2 H) in both coordinate types, its edges ascend strictly, and the
    brute force over the clouds as generated fills the first and the last bin"""
    import pair_counts_mr_worker as w

    for T in (np.float32, np.float64):
        e = w.make_edges(T)
        assert len(e) == w.NB + 1 and e[0] == 0.0 and all(a < b for a, b in zip(e[:-1], e[1:]))
        assert e[-1] == float(np.float32(e[-1])) and abs(e[-1] - 2 * w.H) <= 2 * w.H * 2.0 ** -23
    for name in w.CLOUDS:
        auto, cross = expected_counts(name)
        assert auto[0] > 0 and auto[-1] > 0 and cross[0] > 0 and cross[-1] > 0 and all(c % 2 == 0 for c in auto)


def _launch(nproc, port, names=(), timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "pair_counts_mr_worker.py")] + list(names)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("PAIR_MR_RESULT ")]
    assert lines, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(lines[-1][len("PAIR_MR_RESULT "):])
    print(json.dumps(res))
    assert p.returncode == 0 and res["ok"], str(res["bad"])[:3000] + p.stderr[-2000:]
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [1, 2, 3])
def test_hip_pair_counts_across_ranks(nproc):
    """the comparisons and the refusals of the module's docstring on nproc gloo ranks that share the GPU"""
    import pair_counts_mr_worker as w

    res = _launch(nproc, 29970 + nproc)
    assert res["ranks"] == nproc and set(res["clouds"]) == set(w.CLOUDS)
    for name, figs in res["clouds"].items():
        assert len(figs["assigned"]) == nproc and min(figs["assigned"]) > 0 and sum(figs["assigned"]) == w.N
        assert (figs["halos"] > 0) == (nproc > 1)
        auto, cross = expected_counts(name)
        assert figs["auto"] == auto and figs["cross"] == cross, name  # the same for every number of ranks
        st = figs["statuses"]
        both = lambda keys: {k + tail for k in keys for tail in ("", ", cross")}  # noqa: E731
        want_keys = both({"no sync", "bad edges", "no bins", "null x"}) | {"cover"}
        if nproc > 1:
            want_keys |= both({"NB differs", "w differs"})
        assert set(st) == want_keys
        for what, codes in st.items():
            want = [E_ARG] * nproc
            if what.startswith("null x"):
                want = [E_INTERNAL] * (nproc - 1) + [E_ARG]
            if what == "cover" and nproc == 1:
                want = [0]
            assert codes == want, (name, what, codes)
