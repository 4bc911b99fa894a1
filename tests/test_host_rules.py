"""The host-side rules of the Domain orchestration that need no HIP (cornerstone-octree_amd/csrc/host_rules.hpp) as a
stand-alone program against the oracle (oracle/host_rules_check.cpp): the update step of the global tree that every
steady-state sync makes on the host must decide and rebalance like the oracle's update_octree, step by step from the
root to convergence and on through a drift, a removal and a collapse, for 32- and 64-bit keys and buckets of 16 and 64,
and must have taken every decision (merge, keep, split by 8, 64, 512, 4096) on the way; the exchange plan and the
margins of the result arrays of the multi-rank sync give the answers worked out by hand, and so does the start pass of
the partial-digit sort, which also keeps its defining inequality at every level.  Run as a plain build and as a
build of its own with -fsanitize=address,undefined."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    p = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "rules"], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]


@pytest.mark.parametrize("exe", ["host_rules_check", "host_rules_check_asan"])
def test_global_tree_step_on_the_host_equals_the_oracle(built, exe):
    p = subprocess.run([os.path.join(ROOT, "oracle", exe)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS="2"))
    out = p.stdout + p.stderr
    assert p.returncode == 0 and "HOST_RULES OK" in out, out[-3000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    runs = re.findall(r"HOST_RULES k(\d+) bucket (\d+): (\d+) steps, merge (\d+) keep (\d+) split8 (\d+) split64 (\d+) "
                      r"split512 (\d+) split4096 (\d+)", out)
    assert sorted((int(r[0]), int(r[1])) for r in runs) == [(32, 16), (32, 64), (64, 16), (64, 64)]
    for r in runs:
        assert all(int(c) > 0 for c in r[3:]), r
    # exchangePlan and resultMargins / blockWithHalos of the multi-rank sync: every known answer was checked
    assert re.search(r"HOST_RULES exchangePlan and resultMargins: 19 known answers", out), out[-3000:]
    # partialSortStartPass: the nine values worked out by hand, and three properties (even and in range, the skipped
    # digits lie below the deepest leaf level + margin, two more would not) for every level of both key types at six
    # bucket sizes: 6 x (11 + 22) x 3
    assert re.search(r"HOST_RULES partialSortStartPass: 9 hand values, 594 property checks", out), out[-3000:]
