"""A re-sorted Domain::sync makes the structural half of its focus-tree update (node ops, rebalance, linked octree) on a
third stream beside the mover bins and the leaf pass (DESIGN.md sections 2b, 9b).  CSTONE_NO_TREE_HOIST=1 restores the
order on one stream.  Either way, and combined with the other scheduling switches, a client sees the same bytes: one
process per setting runs tests/tree_hoist_worker.py, all settings at once (each opens the GPU once).  The number of
re-sorted syncs stands beside the digest, not in it: it is the same for every setting but CSTONE_NO_RESORT, whose
point is that it is zero there."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "tree_hoist_worker.py")

SETTINGS = [
    {},
    {"CSTONE_NO_TREE_HOIST": "1"},
    {"CSTONE_NO_GATHER_OVERLAP": "1"},
    {"CSTONE_NO_TREE_HOIST": "1", "CSTONE_NO_GATHER_OVERLAP": "1"},
    {"CSTONE_NO_RESORT": "1"},
    {"CSTONE_DEVICE_GLOBAL_STEP": "1"},
]
# particles : bucketFocus -- a deep tree with many leaves per tile, and a size at which the two chains of a sync really
# are in flight together
SIZES = ["2e5:64", "2e5:8", "2e6:64"]


def _run_all(args):
    procs = []
    for env_extra in SETTINGS:
        env = dict(os.environ, **env_extra)
        for k in ("CSTONE_NO_TREE_HOIST", "CSTONE_NO_GATHER_OVERLAP", "CSTONE_NO_RESORT", "CSTONE_DEVICE_GLOBAL_STEP"):
            if k not in env_extra:
                env.pop(k, None)
        procs.append(subprocess.Popen([sys.executable, WORKER] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True, cwd=ROOT, env=env))
    out = {}
    for env_extra, p in zip(SETTINGS, procs):
        stdout, stderr = p.communicate(timeout=600)
        assert p.returncode == 0, (env_extra, stderr[-3000:])
        out[tuple(sorted(env_extra.items()))] = stdout
    return out


@pytest.mark.gpu
def test_tree_hoist_changes_nothing_a_client_can_see():
    out = _run_all(SIZES)
    line = re.compile(r"DIGEST ([0-9a-f]{64}) n (\d+) bucket (\d+) resorts (\d+) rebuilt (\d+) kept (\d+) fallbacks (\d+) "
                      r"box_redos (\d+)")
    seen = {}
    for setting, stdout in out.items():
        rows = [m.groups() for m in line.finditer(stdout)]
        assert len(rows) == len(SIZES), (setting, stdout[-2000:])
        print(setting, rows)
        seen[setting] = rows
    no_resort = (("CSTONE_NO_RESORT", "1"),)
    for i, size in enumerate(SIZES):
        digests = {rows[i][0] for rows in seen.values()}
        assert len(digests) == 1, (size, {k: v[i] for k, v in seen.items()})
        resorts, rebuilt, kept, fallbacks, box_redos = (int(v) for v in seen[()][i][3:])
        # the default re-sorted (before and after its back-off), fell back inside a sync and redid a box; its tree was
        # rebuilt in some syncs and kept in others
        assert resorts >= 6 and fallbacks >= 1 and box_redos >= 1, (size, seen[()][i])
        assert rebuilt >= 1 and kept >= 1, (size, seen[()][i])
        assert int(seen[no_resort][i][3]) == 0, (size, seen[no_resort][i])
        for setting, rows in seen.items():
            if setting != no_resort:
                assert rows[i][3:] == seen[()][i][3:], (size, setting, rows[i])


@pytest.mark.gpu
def test_all_particles_removed_is_the_same_error_with_and_without_the_hoist():
    out = _run_all(["allremoved"])
    codes = {}
    for setting, stdout in out.items():
        m = re.search(r"ERROR (-?\d+|none) resorts (\d+)", stdout)
        assert m, (setting, stdout[-2000:])
        codes[setting] = m.group(1)
        assert "RECOVERED particles 100000 sorted True" in stdout, (setting, stdout[-2000:])
    print(codes)
    assert codes[()] != "none" and int(codes[()]) != 0
    assert len(set(codes.values())) == 1, codes
