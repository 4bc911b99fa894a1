"""Friends-of-friends groups across ranks (cstone_hip_domain_mr_fof, NativeDistributedDomain.fof, the C++ methods): global
labels, group sizes, the number of groups and of rounds on 1 to 4 ranks against the brute force over the whole cloud and
the numpy restatement of the rounds (tests/fof_mr_support.py, tests/fof_mr_worker.py), the refusals, and the C++ example.

Observed on an MI355X (gloo ranks sharing the GPU; the restatement gives the same numbers): the uniform clouds take 2
rounds on one rank and 3-4 on 2 to 4, the serpentine 2, 18, 34 and 18 rounds on 1, 2, 3 and 4 ranks (at least 8 are
required on 2 or more).  Every launch prints its figures in one result line."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fof_mr_support as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_the_bindings_export_the_two_calls():
    import cstone_amd

    text = open(os.path.join(ROOT, "include", "cstone_hip.h")).read()
    for name in ("cstone_hip_fof_lower_labels", "cstone_hip_domain_mr_fof"):
        assert re.search(rf"\bint {name}\(", text) and name in cstone_amd.EXPORTS
        assert hasattr(cstone_amd.load_library(), name)
    assert "joining groups across ranks is not provided" not in text
    assert int(re.search(r"#define CSTONE_FOF_MR_DEFAULT_ROUNDS (\d+)u", text).group(1)) == cstone_amd.FOF_MR_DEFAULT_ROUNDS


def test_the_serpentine_is_one_chain():
    from helpers import Box

    (x, y, z), b, bc = ms.cloud("serpentine")
    assert 3600 <= x.size <= 3800 and b == 0.01
    steps = np.sqrt(np.diff(x) ** 2 + np.diff(y) ** 2)
    assert steps.max() <= 0.8 * b * (1 + 1e-12) and steps.min() > 0.5 * b
    labels, sizes, ng = ms.groups_of(x, y, z, b, Box([0, 1] * 3, bc))
    assert ng == 1 and sizes.min() == x.size
    # the only links are those along the chain: two per particle, one at the ends
    from fof_support import links, stub_case

    degree = links(stub_case(x, y, z, b, Box([0, 1] * 3, bc)), 0, x.size).sum(1)
    assert degree[0] == degree[-1] == 1 and (degree[1:-1] == 2).all()


def test_restated_rounds_on_hand_made_ranks():
    """the numpy restatement itself, on a chain of 9 particles cut into three ranks that hold one halo on either side:
    the lowest id walks one rank per round"""
    from helpers import Box

    b = 0.1
    x = 0.1 + 0.08 * np.arange(9)
    y = z = np.full(9, 0.5)
    box = Box([0, 1] * 3)
    parts = []
    for a, e in ((0, 3), (3, 6), (6, 9)):
        lo, hi = max(a - 1, 0), min(e + 1, 9)
        parts.append(ms.RankPart(x[lo:hi], y[lo:hi], z[lo:hi], np.arange(lo, hi), a - lo, e - lo))
    labels, rounds = ms.model_rounds(parts, b, box)
    assert all((lab == 0).all() for lab in labels) and rounds == 4
    one, rounds1 = ms.model_rounds([ms.RankPart(x, y, z, np.arange(9), 0, 9)], b, box)
    assert (one[0] == 0).all() and rounds1 == 2


def _launch(nproc, port, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "fof_mr_worker.py")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("FOF_MR_RESULT ")]
    assert lines, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(lines[-1][len("FOF_MR_RESULT "):])
    print(json.dumps(res))
    assert p.returncode == 0 and res["ok"], str(res["bad"])[:3000] + p.stderr[-2000:]
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("nproc", [1, 2, 3, 4])
def test_hip_fof_across_ranks(nproc):
    """every cloud of fof_mr_support.CLOUDS on nproc gloo ranks that share the GPU (tests/fof_mr_worker.py): labels of
    assigned particles == the lowest global id of the group by the brute force over the WHOLE cloud, halo entries == their
    owners' values, sizes and the number of groups likewise, rounds == the restated rounds, two calls identical; the
    same for the first cloud with owner-side halo discovery; the
    refusals (before a sync, b of half a periodic edge, NaN, halos that do not reach b, max_rounds = 1 on the serpentine)
    come on every rank, write nothing and leave the domain usable; one rank == the single-rank call, in 2 rounds"""
    res = _launch(nproc, 29960 + nproc)
    assert res["ranks"] == nproc and set(res["clouds"]) == set(ms.CLOUDS) | {"uniform-open, owner-side halos"}
    for name, figs in res["clouds"].items():
        assert figs["rounds"] == figs["model_rounds"]
        assert all(h > 0 for h in figs["halos"]) == (nproc > 1)
    assert res["clouds"]["serpentine"]["groups"] == 1
    assert res["clouds"]["uniform-pbc"]["groups"] > 100
    if nproc == 1:
        assert all(figs["rounds"] == 2 for figs in res["clouds"].values())
    else:
        assert res["clouds"]["serpentine"]["rounds"] >= 8


def _compile_example(exe):
    libdir = os.path.join(ROOT, "cornerstone-octree_amd", "lib")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Wno-comment", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "cornerstone-octree_amd", "include"),
                    os.path.join(ROOT, "examples", "fof_mr_example.cpp"), "-L", libdir, "-lcstone_hip",
                    f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)


def test_cpp_example_compiles_with_a_host_compiler(tmp_path):
    """examples/fof_mr_example.cpp (Domain::friendsOfFriendsGlobal and through it MultiRankDomain::friendsOfFriends)
    against the C++ host layer, with g++"""
    _compile_example(tmp_path / "fof_mr_example")


@pytest.mark.gpu
def test_hip_cpp_example_runs(tmp_path):
    """a multi-rank Domain on a communicator of one rank: global labels and sizes == Domain::friendsOfFriends, 2 rounds"""
    exe = tmp_path / "fof_mr_example"
    _compile_example(exe)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    m = re.search(r"groups (\d+), largest (\d+), rounds (\d+)", p.stdout)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) > 1 and int(m.group(3)) == 2
    assert "identical" in p.stdout
