"""The step plan of the leaf pass (csrc/leaf_steps.hpp: which leaves of a wave's quarter share a wave step) on the CPU:
tests/leaf_steps_check.cpp compares it with the rule walked leaf by leaf for every sequence of 1-6 leaf sizes from
{0, 1, 32, 33, 64, 65, 128, 129, 255} in quarters of up to 16 leaves.  A stand-alone program, built with g++ and run
directly -- once plain, once with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cornerstone-octree_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "leaf_steps_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_leaf_step_plan_equals_the_rule_walked_leaf_by_leaf(tmp_path, flags):
    exe = str(tmp_path / "leaf_steps_check")
    subprocess.run(["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, SOURCE, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "leaf steps ok" in run.stdout, run.stdout[-2000:]
