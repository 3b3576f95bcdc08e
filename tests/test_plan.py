"""The traversal planner on the host (csrc/pu_plan.h): tests/plan_check.cpp, a
stand-alone program that links the planner's object alone, is built and run.  It checks the
structure of whole plans (sources, chunks, tasks, slot lifetimes, pad, build, variant) with an
LDS stub of its own, so no device and no kernel byte count is involved."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "phylo_utils_amd", "csrc")


def test_plan_check(tmp_path):
    obj = str(tmp_path / "obj")
    build = subprocess.run(["make", "-C", CSRC, "OBJ=" + obj, "plan_check"],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([os.path.join(obj, "plan_check")], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout
