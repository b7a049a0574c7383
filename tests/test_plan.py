"""The dispatch as values, checked without a GPU: the cascade's (csrc/dcmt_plan.h: knobs + call -> plan, cases in
tests/plan_test.cpp) and that of the entry points beside it (csrc/dcmt_plan_side.h: segments, scratch layouts, grids, the winner
plane's state; cases in tests/plan_side_test.cpp).  g++ builds each against the headers alone -- which also shows that the
headers need no HIP."""
import os
import subprocess

from conftest import ROOT


def _build_and_run(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "depth_completion_mt_amd", "csrc"),
                    os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_plan_of_every_dispatch_case(tmp_path):
    _build_and_run(tmp_path, "plan_test")


def test_side_plans(tmp_path):
    _build_and_run(tmp_path, "plan_side_test")
