"""The cascade's dispatch as a value (csrc/dcmt_plan.h: knobs + call -> plan), checked without a GPU: tests/plan_test.cpp holds
the cases, g++ builds it against the header alone -- which also shows that the header needs no HIP."""
import os
import subprocess

from conftest import ROOT


def test_plan_of_every_dispatch_case(tmp_path):
    exe = str(tmp_path / "plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "depth_completion_mt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "plan_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
