"""The connectivity pass through the cv::Mat drop-in (include/img_completion.h): tests/mock_opencv/shim_connectivity_test.cpp compiles
on a CPU against the cv::Mat stand-in; on the GPU the compiled C++ caller compares dcmt_shim::slic_enforce_connectivity ([col][row],
in place) with the C ABI itself, and what it writes is compared with the Python surface and the restatement."""
import os
import subprocess

import numpy as np
import pytest

import connectivity_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_connectivity_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_connectivity_test.o")],
                   check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_python_surface(tmp_path):
    rows, cols, nc = 70, 130, 180
    plane = R.odd_values(rows, cols, 9)
    plane.tofile(tmp_path / "in.i32")
    exe = tmp_path / "shim_connectivity_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([str(exe), str(rows), str(cols), str(nc), str(tmp_path / "in.i32"), str(tmp_path / "out.i32")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    got = np.fromfile(tmp_path / "out.i32", dtype=np.int32).reshape(rows, cols)
    want, count = R.components(plane, nc)
    assert int(r.stdout.split()[-1]) == count and np.array_equal(got, want)
    out, n = api.slic_enforce_connectivity(plane, nc)
    assert n == count and np.array_equal(out, got)
