"""The occlusion filter through the cv::Mat drop-in (include/img_completion.h): tests/mock_opencv/shim_occlusion_test.cpp compiles on a
CPU against the cv::Mat stand-in; on the GPU the compiled C++ caller compares dcmt_shim::filter_occluded_returns (cv::Mat in, a fresh
cv::Mat out) with the C ABI itself, and what it writes is compared with the Python surface and the literal restatement."""
import os
import subprocess

import numpy as np
import pytest

import occlusion_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_occlusion_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_occlusion_test.o")],
                   check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_python_surface(tmp_path):
    rows, cols = 70, 130
    depth = R.sparse_plane(rows, cols, 0.3, 9)
    depth.tofile(tmp_path / "depth.f32")
    exe = tmp_path / "shim_occlusion_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([str(exe), str(rows), str(cols), str(tmp_path / "depth.f32"), str(tmp_path / "filtered.f32")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    filtered = np.fromfile(tmp_path / "filtered.f32", dtype=np.float32).reshape(rows, cols)
    want, n = R.literal_occlusion(depth)
    assert n > 0 and np.array_equal(filtered.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(api.filter_occluded_returns(depth).view(np.uint32), filtered.view(np.uint32))
