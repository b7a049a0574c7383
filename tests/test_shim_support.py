"""The support map and the trust mask through the cv::Mat drop-in (include/img_completion.h): tests/mock_opencv/shim_support_test.cpp
compiles on a CPU against the cv::Mat stand-in; on the GPU the compiled C++ caller compares dcmt_shim::distance_to_returns and
dcmt_shim::trust_mask (cv::Mat in, a fresh cv::Mat out) with the C ABI itself, and what it writes is compared with the Python surface
and the literal restatement."""
import os
import subprocess

import numpy as np
import pytest

import support_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_support_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_support_test.o")],
                   check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_python_surface(tmp_path):
    rows, cols = 70, 130
    sparse = R.sparse_plane(rows, cols, 0.01, 9)
    dense, fallback = R.dense_planes(rows, cols, 10)
    for name, a in (("sparse", sparse), ("dense", dense), ("fallback", fallback)):
        a.tofile(tmp_path / f"{name}.f32")
    exe = tmp_path / "shim_support_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([str(exe), str(rows), str(cols)] + [str(tmp_path / f"{n}.f32") for n in ("sparse", "dense", "fallback", "dist2", "trusted")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    dist2 = np.fromfile(tmp_path / "dist2.f32", dtype=np.float32).reshape(rows, cols)
    trusted = np.fromfile(tmp_path / "trusted.f32", dtype=np.float32).reshape(rows, cols)
    want, n = R.literal_dist2(sparse)
    assert 0 < n < rows * cols and np.array_equal(dist2, want.astype(np.float32))
    assert np.array_equal(api.distance_to_returns(sparse), want)
    near = R.literal_dist2(sparse, max_radius=3)[0]
    assert np.array_equal(trusted.view(np.uint32), R.select(near, dense, fallback).view(np.uint32))
    assert np.array_equal(api.trust_mask(sparse, dense, fallback, max_radius=3).view(np.uint32), trusted.view(np.uint32))
