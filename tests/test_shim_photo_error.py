"""get_initial_error through the cv::Mat drop-in (include/img_completion.h): tests/mock_opencv/shim_photo_error_test.cpp compiles on a
CPU against the cv::Mat stand-in; on the GPU the compiled C++ caller compares dcmt_shim::get_initial_error (a packed depth, a left
image with padded rows) with the C ABI itself, and what it writes is compared with the Python surface and the restatement."""
import os
import subprocess

import numpy as np
import pytest

import photo_error_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_photo_error_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_photo_error_test.o")],
                   check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_python_surface(tmp_path):
    rows, cols, window = 37, 131, 3
    depth = R.adversarial_depth(rows, cols, 12)[0]
    left, right = R.random_pair(rows, cols, 13)
    depth.tofile(tmp_path / "depth.f32")
    left.tofile(tmp_path / "left.u8")
    right.tofile(tmp_path / "right.u8")
    exe = tmp_path / "shim_photo_error_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([str(exe), str(rows), str(cols), str(window)] + [str(tmp_path / f) for f in ("depth.f32", "left.u8", "right.u8", "err.u8", "stats.u64")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    err = np.fromfile(tmp_path / "err.u8", dtype=np.uint8).reshape(rows, cols)
    stats = np.fromfile(tmp_path / "stats.u64", dtype=np.uint64)
    want_err, want_stats = R.vectorised(depth, left, right, window=window)
    assert np.array_equal(err, want_err) and np.array_equal(stats, want_stats) and int(stats[0]) > 0
    got_err, got_stats = api.get_initial_error(depth, left, right, window=window)
    assert np.array_equal(got_err, err) and [got_stats[k] for k in api.PHOTO_STATS] == [int(v) for v in stats]
