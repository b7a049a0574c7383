"""Undistortion and rectification through the cv::Mat drop-in (include/img_completion.h, dcmt_shim::undistort_rectify):
tests/mock_opencv/shim_rectify_test.cpp compiles on a CPU against the cv::Mat stand-in; on the GPU the compiled C++ caller compares
the shim with the C ABI itself, and what it writes is compared with the restatement (tests/rectify_restatement.py)."""
import os
import subprocess

import numpy as np
import pytest

import rectify_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_rectify_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_rectify_test.o")],
                   check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_restatement(tmp_path):
    src_shape, rows, cols = (70, 170), 50, 140
    K = np.array([[150.0, 0.0, 84.2], [0.0, 149.0, 33.4], [0.0, 0.0, 1.0]])
    P = np.array([[130.0, 0.0, 70.0], [0.0, 130.0, 25.0], [0.0, 0.0, 1.0]])
    rec = R.roll_record(3.0, K, P)
    rec["k1"], rec["p1"] = -0.25, 1e-3
    rec.tofile(tmp_path / "calib.f64")
    exe = tmp_path / "shim_rectify_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    m = R.rectify_map(rec, rows, cols)
    for ch in (1, 3):
        src = R.noise(src_shape + ((3,) if ch == 3 else ()), 80 + ch)
        src.tofile(tmp_path / "in.u8")
        r = subprocess.run([str(exe), str(src_shape[0]), str(src_shape[1]), str(ch), str(rows), str(cols), str(tmp_path / "in.u8"),
                            str(tmp_path / "calib.f64"), str(tmp_path / "out.u8")], capture_output=True, text=True)
        assert r.returncode == 0, (ch, r.returncode, r.stdout, r.stderr)
        want = R.remap(src, m)
        got = np.fromfile(tmp_path / "out.u8", dtype=np.uint8).reshape(want.shape)
        assert np.array_equal(got, want) and want.any()
