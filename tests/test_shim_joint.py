"""The joint bilateral filter through the cv::Mat drop-in (include/img_completion.h): tests/mock_opencv/shim_joint_test.cpp compiles on
a CPU against the cv::Mat stand-in; on the GPU the compiled C++ caller compares dcmt_shim::joint_bilateral_fill (cv::Mat in, a fresh
cv::Mat out) with the C ABI itself, and what it writes is compared with the Python surface and the restatements."""
import os
import subprocess

import numpy as np
import pytest

import joint_restatement as J
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_joint_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_joint_test.o")],
                   check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_python_surface(tmp_path):
    rows, cols = 70, 130
    depth, grey, bgr = J.holed_plane(rows, cols, 9), J.guide_plane(rows, cols, 1, 9), J.guide_plane(rows, cols, 3, 9)
    for name, a in (("depth.f32", depth), ("grey.u8", grey), ("bgr.u8", bgr)):
        a.tofile(tmp_path / name)
    exe = tmp_path / "shim_joint_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([str(exe), str(rows), str(cols)] + [str(tmp_path / n) for n in ("depth.f32", "grey.u8", "bgr.u8", "filled_grey.f32", "filled_bgr.f32")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    a = np.fromfile(tmp_path / "filled_grey.f32", dtype=np.float32).reshape(rows, cols)
    b = np.fromfile(tmp_path / "filled_bgr.f32", dtype=np.float32).reshape(rows, cols)
    dflt = J.as_record(*J.tables(**J.SIGMAS))
    for form in (J.literal, J.tap_major):
        want, filled, left = form(depth, grey, dflt)
        assert filled > 0 and a.tobytes() == want.tobytes()
        want, filled, left = form(depth, bgr, J.tables(3, 1.5, 25.0), radius=3, smooth=True)
        assert filled > 0 and b.tobytes() == want.tobytes()
    assert api.joint_bilateral_fill(depth, grey).tobytes() == a.tobytes()
    assert api.joint_bilateral_fill(depth, bgr, api.make_joint_tables(3, 1.5, 25.0), radius=3, smooth=True).tobytes() == b.tobytes()
