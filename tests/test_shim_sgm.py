"""The stereo matcher through the cv::Mat drop-in (include/img_completion.h): tests/mock_opencv/shim_sgm_test.cpp compiles on a CPU
against the cv::Mat stand-in; on the GPU the compiled C++ caller compares dcmt_shim::stereo_sgm (a left image with padded rows) with
the C ABI itself, and what it writes is compared with the Python surface and the restatement.  With the stand-in the other shim
tests use, which has no CV_16SC1, the header must still compile, without the function."""
import os
import subprocess

import numpy as np
import pytest

import sgm_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_sgm_test.cpp")
# the stand-in with CV_16SC1 (tests/mock_opencv/with_16s), a file of its own: the one the other shim tests use has no 16-bit elements
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv", "with_16s")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_sgm_test.o")],
                   check=True, capture_output=True)


def test_header_compiles_against_a_stand_in_without_16_bit_elements(tmp_path):
    src = tmp_path / "plain.cpp"
    src.write_text('#include "img_completion.h"\n#ifdef CV_16SC1\n#error "this stand-in was expected to have no CV_16SC1"\n#endif\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv"),
                    "-c", str(src), "-o", str(tmp_path / "plain.o")], check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_python_surface(tmp_path):
    rows, cols, D = 21, 131, 32
    left, right = R.shifted_pair(rows, cols, 14)
    left.tofile(tmp_path / "left.u8")
    right.tofile(tmp_path / "right.u8")
    exe = tmp_path / "shim_sgm_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([str(exe), str(rows), str(cols), str(D)] + [str(tmp_path / f) for f in ("left.u8", "right.u8", "disp16.i16")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    d16 = np.fromfile(tmp_path / "disp16.i16", dtype=np.int16).reshape(rows, cols)
    want16 = R.vectorised(left, right, num_disparities=D)[0]
    assert np.array_equal(d16, want16) and (d16 > 0).mean() > 0.5
    assert np.array_equal(api.stereo_sgm(left, right, num_disparities=D), d16)
