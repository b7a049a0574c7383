"""The bilateral finish through the cv::Mat drop-in (include/img_completion.h): tests/mock_opencv/shim_bilateral_test.cpp compiles on a
CPU against the cv::Mat stand-in; on the GPU the compiled C++ caller compares the shim with the C ABI itself, and what it writes is
compared with the Python surface."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_bilateral_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_bilateral_test.o")],
                   check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_python_surface(tmp_path):
    rows, cols = 70, 130
    x = synth.synth_frame(rows, cols, 6)
    x.tofile(tmp_path / "in.f32")
    exe = tmp_path / "shim_bilateral_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([str(exe), str(rows), str(cols), str(tmp_path / "in.f32"), str(tmp_path / "out.f32"), str(tmp_path / "filt.f32")],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    dense = np.fromfile(tmp_path / "out.f32", dtype=np.float32).reshape(rows, cols)
    filt = np.fromfile(tmp_path / "filt.f32", dtype=np.float32).reshape(rows, cols)
    with api.Context(0, rows, cols, 1) as ctx:
        assert_bit_equal(dense, ctx.complete(x, api.make_params(blur_type="bilateral_clone")), "C++ img_completion(bilateral_clone)")
        assert_bit_equal(filt, ctx.bilateral5(dense), "C++ bilateral_filter5")
