"""The cascade without its extrapolation through the cv::Mat drop-in (include/img_completion.h):
tests/mock_opencv/shim_no_extrapolate_test.cpp compiles on a CPU against the cv::Mat stand-in; on the GPU the compiled C++ caller
compares the shim with the C ABI itself, and what it writes and prints is compared with the restatement."""
import os
import subprocess

import numpy as np
import pytest

import no_extrapolate_restatement as R
from conftest import ROOT, assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import synth

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_no_extrapolate_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_no_extrapolate_test.o")],
                   check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_restatement(tmp_path):
    rows, cols = 70, 130
    x = synth.synth_frame(rows, cols, 6)
    x.tofile(tmp_path / "in.f32")
    exe = tmp_path / "shim_no_extrapolate_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([str(exe), str(rows), str(cols), str(tmp_path / "in.f32"), str(tmp_path / "out.f32"), str(tmp_path / "lab.f32")],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    # the reference's two header lines and no hole counts; the labeled twin prints nothing
    assert r.stdout.strip().splitlines() == [f"NUMERO ROWS, COLS: {rows} {cols}", f"max range is{float(x.max()):g}"], r.stdout
    dense = np.fromfile(tmp_path / "out.f32", dtype=np.float32).reshape(rows, cols)
    assert_bit_equal(dense, R.restatement_oracle(x), "C++ img_completion_no_extrapolate")
    assert (dense == 0).any()
    yy, xx = np.mgrid[0:rows, 0:cols]
    gx = (cols + 8) // 9
    labels = ((yy // 9) * gx + xx // 9).astype(np.int32)
    lab = np.fromfile(tmp_path / "lab.f32", dtype=np.float32).reshape(rows, cols)
    assert_bit_equal(lab, R.restatement_oracle(x, labels=labels, n_labels=int(labels.max()) + 1), "C++ interpolate_with_labels_no_extrapolate")
