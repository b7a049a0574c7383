"""SLIC's two pixel renderings through the cv::Mat drop-in (include/img_completion.h): tests/mock_opencv/shim_contours_test.cpp compiles
on a CPU against the cv::Mat stand-in; on the GPU the compiled C++ caller compares dcmt_shim::slic_display_contours and
dcmt_shim::slic_colour_with_cluster_means ([col][row] labels, cv::Mat in place) with the C ABI itself, and what it writes is compared
with the Python surface and the literal restatements."""
import os
import subprocess

import numpy as np
import pytest

import contours_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_contours_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_contours_test.o")],
                   check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_python_surface(tmp_path):
    rows, cols, n_labels = 70, 130, 12
    plane, img = R.voronoi(rows, cols, 14, 9), R.image_for(rows, cols, 9)         # labels 12 and 13 are out of range
    assert plane.max() == 13
    plane.tofile(tmp_path / "labels.i32")
    img.tofile(tmp_path / "image.u8")
    exe = tmp_path / "shim_contours_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([str(exe), str(rows), str(cols), str(n_labels)] + [str(tmp_path / f) for f in ("labels.i32", "image.u8", "contours.u8", "means.u8")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    contours = np.fromfile(tmp_path / "contours.u8", dtype=np.uint8).reshape(rows, cols, 3)
    means = np.fromfile(tmp_path / "means.u8", dtype=np.uint8).reshape(rows, cols, 3)
    assert np.array_equal(contours, R.paint(img, R.literal_contours(plane))) and np.array_equal(means, R.literal_means(plane, img, n_labels)[0])
    assert np.array_equal(api.slic_display_contours(plane, img), contours) and np.array_equal(api.slic_colour_with_cluster_means(plane, img, n_labels), means)
