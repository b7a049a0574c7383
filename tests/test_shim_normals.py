"""The normals and the flying-pixel filter through the cv::Mat drop-in (include/img_completion.h): tests/mock_opencv/shim_normals_test.cpp
compiles on a CPU against the cv::Mat stand-in; on the GPU the compiled C++ caller compares dcmt_shim::depth_normals and
dcmt_shim::filter_flying_pixels (cv::Mat in, a fresh cv::Mat and a vector of records out) with the C ABI itself, and what it writes is
compared with the Python surface and the literal restatement."""
import os
import subprocess

import numpy as np
import pytest

import normals_restatement as N
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_normals_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv")]
u32 = np.uint32


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_normals_test.o")],
                   check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_python_surface(tmp_path):
    rows, cols = 70, 131
    depth = N.holey_plane(rows, cols, 9)
    depth.tofile(tmp_path / "depth.f32")
    exe = tmp_path / "shim_normals_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([str(exe), str(rows), str(cols), str(tmp_path / "depth.f32"), str(tmp_path / "filtered.f32"), str(tmp_path / "normals.f32")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    filtered = np.fromfile(tmp_path / "filtered.f32", dtype=np.float32).reshape(rows, cols)
    normals = np.fromfile(tmp_path / "normals.f32", dtype=np.float32).reshape(rows, cols, 4)
    want_n = N.literal(depth)[0]
    want_f, removed = N.literal(depth, min_plane_dist=30.0, **N.KITTI)[1:3]
    assert removed > 0 and np.array_equal(filtered.view(u32), want_f.view(u32)) and np.array_equal(normals.view(u32), want_n.view(u32))
    assert np.array_equal(api.depth_normals(depth).view(u32), normals.view(u32))
    assert np.array_equal(api.filter_flying_pixels(depth, api.make_cloud_params(**N.KITTI), min_plane_dist=30.0).view(u32), filtered.view(u32))
