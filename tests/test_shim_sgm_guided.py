"""The guided stereo matcher through the cv::Mat drop-in (include/img_completion.h): dcmt_shim::stereo_sgm_guided.
tests/mock_opencv/shim_sgm_guided_test.cpp compiles on a CPU against the cv::Mat stand-in with 16-bit elements, the way
tests/test_shim_sgm_paths.py compiles its program; on the GPU the compiled C++ caller compares the shim with the C ABI itself, and what
it writes is compared with the Python surface and the guided restatement."""
import os
import subprocess

import numpy as np
import pytest

import sgm_guided_restatement as GR
import sgm_paths_restatement as P
import sgm_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_sgm_guided_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv", "with_16s")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_sgm_guided_test.o")],
                   check=True, capture_output=True)


def test_header_without_16_bit_elements_has_no_guided_function(tmp_path):
    src = tmp_path / "plain.cpp"
    src.write_text('#include "img_completion.h"\n#ifdef CV_16SC1\n#error "this stand-in was expected to have no CV_16SC1"\n#endif\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv"),
                    "-c", str(src), "-o", str(tmp_path / "plain.o")], check=True, capture_output=True)
    hdr = open(os.path.join(ROOT, "include", "img_completion.h")).read()
    guard, end = hdr.index("#ifdef CV_16SC1"), hdr.index("#endif", hdr.index("inline void stereo_sgm_guided("))
    assert guard < hdr.index("inline void stereo_sgm_guided(const cv::Mat& left_gray, const cv::Mat& right_gray, const cv::Mat& guide, cv::Mat& disp16, int paths,") < end
    assert "#endif" not in hdr[hdr.index("inline void stereo_sgm_paths("):hdr.index("inline void stereo_sgm_guided(")]      # the siblings' guard


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_python_surface(tmp_path):
    rows, cols, D = 21, 131, 32
    left, right = R.shifted_pair(rows, cols, 14)
    guide = GR.guide_kinds(rows, cols, D)["dense"]
    want16 = GR.vectorised(left, right, guide, 8, num_disparities=D)[0]
    assert not np.array_equal(want16, P.vectorised(left, right, num_disparities=D)[0])        # the driver relies on it: the guide changes something
    for name, a in (("left.u8", left), ("right.u8", right), ("guide.f32", guide)):
        a.tofile(tmp_path / name)
    exe = tmp_path / "shim_sgm_guided_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    r = subprocess.run([str(exe), str(rows), str(cols), str(D)] + [str(tmp_path / f) for f in ("left.u8", "right.u8", "guide.f32", "disp16.i16")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    d16 = np.fromfile(tmp_path / "disp16.i16", dtype=np.int16).reshape(rows, cols)
    assert np.array_equal(d16, want16) and (d16 > 0).mean() > 0.5
    assert np.array_equal(api.stereo_sgm(left, right, num_disparities=D, paths=8, guide=guide), d16)
