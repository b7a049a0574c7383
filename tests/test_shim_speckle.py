"""The speckle filter through the cv::Mat drop-in (include/img_completion.h): tests/mock_opencv/shim_speckle_test.cpp compiles on a CPU
against the cv::Mat stand-in with 16-bit elements; on the GPU the compiled C++ caller compares dcmt_shim::filter_speckles (a plane
with padded rows, in place, cv::filterSpeckles' argument order) with the C ABI itself, and what it leaves is compared with the
Python surface and the restatement.  With the stand-in the other shim tests use, which has no CV_16SC1, the header must still
compile, without the function."""
import os
import subprocess

import numpy as np
import pytest

import speckle_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_speckle_test.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv", "with_16s")]


def test_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall"] + INCLUDES + ["-c", DRIVER, "-o", str(tmp_path / "shim_speckle_test.o")],
                   check=True, capture_output=True)


def test_header_without_16_bit_elements_has_no_filter(tmp_path):
    src = tmp_path / "plain.cpp"
    src.write_text('#include "img_completion.h"\n#ifdef CV_16SC1\n#error "this stand-in was expected to have no CV_16SC1"\n#endif\n'
                   'namespace dcmt_shim { inline int filter_speckles(int) { return 1; } }      // no clash: the header left its own out\n'
                   'int main() { return dcmt_shim::filter_speckles(0) - 1; }\n')
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv"),
                    "-c", str(src), "-o", str(tmp_path / "plain.o")], check=True, capture_output=True)


@pytest.mark.gpu
def test_cpp_caller_matches_the_c_abi_and_the_python_surface(tmp_path):
    rows, cols = 21, 131
    for new_val, max_size, max_diff in ((-16, 5, 16), (123, 200, 32)):
        v = R.random_plane(rows, cols, 3, 0.6, 14, new_val=new_val)
        v.tofile(tmp_path / "disp16.i16")
        exe = tmp_path / "shim_speckle_test"
        lib_dir = os.path.dirname(L.LIB_PATH)
        subprocess.run(["g++", "-std=c++11", "-O1"] + INCLUDES + [DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
        r = subprocess.run([str(exe), str(rows), str(cols), str(new_val), str(max_size), str(max_diff)] +
                           [str(tmp_path / f) for f in ("disp16.i16", "out.i16")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
        out = np.fromfile(tmp_path / "out.i16", dtype=np.int16).reshape(rows, cols)
        want, changed = R.vectorised(v, max_size=max_size, max_diff=max_diff, new_val=new_val)
        assert np.array_equal(out, want) and 0 < changed.sum() and (want != new_val).any()
        got, n = api.filter_speckles(v, max_size=max_size, max_diff=max_diff, new_val=new_val)
        assert np.array_equal(got, out) and n == changed.sum()
