"""8-bit BGR -> Lab and BGR -> grey (dcmt_bgr_convert*, dcmt_lab_tables, tools/make_lab_tables.py, plan_bgr_convert, the shim's
bgr_to_lab / bgr_to_gray): everything that needs no GPU.  The definition is restated in numpy in tests/bgr_restatement.py; the
pins below were computed once, on a CPU, and are what DESIGN section 15 states.  The GPU side is tests/test_gpu_bgr_convert.py."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np

import bgr_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L

CSRC = os.path.join(ROOT, "depth_completion_mt_amd", "csrc")
SHA_GAMMA = "8bfeace00785402e67e5c7d4c53961990e4987ccd31692c42d4b080aeb6dc153"
SHA_CBRT = "e34f178a79f106b857ad23da4f18224536271e8a14e858797f7b8e723fd9ff64"
SHA_CUBE_LAB = "2f00e5b9a30983704f83a0a5aa4e39f5f5794b8e2ba161e8218a53f92ffddcf3"
SHA_CUBE_GRAY = "6d4f6d7f4301c52d2672db66451b4a06a5502bef956dd81b577660f956f410ae"
COEF = [[1777, 1541, 778], [871, 2929, 296], [73, 448, 3575]]
# (B, G, R) -> (L, a, b), Y; the three pure colours agree with what OpenCV is known to return for them
SAMPLES = [((0, 0, 0), (0, 128, 128), 0), ((255, 255, 255), (255, 128, 128), 255), ((255, 0, 0), (82, 207, 20), 29),
           ((0, 255, 0), (224, 42, 211), 150), ((0, 0, 255), (136, 208, 195), 76), ((1, 2, 3), (1, 128, 128), 2),
           ((30, 60, 90), (72, 138, 152), 66), ((128, 128, 128), (137, 128, 128), 128)]


def _generator():
    spec = importlib.util.spec_from_file_location("make_lab_tables", os.path.join(ROOT, "tools", "make_lab_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_reproduces_the_table_pins():
    assert R.GAMMA.dtype == np.uint16 and R.GAMMA.shape == (256,) and R.CBRT.dtype == np.uint16 and R.CBRT.shape == (3072,)
    assert R.sha256(R.GAMMA.astype("<u2")) == SHA_GAMMA
    assert R.sha256(R.CBRT.astype("<u2")) == SHA_CBRT
    assert R.GAMMA[[0, 1, 10, 11, 12, 128, 255]].tolist() == [0, 1, 6, 7, 8, 440, 2040] and int(R.GAMMA.max()) == 2040
    assert R.CBRT[[0, 1, 18, 19, 20, 2040, 3071]].tolist() == [4520, 4645, 6771, 6894, 7013, 32768, 37555] and int(R.CBRT.max()) == 37555
    assert R.C.tolist() == COEF and R.C.sum(axis=1).tolist() == [4096] * 3


def test_restatement_reproduces_the_sample_pixels():
    for bgr, lab, y in SAMPLES:
        px = np.array(bgr, np.uint8)
        assert tuple(R.bgr_to_lab(px).tolist()) == lab, bgr
        assert int(R.bgr_to_gray(px)) == y, bgr


def test_restatement_over_the_whole_colour_cube():
    cube = R.cube_reference()
    assert R.colour_cube(0x030201, 1).tolist() == [[1, 2, 3]]                       # pixel k: B = k & 255, G = (k >> 8) & 255, R = k >> 16
    assert R.sha256(cube["lab"]) == SHA_CUBE_LAB
    assert R.sha256(cube["gray"]) == SHA_CUBE_GRAY
    # L, a, b fit a byte as they come: the kernel does not clamp
    assert cube["lo"].tolist() == [0, 42, 20] and cube["hi"].tolist() == [255, 226, 223]
    assert cube["max_index"] == 2040                                                # the rows of C sum to 4096: cbrt is never read past gamma's maximum
    assert int(cube["gray"].min()) == 0 and int(cube["gray"].max()) == 255


def test_deviation_from_the_documented_conversion_is_capped():
    """Against L * 255 / 100, a + 128, b + 128 of the CIE formulas in f64 and round(0.299 R + 0.587 G + 0.114 B), over all 2^24
    colours: properties of the fixed-point scheme, asserted as caps so that a slip in a constant cannot hide."""
    dev = R.cube_deviation()
    worst = [int(np.nonzero(h)[0].max()) for h in list(dev["lab"]) + [dev["gray"]]]
    print("largest deviation of L, a, b, grey:", worst, "; colours at each number of levels, L, a, b:", dev["lab"][:, :5].tolist(),
          "grey:", dev["gray"][:5].tolist())
    assert int(dev["lab"].sum()) == 3 << 24 and int(dev["gray"].sum()) == 1 << 24
    assert worst[3] <= 1
    assert worst[0] <= 2 and worst[1] <= 3 and worst[2] <= 2


def test_generator_regenerates_the_committed_tables_exactly():
    gen = _generator()
    assert np.array_equal(gen.gamma_table(), R.GAMMA) and np.array_equal(gen.cbrt_table(), R.CBRT)
    assert gen.coefficients().tolist() == COEF
    assert gen.sha256_le16(gen.gamma_table()) == SHA_GAMMA and gen.sha256_le16(gen.cbrt_table()) == SHA_CBRT
    with open(os.path.join(CSRC, "dcmt_lab_tables.h")) as f:
        assert f.read() == gen.render()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_lab_tables.py")], capture_output=True, text=True, check=True)
    assert SHA_GAMMA in r.stdout and SHA_CBRT in r.stdout


def test_library_returns_the_same_tables():
    gamma, cbrt, coef = (ctypes.c_uint16 * 256)(), (ctypes.c_uint16 * 3072)(), (ctypes.c_int32 * 9)()
    lib = L.lib()
    lib.dcmt_lab_tables(gamma, cbrt, coef)
    assert np.array_equal(np.ctypeslib.as_array(gamma), R.GAMMA)
    assert np.array_equal(np.ctypeslib.as_array(cbrt), R.CBRT)
    assert np.ctypeslib.as_array(coef).reshape(3, 3).tolist() == COEF
    lib.dcmt_lab_tables(None, None, None)                                           # each pointer is optional
    only = (ctypes.c_int32 * 9)()
    lib.dcmt_lab_tables(None, None, only)
    assert list(only) == sum(COEF, [])


def test_entry_points_are_exported_and_reject_bad_arguments_without_gpu():
    nm = subprocess.run(["nm", "-D", "--defined-only", L.build()], capture_output=True, text=True, check=True).stdout
    for name in ("dcmt_bgr_convert_dev", "dcmt_bgr_convert", "dcmt_lab_tables"):
        assert name in L.EXPORTS and f" T {name}\n" in nm, name
    lib = L.lib()
    assert lib.dcmt_version() == 120
    buf = np.zeros(3 * 64 + 64 + 3 * 64, np.uint8)
    bgr, gray, lab = buf.ctypes.data, buf.ctypes.data + 192, buf.ctypes.data + 256
    # no context: nothing is looked at, nothing is written (the checks on the buffers themselves: tests/plan_bgr_test.cpp)
    assert lib.dcmt_bgr_convert_dev(None, bgr, 8, 8, 1, lab, gray, None) == L.E_INVALID
    assert lib.dcmt_bgr_convert_dev(None, None, 8, 8, 1, lab, gray, None) == L.E_INVALID
    assert lib.dcmt_bgr_convert_dev(None, bgr, 8, 8, 1, None, None, None) == L.E_INVALID
    assert lib.dcmt_bgr_convert_dev(None, bgr, 0, 8, 1, lab, None, None) == L.E_INVALID
    assert lib.dcmt_bgr_convert_dev(None, bgr, 8, -1, 1, None, gray, None) == L.E_INVALID
    assert lib.dcmt_bgr_convert_dev(None, bgr, 1 << 20, 1 << 20, 70000, lab, gray, None) == L.E_INVALID
    assert lib.dcmt_bgr_convert_dev(None, bgr, 8, 8, 1, bgr + 3, None, None) == L.E_INVALID          # partial overlap
    assert lib.dcmt_bgr_convert_dev(None, bgr, 8, 8, 1, None, bgr + 8, None) == L.E_INVALID          # gray inside bgr
    assert lib.dcmt_bgr_convert(None, bgr, 24, 8, 8, lab, 24, gray, 8) == L.E_INVALID
    assert lib.dcmt_bgr_convert(None, None, 24, 8, 8, lab, 24, gray, 8) == L.E_INVALID
    assert lib.dcmt_bgr_convert(None, bgr, 24, 8, 8, None, 0, None, 0) == L.E_INVALID
    assert lib.dcmt_bgr_convert(None, bgr, 24, 1 << 20, 1 << 20, lab, 3 << 20, None, 0) == L.E_INVALID
    assert not buf.any()


def test_plan_of_the_bgr_conversion(tmp_path):
    exe = str(tmp_path / "plan_bgr_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + CSRC, os.path.join(ROOT, "tests", "plan_bgr_test.cpp"),
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_shim_driver_compiles_against_the_mock_headers(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv"),
                    "-c", os.path.join(ROOT, "tests", "mock_opencv", "bgr_test.cpp"), "-o", str(tmp_path / "bgr_test.o")],
                   check=True, capture_output=True)


def test_python_layer_exports_the_new_functions():
    import depth_completion_mt_amd as pkg
    from depth_completion_mt_amd import api
    assert "bgr_to_lab" in pkg.__all__ and "bgr_to_gray" in pkg.__all__
    assert pkg.bgr_to_lab is api.bgr_to_lab and pkg.bgr_to_gray is api.bgr_to_gray
    assert callable(api.Context.bgr_convert_dev) and callable(api.Context.bgr_convert)
