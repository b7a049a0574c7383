"""DCMT_FLAG_NO_EXTRAPOLATE without a GPU: the two restatements of its definition (tests/no_extrapolate_restatement.py: (a) from the
oracle's exports, (b) from oracle/np_restatement.py) agree bit for bit, the definition's stated consequences hold, the dispatch
plans what the issue pins (tests/plan_noext_test.cpp), and the flag reaches dcmt_params through make_params(extrapolate=False)."""
import os
import subprocess

import numpy as np
import pytest

import no_extrapolate_restatement as R
from conftest import ROOT, assert_bit_equal
from oracle import oracle as O

f32 = np.float32
SHAPES = [(8, 8), (9, 70), (33, 129), (64, 250)]


@pytest.mark.parametrize("k0", ["as_compiled", "diamond"])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_restatements_agree_on_random_planes(rows, cols, k0):
    x = R.random_plane(rows, cols, 100 * rows + cols)
    for stop in (9, 10, 11):
        for blur in ("none", "gaussian"):
            a = R.restatement_oracle(x, k0, blur, stop)
            b = R.restatement_numpy(x, k0, blur, stop)
            assert_bit_equal(a, b, f"{rows}x{cols} {k0} stop {stop} {blur}")
    if rows >= 33:
        assert (R.restatement_oracle(x, k0) < R.THR).any(), "the plane keeps holes: nothing is extrapolated"


@pytest.mark.parametrize("k0", ["as_compiled", "diamond"])
def test_restatements_agree_on_adversarial_planes(k0):
    for name, x in R.adversarial_planes().items():
        for stop in (9, 10, 11):
            for blur in ("none", "gaussian"):
                assert_bit_equal(R.restatement_oracle(x, k0, blur, stop), R.restatement_numpy(x, k0, blur, stop), f"{name} {k0} stop {stop} {blur}")


def test_restatements_agree_with_labels():
    rows, cols = 33, 70
    x = R.random_plane(rows, cols, 5, density=0.02)
    yy, xx = np.mgrid[0:rows, 0:cols]
    labels = ((yy // 9) * 8 + xx // 9).astype(np.int32)
    n = int(labels.max()) + 1
    for k0 in ("as_compiled", "diamond"):
        for stop in (9, 10, 11):
            assert_bit_equal(R.restatement_oracle(x, k0, "none", stop, labels, n), R.restatement_numpy(x, k0, "none", stop, labels, n), f"labels {k0} {stop}")


def test_consequences_of_the_definition():
    planes = R.adversarial_planes()
    z = planes["all zero"]
    for blur in ("none", "gaussian"):
        assert_bit_equal(R.restatement_oracle(z, blur=blur), z, "an all-zero frame stays all zero")
    # X5 without a hole: the extension and both fills change nothing, so the default call's bits
    full = planes["fully valid"]
    for k0 in ("as_compiled", "diamond"):
        assert (R.x5_oracle(full, k0) >= R.THR).all()
        for blur in ("none", "gaussian"):
            for stop in (9, 10, 11):
                assert_bit_equal(R.restatement_oracle(full, k0, blur, stop), O.img_completion(full, O.default_params(k0=k0, blur=blur, stop_after=stop)),
                                 f"fully valid {k0} {blur} {stop}")
    # a median that is valid with a blurred value below thr: not inverted
    far = planes["far"]
    m = R.uninverted_pixels(far)
    assert m.any(), "the fixture holds no un-inverted pixel"
    x10, x11 = R.restatement_oracle(far, stop_after=10), R.restatement_oracle(far, stop_after=11)
    assert_bit_equal(x11[m], x10[m], "un-inverted pixels")
    inv = x10 >= R.THR
    assert inv.any() and np.array_equal(x11[inv], f32(100.0) - x10[inv])
    # the threshold itself is valid, the float below it is not
    t = planes["threshold"]
    x2 = O.img_completion(t, O.default_params(stop_after=2))
    assert (x2[t == R.THR] == f32(100.0) - R.THR).all() and (x2[(t > 0) & (t < R.THR)] < R.THR).all()
    # on the project's own input the mode is far from a no-op
    x = O.synth_frame(352, 1216, 1)
    x5 = R.x5_oracle(x)
    got = R.restatement_oracle(x)
    assert int((x5 < R.THR).sum()) == 152937 and int((got == 0).sum()) == 150544
    assert int((got.view(np.uint32) != O.img_completion(x).view(np.uint32)).sum()) == 192275


def test_plan(tmp_path):
    exe = str(tmp_path / "plan_noext_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "depth_completion_mt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "plan_noext_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_make_params_sets_the_flag():
    from depth_completion_mt_amd import _lib as L
    from depth_completion_mt_amd import api
    assert L.FLAG_NO_EXTRAPOLATE == 8
    assert api.make_params().flags & L.FLAG_NO_EXTRAPOLATE == 0
    assert api.make_params(extrapolate=True).flags == api.make_params().flags
    p = api.make_params(extrapolate=False, normalize=(0, 80), force_staged=True)
    assert p.flags == L.FLAG_NO_EXTRAPOLATE | L.FLAG_NORMALIZE | L.FLAG_FORCE_STAGED
    q = api.make_params()
    for name, _ in L.Params._fields_:
        if name not in ("flags", "k0", "_pad"):
            assert getattr(api.make_params(extrapolate=False), name) == getattr(q, name), name
    assert L.lib().dcmt_version() == 120
    with open(os.path.join(ROOT, "include", "dcmt.h")) as f:
        assert "#define DCMT_FLAG_NO_EXTRAPOLATE 8" in f.read()
