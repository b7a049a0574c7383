"""Undistortion and rectification (dcmt_rectify_map_dev, dcmt_rectify_dev, dcmt_rectify, make_rectify_calib, plan_rectify):
everything that needs no GPU.  The definition is include/dcmt.h's, restated in numpy in tests/rectify_restatement.py; these tests
hold the restatement to the properties the header promises.  The GPU side is tests/test_gpu_rectify.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rectify_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

CSRC = os.path.join(ROOT, "depth_completion_mt_amd", "csrc")
NEW = ("dcmt_rectify_map_dev", "dcmt_rectify_dev", "dcmt_rectify")
TOY_K = np.array([[25.0, 0.0, 14.5], [0.0, 24.0, 9.5], [0.0, 0.0, 1.0]])


def identity(K):
    return R.record(K, np.zeros(5), np.eye(3), K)


def test_entry_points_are_exported_and_reject_bad_arguments_without_gpu():
    nm = subprocess.run(["nm", "-D", "--defined-only", L.build()], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in L.EXPORTS and f" T {name}\n" in nm, name
    lib = L.lib()
    buf = np.zeros(1 << 16, np.uint8)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16
    src, table, mp, dst = a, a + 8192, a + 16384, a + 32768
    # no context: nothing is looked at, nothing is written (the checks on the buffers themselves: tests/plan_rectify_test.cpp)
    assert lib.dcmt_rectify_map_dev(None, table, 1, 4, 4, mp, None) == L.E_INVALID
    assert lib.dcmt_rectify_map_dev(None, None, 1, 4, 4, mp, None) == L.E_INVALID
    assert lib.dcmt_rectify_map_dev(None, table, 0, 4, 4, mp, None) == L.E_INVALID
    assert lib.dcmt_rectify_dev(None, src, 8, 8, 1, mp, 1, None, 0, dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_rectify_dev(None, src, 8, 8, 2, mp, 1, None, 0, dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_rectify_dev(None, src, 8, 8, 1, mp, 0, None, 0, dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_rectify_dev(None, src, 8, 8, 1, mp, 1, None, 2, dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_rectify_dev(None, src, 8, 8, 1, mp, 1, None, 0, src, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_rectify(None, src, 8, 8, 8, 1, table, dst, 4, 4, 4) == L.E_INVALID
    assert lib.dcmt_rectify(None, None, 8, 8, 8, 1, table, dst, 4, 4, 4) == L.E_INVALID
    assert not buf.any()


def test_plan_rectify(tmp_path):
    exe = str(tmp_path / "plan_rectify_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + CSRC, os.path.join(ROOT, "tests", "plan_rectify_test.cpp"),
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_record_layout():
    assert ctypes.sizeof(L.RectifyCalib) == 176
    offs = {n: getattr(L.RectifyCalib, n).offset for n, _ in L.RectifyCalib._fields_}
    want = {n: 8 * i for i, n in enumerate(("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3"))}
    want.update({"R": 72, "fxp": 144, "fyp": 152, "cxp": 160, "cyp": 168})
    assert offs == want
    d = api.RECTIFY_CALIB_DTYPE
    assert d.itemsize == 176 and {n: d.fields[n][1] for n in d.names} == want
    assert all(d.fields[n][0].base == np.dtype("<f8") for n in d.names) and d.fields["R"][0].shape == (9,)
    hdr = open(os.path.join(ROOT, "include", "dcmt.h")).read()
    assert "stated, never compared with an executing OpenCV" in hdr and "#define DCMT_RECTIFY_FORCE_GATHER 1u" in hdr
    assert L.RECTIFY_FORCE_GATHER == 1


def test_make_rectify_calib_refuses_what_the_device_answers_with_an_empty_map():
    t = api.make_rectify_calib(R.KITTI_K, R.KITTI_D, R.KITTI_R, R.KITTI_P, device=None)
    assert t.dtype == api.RECTIFY_CALIB_DTYPE and len(t) == 1
    assert t.tobytes() == R.record(R.KITTI_K, R.KITTI_D, R.KITTI_R, R.KITTI_P).tobytes()
    assert (t["fxp"][0], t["cyp"][0], t["k3"][0], t["R"][0][5]) == (R.KITTI_P[0, 0], R.KITTI_P[1, 2], R.KITTI_D[4], R.KITTI_R[1, 2])
    t3 = api.make_rectify_calib(R.KITTI_K, R.KITTI_D, R.KITTI_R, R.KITTI_P[:, :3], device=None)
    assert t3.tobytes() == t.tobytes()                                  # P as 3 x 3
    K2 = np.stack([R.KITTI_K, TOY_K])
    t2 = api.make_rectify_calib(K2, R.KITTI_D, np.stack([R.KITTI_R, np.eye(3)]), R.KITTI_P, device=None)
    assert len(t2) == 2 and t2[0].tobytes() == t[0].tobytes() and t2["fx"][1] == 25.0 and np.array_equal(t2["R"][1], np.eye(3).reshape(9))
    for bad in (np.nan, np.inf, -np.inf):
        for which in range(4):
            args = [R.KITTI_K.copy(), R.KITTI_D.copy(), R.KITTI_R.copy(), R.KITTI_P.copy()]
            args[which][(0,) * args[which].ndim] = bad                 # fx, k1, R[0], fxp
            with pytest.raises(ValueError):
                api.make_rectify_calib(*args, device=None)
            assert not R.record_ok(R.record(*args)[0])
    for i in (0, 1):
        P = R.KITTI_P.copy()
        P[i, i] = -0.0 if i else 0.0
        with pytest.raises(ValueError):
            api.make_rectify_calib(R.KITTI_K, R.KITTI_D, R.KITTI_R, P, device=None)
        assert not R.record_ok(R.record(R.KITTI_K, R.KITTI_D, R.KITTI_R, P)[0])
    with pytest.raises(ValueError):
        api.make_rectify_calib(R.KITTI_K, R.KITTI_D[:4], R.KITTI_R, R.KITTI_P, device=None)
    with pytest.raises(ValueError):
        api.make_rectify_calib(K2, R.KITTI_D, np.stack([R.KITTI_R] * 3), R.KITTI_P, device=None)


@pytest.mark.parametrize("K,shape", [(TOY_K, (20, 30)), (R.KITTI_K, (375, 1242))], ids=["toy", "kitti"])
def test_identity_map_and_remap(K, shape):
    rows, cols = shape
    m = R.rectify_map(identity(K), rows, cols)
    assert np.array_equal(m[..., 0], np.broadcast_to(32 * np.arange(cols, dtype=np.int32)[None, :], shape))
    assert np.array_equal(m[..., 1], np.broadcast_to(32 * np.arange(rows, dtype=np.int32)[:, None], shape))
    for ch in ((), (3,)):
        src = R.noise(shape + ch, 11)
        assert np.array_equal(R.remap(src, m), src)


def test_integer_and_half_pixel_shifts():
    rows, cols = 20, 30
    src = R.noise((rows, cols), 5)
    s = src.astype(np.int32)
    P = TOY_K.copy()
    P[0, 2] -= 3.0                                                      # the new camera looks 3 pixels to the right, 2 down
    P[1, 2] -= 2.0
    m = R.rectify_map(R.record(TOY_K, np.zeros(5), np.eye(3), P), rows, cols)
    assert np.array_equal(m[..., 0], np.broadcast_to(32 * (np.arange(cols) + 3)[None, :], (rows, cols)))
    want = np.zeros_like(src)
    want[:rows - 2, :cols - 3] = src[2:, 3:]
    assert np.array_equal(R.remap(src, m), want)                        # zeros where the source ends
    P = TOY_K.copy()
    P[0, 2] -= 0.5
    m = R.rectify_map(R.record(TOY_K, np.zeros(5), np.eye(3), P), rows, cols)
    assert np.array_equal(m[..., 0], np.broadcast_to((32 * np.arange(cols) + 16)[None, :], (rows, cols)))
    want = np.zeros((rows, cols), np.int32)
    want[:, :cols - 1] = (s[:, :-1] + s[:, 1:] + 1) >> 1
    want[:, cols - 1] = (s[:, -1] + 0 + 1) >> 1
    assert np.array_equal(R.remap(src, m), want.astype(np.uint8))
    P = TOY_K.copy()
    P[1, 2] -= 0.5
    m = R.rectify_map(R.record(TOY_K, np.zeros(5), np.eye(3), P), rows, cols)
    want = np.zeros((rows, cols), np.int32)
    want[:rows - 1] = (s[:-1] + s[1:] + 1) >> 1
    want[rows - 1] = (s[-1] + 1) >> 1
    assert np.array_equal(R.remap(src, m), want.astype(np.uint8))


def kitti_map():
    return R.rectify_map(R.record(R.KITTI_K, R.KITTI_D, R.KITTI_R, R.KITTI_P), *R.KITTI_DST)


def test_fixed_point_is_the_bilinear_sample_rounded_half_up():
    m = kitti_map()
    for ch in ((), (3,)):
        src = R.noise(R.KITTI_SRC + ch, 21)
        out = R.remap(src, m).astype(np.float64)
        ref = R.bilinear_f64(src, m)
        assert np.abs(out - ref).max() <= 0.5
        assert np.array_equal(out, np.floor(ref + 0.5))
    # ... also where samples fall outside: a view wider than the source
    small = R.noise((41, 150), 22)
    assert np.abs(R.remap(small, m[:60, :300]).astype(np.float64) - R.bilinear_f64(small, m[:60, :300])).max() <= 0.5


def test_map_accuracy_against_longdouble():
    rec = R.record(R.KITTI_K, R.KITTI_D, R.KITTI_R, R.KITTI_P)
    m = kitti_map()
    assert (m != R.OUTSIDE).all()
    tx, ty = R.coords_longdouble(rec, *R.KITTI_DST)
    assert float(np.abs(m[..., 0] - tx).max()) <= 0.5 + 1e-6 and float(np.abs(m[..., 1] - ty).max()) <= 0.5 + 1e-6
    # the map lies inside the 512 x 1392 sensor, all four samples of every pixel
    ix, iy = m[..., 0] >> 5, m[..., 1] >> 5
    assert ix.min() >= 0 and ix.max() + 1 < R.KITTI_SRC[1] and iy.min() >= 0 and iy.max() + 1 < R.KITTI_SRC[0]


def test_outside_maps_and_bad_records_give_zeros():
    src = R.noise((41, 150, 3), 31)
    for which, where, bad in ((0, (0, 2), np.nan), (1, (4,), np.inf), (2, (2, 2), -np.inf), (3, (1, 2), np.nan)):    # cx, k3, R[8], cyp
        args = [R.KITTI_K.copy(), R.KITTI_D.copy(), R.KITTI_R.copy(), R.KITTI_P.copy()]
        args[which][where] = bad
        m = R.rectify_map(R.record(*args), 37, 131)
        assert (m == R.OUTSIDE).all()
        assert not R.remap(src, m).any()
    P = R.KITTI_P.copy()
    P[0, 0] = 0.0
    assert (R.rectify_map(R.record(R.KITTI_K, R.KITTI_D, R.KITTI_R, P), 37, 131) == R.OUTSIDE).all()
    # a finite record whose coordinates overflow: a focal length of 1e300 puts every pixel but the principal column beyond 2^30
    K = TOY_K.copy()
    K[0, 0] = 1e300
    m = R.rectify_map(R.record(K, np.zeros(5), np.eye(3), np.array([[25.0, 0, 14.0], [0, 24.0, 9.0], [0, 0, 1.0]])), 20, 30)
    assert (m[:, np.arange(30) != 14] == R.OUTSIDE).all() and (m[:, 14] != R.OUTSIDE).all()
    # adversarial elements: nothing of the source is sampled
    adv = np.array([-2**31, 2**31 - 1, 2**30, -2**30, 0], np.int32)
    mm = np.stack(np.meshgrid(adv, adv, indexing="ij"), axis=-1).astype(np.int32)
    out = R.remap(src, mm)
    assert out.shape == (5, 5, 3) and not out[:4].any() and not out[:, :4].any() and np.array_equal(out[4, 4], src[0, 0])
    # the batch form: map by index, a bad index is a zero frame
    maps = np.stack([kitti_map()[:37, :131], R.rectify_map(identity(TOY_K), 37, 131)])
    frames = R.noise((4, 41, 150), 32)
    got = R.rectify(frames, maps, index=[1, 2, 0, -1])
    assert np.array_equal(got[0], R.remap(frames[0], maps[1])) and not got[1].any() and not got[3].any()
    assert np.array_equal(R.rectify(frames, maps)[3], R.remap(frames[3], maps[1]))


def test_python_layer_exports_the_new_functions():
    import depth_completion_mt_amd as pkg
    for name in ("RECTIFY_CALIB_DTYPE", "make_rectify_calib", "undistort_rectify"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(api, name)
    for name in ("rectify_map_dev", "rectify_dev", "rectify"):
        assert callable(getattr(api.Context, name))
