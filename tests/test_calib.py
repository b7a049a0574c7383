"""Per-frame calibration tables for the four geometric *_dev calls (dcmt_project_points_calib_dev, dcmt_depth_to_cloud_calib_dev,
dcmt_reproject_depth_calib_dev, dcmt_stereo_refine_calib_dev; api.make_*_calib, Context.*_calib_dev): what needs no GPU.  The
exports and layouts of include/dcmt.h, the argument checks, the table builders, and -- the premise of test_gpu_calib.py -- that
every input set used there tells a frame's own record from every other frame's (calib_cases.power)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import calib_cases as C
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

NAMES = ("dcmt_project_points_calib_dev", "dcmt_depth_to_cloud_calib_dev", "dcmt_reproject_depth_calib_dev", "dcmt_stereo_refine_calib_dev")
f32 = np.float32


def test_the_four_names_are_exported():
    nm = subprocess.run(["nm", "-D", "--defined-only", L.build()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dcmt_[a-z0-9_]+)", nm))
    hdr = open(os.path.join(ROOT, "include", "dcmt.h")).read()
    for name in NAMES:
        assert name in L.EXPORTS and name in exported and getattr(L.lib(), name) is not None
        assert re.search(r"\bint " + name + r"\(", hdr), name
    assert L.lib().dcmt_version() == 120
    import depth_completion_mt_amd as pkg
    for name in ("make_project_calib", "make_cloud_calib", "make_reproject_calib", "make_stereo_calib", "calib_to_device"):
        assert getattr(pkg, name) is getattr(api, name)
    for name in ("project_points_calib_dev", "depth_to_cloud_calib_dev", "reproject_depth_calib_dev", "stereo_refine_calib_dev"):
        assert callable(getattr(api.Context, name))


def test_struct_sizes_and_field_offsets_are_the_header_s():
    assert ctypes.sizeof(L.ProjectCalib) == 96 and ctypes.sizeof(L.StereoCalib) == 8
    assert (L.ProjectCalib.T.offset, L.ProjectCalib.P.offset) == (0, 48)
    assert (L.StereoCalib.baseline.offset, L.StereoCalib.focal.offset) == (0, 4)
    # the two tables that reuse a parameter struct
    assert ctypes.sizeof(L.CloudParams) == 32 and [getattr(L.CloudParams, k).offset for k in ("fx", "fy", "cx", "cy")] == [0, 8, 16, 24]
    assert ctypes.sizeof(L.ReprojectParams) == 136
    assert [getattr(L.ReprojectParams, k).offset for k in ("fx", "fy", "cx", "cy", "M", "K")] == [0, 8, 16, 24, 32, 96]
    hdr = open(os.path.join(ROOT, "include", "dcmt.h")).read()
    assert "typedef struct { float T[12]; float P[12]; } dcmt_project_calib;" in hdr
    assert re.search(r"typedef struct \{ float baseline, focal; \}\s+dcmt_stereo_calib;", hdr)
    for dt, ct in ((api.PROJECT_CALIB_DTYPE, L.ProjectCalib), (api.STEREO_CALIB_DTYPE, L.StereoCalib), (api.CLOUD_CALIB_DTYPE, L.CloudParams),
                   (api.REPROJECT_CALIB_DTYPE, L.ReprojectParams)):
        assert dt.itemsize == ctypes.sizeof(ct)
        assert {k: dt.fields[k][1] for k in dt.names} == {k: getattr(ct, k).offset for k, _ in ct._fields_}


def test_table_checks_on_a_cpu(tmp_path):
    """The null / misaligned / overlapping table decisions of the four entry points are two pure functions of csrc/dcmt_plan_side.h
    (calib_table_aligned, calib_table_clear_of); tests/plan_calib_test.cpp runs them on a CPU, built against the headers alone.  The
    same decisions through the entry points, on a live context, are in test_gpu_calib.py."""
    exe = str(tmp_path / "plan_calib_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "depth_completion_mt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "plan_calib_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    for src in ("dcmt.hip", "dcmt_cloud.hip"):                  # ... and the entry points do decide with them
        txt = open(os.path.join(ROOT, "depth_completion_mt_amd", "csrc", src)).read()
        assert txt.count("plan::calib_table_aligned(") == 2 and txt.count("plan::calib_table_clear_of(") >= 2, src


def test_null_context_without_gpu():
    """Without a device no context exists, so every call here ends at the null context, whatever its table: DCMT_E_INVALID, and
    nothing is touched."""
    lib = L.lib()
    src = (ctypes.c_float * 64)()
    img = (ctypes.c_uint8 * 64)()
    pts = (L.CloudPoint * 16)()
    off = (ctypes.c_int32 * 4)()
    table = (ctypes.c_uint8 * 1024)()
    at = ctypes.addressof(table)
    at += -at % 16
    sp = L.StereoParams()
    lib.dcmt_default_stereo_params(ctypes.byref(sp))
    out = ctypes.addressof(src)
    for t in (at, None, at + 4, out):                       # good, null, misaligned, overlapping the output
        assert lib.dcmt_project_points_calib_dev(None, src, off, 4, 1, t, out, 4, 4, None) == L.E_INVALID
        assert lib.dcmt_depth_to_cloud_calib_dev(None, src, None, 4, 4, 1, t if t != out else ctypes.addressof(pts), pts, 16, off, None) == L.E_INVALID
        assert lib.dcmt_reproject_depth_calib_dev(None, src, 4, 4, 1, t, out, 4, 4, None) == L.E_INVALID
        assert lib.dcmt_stereo_refine_calib_dev(None, src, img, img, out, 4, 4, 1, ctypes.byref(sp), t, None) == L.E_INVALID
    assert lib.dcmt_stereo_refine_calib_dev(None, None, None, None, None, 4, 4, 1, None, None, None) == L.E_INVALID
    assert lib.dcmt_depth_to_cloud_calib_dev(None, src, None, 1 << 20, 1 << 20, 70000, at, pts, 16, off, None) == L.E_INVALID


def test_make_calib_helpers_produce_the_c_layout():
    b = 3
    T, P = C.project_records(b, 16, 24)
    t = api.make_project_calib(T, P)
    assert t.dtype == api.PROJECT_CALIB_DTYPE and t.shape == (b,) and t.nbytes == 96 * b
    raw = np.frombuffer(t.tobytes(), f32).reshape(b, 24)
    assert np.array_equal(raw[:, :12], T[:, :3].reshape(b, 12)) and np.array_equal(raw[:, 12:], P.reshape(b, 12))
    assert np.array_equal(api.make_project_calib(T[:, :3], P).view(np.uint8), t.view(np.uint8))          # [b][3][4] is taken too
    rec = ctypes.cast(t.ctypes.data, ctypes.POINTER(L.ProjectCalib))
    assert list(rec[2].T) == T[2, :3].ravel().tolist() and list(rec[2].P) == P[2].ravel().tolist()

    c = api.make_cloud_calib([700.0, 800.0, 900.0], 650.0, [10.0, 11.0, 12.0], -3.5)
    assert c.dtype == api.CLOUD_CALIB_DTYPE and c.nbytes == 32 * b
    assert np.array_equal(np.frombuffer(c.tobytes(), np.float64).reshape(b, 4), [[700, 650, 10, -3.5], [800, 650, 11, -3.5], [900, 650, 12, -3.5]])

    M, K, kw = C.reproject_records(b, 6, 9, 5, 7)
    r = C.reproject_table(M, K, kw)
    assert r.dtype == api.REPROJECT_CALIB_DTYPE and r.nbytes == 136 * b
    rec = ctypes.cast(r.ctypes.data, ctypes.POINTER(L.ReprojectParams))
    for f in range(b):
        assert (rec[f].fx, rec[f].fy, rec[f].cx, rec[f].cy) == tuple(kw[f][k] for k in ("fx", "fy", "cx", "cy"))
        assert list(rec[f].M) == M[f].ravel().tolist() and list(rec[f].K) == K[f].ravel().tolist()
        one = api.make_reproject_params(M=M[f], K=K[f], **kw[f])          # the record IS the uniform call's struct
        assert bytes(one)[:132] == r[f].tobytes()[:132]

    s = api.make_stereo_calib([0.5, 0.54, 0.6], [700.0, 800.0, 959.791])
    assert s.dtype == api.STEREO_CALIB_DTYPE and s.nbytes == 8 * b
    assert np.array_equal(np.frombuffer(s.tobytes(), f32).reshape(b, 2), np.array([[0.5, 700.0], [0.54, 800.0], [0.6, 959.791]], f32))
    assert np.array_equal(api.make_stereo_calib(0.54, [1.0, 2.0])["baseline"], np.array([0.54, 0.54], f32))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_make_calib_helpers_reject_a_non_finite_entry(bad):
    b = 3
    T, P = C.project_records(b, 16, 24)
    for where in ((0, 0, 0), (1, 2, 3)):
        for which in (0, 1):
            m = [T.copy(), P.copy()]
            m[which][where] = bad
            with pytest.raises(ValueError):
                api.make_project_calib(*m)
    T2 = T.copy()
    T2[1, 3, 2] = bad                                        # the bottom row of T is never used
    assert np.array_equal(api.make_project_calib(T2, P).view(np.uint8), api.make_project_calib(T, P).view(np.uint8))
    good = dict(fx=[700.0, 800.0, 900.0], fy=[650.0] * 3, cx=[10.0] * 3, cy=[5.0] * 3)
    M, K, _ = C.reproject_records(b, 6, 9, 5, 7)
    for k in good:
        kw = {n: list(v) for n, v in good.items()}
        kw[k][1] = bad
        with pytest.raises(ValueError):
            api.make_cloud_calib(**kw)
        with pytest.raises(ValueError):
            api.make_reproject_calib(M, K, **kw)
    for which, where in ((0, (2, 1, 3)), (0, (0, 2, 0)), (1, (1, 0, 2)), (1, (2, 1, 1))):
        m = [M.copy(), K.copy()]
        m[which][where] = bad
        with pytest.raises(ValueError):
            api.make_reproject_calib(*m, **good)
    M2, K2 = M.copy(), K.copy()
    M2[0, 3, 1] = bad                                        # M's 4th row and K's 3rd are never read
    K2[2, 2, 0] = bad
    assert api.make_reproject_calib(M2, K2, **good).shape == (b,)
    with pytest.raises(ValueError):
        api.make_stereo_calib([0.5, bad, 0.6], [700.0, 800.0, 900.0])
    with pytest.raises(ValueError):
        api.make_stereo_calib([0.5, 0.54, 0.6], [700.0, 800.0, bad])


def test_make_calib_helpers_take_scalars_for_any_argument_but_not_for_all():
    c = api.make_cloud_calib(700.0, [650.0, 660.0], 10.0, 5.0)                    # fx a scalar, fy the array
    assert c.shape == (2,) and c["fx"].tolist() == [700.0, 700.0] and c["fy"].tolist() == [650.0, 660.0]
    s = api.make_stereo_calib([0.5, 0.54, 0.6], 800.0)                            # focal a scalar, baseline the array
    assert s.shape == (3,) and s["focal"].tolist() == [800.0] * 3
    for bad in (lambda: api.make_cloud_calib(700.0, 650.0, 10.0, 5.0), lambda: api.make_stereo_calib(0.54, 800.0),
                lambda: api.make_cloud_calib([700.0, 800.0], [650.0] * 3, 10.0, 5.0), lambda: api.make_stereo_calib([[0.5]], [800.0])):
        with pytest.raises(ValueError, match="arrays of one common length"):
            bad()


def test_make_calib_helpers_reject_a_zero_focal_length():
    M, K, _ = C.reproject_records(3, 6, 9, 5, 7)
    for k in ("fx", "fy"):
        for zero in (0.0, -0.0):
            kw = dict(fx=[700.0, 800.0, 900.0], fy=[650.0] * 3, cx=[10.0] * 3, cy=[5.0] * 3)
            kw[k][2] = zero
            with pytest.raises(ValueError):
                api.make_cloud_calib(**kw)
            with pytest.raises(ValueError):
                api.make_reproject_calib(M, K, **kw)
    assert api.make_cloud_calib([700.0], [650.0], [0.0], [0.0]).shape == (1,)           # cx, cy zero are fine
    with pytest.raises(ValueError):
        api.make_stereo_calib([0.5, 0.54], [700.0, 0.0])


@pytest.mark.parametrize("name", sorted(C.cases()))
def test_every_gpu_input_set_tells_the_records_apart(name):
    """Power of the GPU inputs: per frame, the restatement with the frame's own record differs bitwise from the restatement with each
    other frame's record.  Frames without input (the empty sweep, the all-zero plane of the cloud) are empty under every record."""
    case = C.cases()[name]
    assert case.b >= 2 and len(case.empty) <= 1
    C.power(case)
    for f in case.empty:
        assert not case.want(f).any()
    for f in range(case.b):
        if f not in case.empty:
            assert case.want(f).size and np.asarray(case.want(f)).any(), (name, f)      # the expectation is not the empty result


@pytest.mark.parametrize("name, px", [("project straddle 5x7", 35), ("reproject 6x9 -> 5x7", 35), ("reproject 40x50 -> 33x41", 33 * 41)])
def test_the_straddling_threads_have_winners_on_both_sides(name, px):
    """With 4 pixels per thread a frame of px pixels (px % 4 != 0) ends inside a thread.  The first such thread holds winners in all
    of its pixels (pixels 32..35 of the 5x7 sets), and every such thread at least one on either side: the per-pixel choice of the record
    is exercised."""
    case = C.cases()[name]
    flat = np.concatenate([case.want(f).ravel() for f in range(case.b)])
    assert px % 4 != 0
    for k in range(1, case.b):
        t0 = px * k - px * k % 4
        hit = flat[t0:t0 + 4] != 0
        assert hit[:px * k - t0].any() and hit[px * k - t0:].any(), (name, k, hit)
        if k == 1 and px == 35:
            assert hit.all(), (name, hit)
    if name.startswith("project"):
        n = np.diff(case.offsets)
        assert all((case.want(f) != 0).sum() < n[f] for f in range(case.b)), "no last-writer collisions"


def test_the_sweep_case_has_the_boundaries_the_kernel_has_to_find():
    case = C.cases()["project sweeps 16x24"]
    assert case.offsets.tolist() == [0, 100, 100, 400, 437, 693, 694]             # boundaries inside workgroups 0, 1 and 2, one empty sweep
    n = np.diff(case.offsets)
    landed = [(case.want(f) != 0).sum() for f in range(case.b)]
    assert all(landed[f] > 0 for f in range(case.b) if n[f]) and landed[2] < n[2] and landed[4] < n[4]        # collisions in the tiny image
