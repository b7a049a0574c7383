"""Nearest-wins projection and reprojection (dcmt_project_points_nearest*, dcmt_reproject_depth_nearest*) without a GPU: the numpy
restatements of tests/nearest_restatement.py against their slow forms and against the last-wins restatements on the tiny inputs the
GPU tests use, the key map and the launch plans as stand-alone CPU programs, the ABI and the Python keyword."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nearest_restatement as R
from conftest import ROOT, assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

CSRC = os.path.join(ROOT, "depth_completion_mt_amd", "csrc")
f32 = np.float32
DEV = ("dcmt_project_points_nearest_dev", "dcmt_project_points_nearest_calib_dev", "dcmt_reproject_depth_nearest_dev",
       "dcmt_reproject_depth_nearest_calib_dev")
HOST = ("dcmt_project_points_nearest", "dcmt_reproject_depth_nearest")


# ---------------------------------------------------------------- the restatements
def test_order_map_of_the_restatement():
    v = np.array([-np.finfo(f32).max, -80.0, -1.0, -np.finfo(f32).tiny, -1e-45, -0.0, 0.0, 1e-45, np.finfo(f32).tiny, 1.0, 5.37, 80.0,
                  np.finfo(f32).max], f32)
    o = R.ord_of(v).astype(np.int64)
    assert (np.diff(o) > 0).all()
    assert np.array_equal(R.unord(R.ord_of(v)).view(np.uint32), v.view(np.uint32))
    k = R.key_of(v).astype(np.int64)
    assert (np.diff(k) < 0).all() and (k >= 0x00800000).all() and (k <= 0xFF7FFFFF).all()
    assert R.below(-0.0, 0.0) and not R.below(0.0, -0.0) and not R.below(0.0, 0.0) and R.below(-1.0, -0.0) and R.below(1.0, 2.0)


@pytest.mark.parametrize("rows,cols", R.PROJECT_SHAPES)
def test_projection_rules_on_the_tiny_inputs(rows, cols):
    inp = R.project_inputs(rows, cols)
    pts, off, recs = inp["points"], inp["offsets"], inp["records"]
    for name, Ts, Ps in (("uniform", *recs[0]), ("table", [r[0] for r in recs], [r[1] for r in recs])):
        near = R.project_batch(pts, off, Ts, Ps, rows, cols)
        assert_bit_equal(near, R.project_batch(pts, off, Ts, Ps, rows, cols, rule=R.nearest_of_loop), f"{name}: key form against the running minimum")
        last = R.project_last(pts, off, Ts, Ps, rows, cols)
        assert_bit_equal(last, R.project_batch(pts, off, Ts, Ps, rows, cols, rule=R.last_of), f"{name}: per-point landings against the last-wins restatement")
        assert not near[1].any() and not last[1].any()                                   # the empty sweep
        for f in (0, 2):
            occ, diff = R.compare_rules(near[f], last[f])
            flat, values = R.project_landings(pts[off[f]:off[f + 1]], Ts if name == "uniform" else Ts[f], Ps if name == "uniform" else Ps[f], rows, cols)
            print(f"{rows}x{cols} {name} sweep {f}: {len(flat)} of {off[f + 1] - off[f]} points land on {occ} of {rows * cols} pixels, the rules differ in {diff}")
            assert occ >= rows * cols // 2 and len(flat) >= 4 * occ
            assert 2 * diff >= occ, "the two rules coincide too often for a comparison to mean anything"
            assert (values < 0).any() and (near[f] < 0).any(), "no negative p.z lands"
            assert len(flat) < off[f + 1] - off[f], "nothing is rejected"


def reproject_records(src, dst, mat):
    return R.reproject_record(src, dst, mat), [R.reproject_record(src, dst, m, k) for k, m in enumerate((mat, "small", "shift"))]


@pytest.mark.parametrize("src,dst", R.REPROJECT_SHAPES)
@pytest.mark.parametrize("mat", list(R.REPROJECT_MATS))
def test_reprojection_rules_on_the_tiny_inputs(src, dst, mat):
    frames = R.reproject_inputs(src)
    one, table = reproject_records(src, dst, mat)
    for name, recs in (("uniform", one), ("table", table)):
        near = R.reproject_batch(frames, *dst, recs)
        assert_bit_equal(near, R.reproject_batch(frames, *dst, recs, rule=R.nearest_of_loop), f"{name}: key form against the running minimum")
        last = R.reproject_last(frames, *dst, recs)
        assert_bit_equal(last, R.reproject_batch(frames, *dst, recs, rule=R.last_of), f"{name}: landings against np_reproject")
        occ = diff = 0
        for f in range(3):
            o, d = R.compare_rules(near[f], last[f])
            occ, diff = occ + o, diff + d
        print(f"{src}->{dst} {mat} {name}: {occ} occupied pixels, the rules differ in {diff}")
        if mat == "behind" and name == "uniform":        # rotated by 65 degrees nothing stays in view: the all-zero result
            assert occ == 0
            continue
        assert occ >= dst[0] * dst[1] // 2
        assert 2 * diff >= occ, "the two rules coincide too often for a comparison to mean anything"


def test_bad_records_empty_their_frame_in_the_restatement():
    rows, cols = 5, 7
    inp = R.project_inputs(rows, cols)
    Ts, Ps = [r[0].copy() for r in inp["records"]], [r[1].copy() for r in inp["records"]]
    good = R.project_batch(inp["points"], inp["offsets"], Ts, Ps, rows, cols)
    Ps[2][1, 2] = np.nan
    bad = R.project_batch(inp["points"], inp["offsets"], Ts, Ps, rows, cols)
    assert good[2].any() and not bad[2].any()
    assert_bit_equal(bad[:2], good[:2], "the other frames")


# ---------------------------------------------------------------- the stand-alone programs
def build_and_run(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I" + CSRC, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_key_map(tmp_path):
    build_and_run(tmp_path, "key_map_test")


def test_key_map_under_the_host_sanitizers(tmp_path):
    build_and_run(tmp_path, "key_map_test", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def test_launch_plans_and_buffer_checks(tmp_path):
    build_and_run(tmp_path, "plan_nearest_test")


def test_key_header_agrees_with_the_restatement(tmp_path):
    """The header's key of a few values, printed by a three-line program, against R.key_of."""
    vals = np.array([-80.0, -0.0, 0.0, 1e-45, 1.0, 5.37, 85.0, 3.4e38], f32)
    src = tmp_path / "k.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "dcmt_depth_key.h"\n'
                   'int main(int n, char** a) { for (int i = 1; i < n; ++i) std::printf("%u\\n", dcmt::depth_key((uint32_t)std::strtoul(a[i], nullptr, 10))); }\n')
    exe = str(tmp_path / "k")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe] + [str(int(b)) for b in vals.view(np.uint32)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [int(k) for k in R.key_of(vals)]


# ---------------------------------------------------------------- ABI
def test_the_six_names_are_exported_and_declared():
    nm = subprocess.run(["nm", "-D", "--defined-only", L.build()], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "dcmt.h")).read()
    for name in DEV + HOST:
        assert name in L.EXPORTS and f" T {name}\n" in nm and getattr(L.lib(), name) is not None, name
        assert re.search(r"\bint " + name + r"\(", hdr), name
    assert L.lib().dcmt_version() == 120
    twins = ("dcmt_project_points_dev", "dcmt_project_points_calib_dev", "dcmt_reproject_depth_dev", "dcmt_reproject_depth_calib_dev",
             "dcmt_project_points", "dcmt_reproject_depth")
    assert tuple(L.nearest_name(t) for t in twins) == DEV + HOST
    for t in twins:
        assert getattr(L.lib(), L.nearest_name(t)).argtypes == getattr(L.lib(), t).argtypes
    shim = open(os.path.join(ROOT, "include", "img_completion.h")).read()
    assert "inline void unrectify_sol_nearest(const cv::Mat& depth, cv::Mat& depth_unrect, const float Minv[16])" in shim


def test_entry_points_reject_bad_arguments_without_gpu():
    """No context can exist here, so every call is refused before anything is looked at; what the calls refuse WITH a context --
    misaligned and overlapping buffers -- is plan_nearest_test.cpp above and, on a device, tests/test_gpu_nearest.py."""
    lib = L.lib()
    buf = np.zeros(8192, np.uint8)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16
    pts, off, out, tab = a, a + 2048, a + 4096, a + 6144
    T, P = (ctypes.c_float * 16)(), (ctypes.c_float * 12)()
    rp = api.make_reproject_params()
    for args in ((None, pts, off, 4, 1, T, P, out, 4, 4, None), (None, None, off, 4, 1, T, P, out, 4, 4, None), (None, pts, None, 4, 1, T, P, out, 4, 4, None),
                 (None, pts, off, 4, 1, None, P, out, 4, 4, None), (None, pts, off, 4, 1, T, None, out, 4, 4, None), (None, pts, off, 4, 1, T, P, None, 4, 4, None),
                 (None, pts + 4, off, 4, 1, T, P, out, 4, 4, None), (None, pts, off, 4, 1, T, P, pts + 16, 4, 4, None),
                 (None, pts, off, 4, 1, T, P, out, 1 << 20, 1 << 20, None), (None, pts, off, 4, 70000, T, P, out, 4, 4, None)):
        assert lib.dcmt_project_points_nearest_dev(*args) == L.E_INVALID, args
    for args in ((None, pts, off, 4, 1, tab, out, 4, 4, None), (None, pts, off, 4, 1, None, out, 4, 4, None), (None, pts, off, 4, 1, tab + 8, out, 4, 4, None),
                 (None, pts, off, 4, 1, tab, tab, 4, 4, None)):
        assert lib.dcmt_project_points_nearest_calib_dev(*args) == L.E_INVALID, args
    for args in ((None, pts, 4, 4, 1, ctypes.byref(rp), out, 4, 4, None), (None, None, 4, 4, 1, ctypes.byref(rp), out, 4, 4, None),
                 (None, pts, 4, 4, 1, None, out, 4, 4, None), (None, pts, 4, 4, 1, ctypes.byref(rp), None, 4, 4, None),
                 (None, pts, 4, 4, 1, ctypes.byref(rp), pts + 8, 4, 4, None), (None, pts, 1 << 20, 1 << 20, 70000, ctypes.byref(rp), out, 4, 4, None)):
        assert lib.dcmt_reproject_depth_nearest_dev(*args) == L.E_INVALID, args
    for args in ((None, pts, 4, 4, 1, tab, out, 4, 4, None), (None, pts, 4, 4, 1, None, out, 4, 4, None), (None, pts, 4, 4, 1, tab, tab, 4, 4, None)):
        assert lib.dcmt_reproject_depth_nearest_calib_dev(*args) == L.E_INVALID, args
    assert lib.dcmt_project_points_nearest(None, pts, 4, T, P, out, 16, 4, 4) == L.E_INVALID
    assert lib.dcmt_reproject_depth_nearest(None, pts, 16, 4, 4, ctypes.byref(rp), out, 16, 4, 4) == L.E_INVALID
    assert not buf.any()


# ---------------------------------------------------------------- Python
class FakeTensor:
    """What the wrappers look at in a CUDA tensor, without a device."""
    is_cuda, device = True, "cuda:0"

    def __init__(self, shape, dtype, itemsize=4):
        self.shape, self.dtype, self.itemsize = tuple(shape), dtype, itemsize

    def is_contiguous(self):
        return True

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))

    def element_size(self):
        return self.itemsize

    def data_ptr(self):
        return 4096


class Recorder:
    """Stands in for the loaded library: every function records its name and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return L.OK
        return fn


def test_the_nearest_keyword_reaches_the_right_symbol(monkeypatch):
    import inspect
    import torch
    for name in ("project_points_dev", "project_points_calib_dev", "reproject_depth_dev", "reproject_depth_calib_dev", "reproject_depth"):
        p = inspect.signature(getattr(api.Context, name)).parameters["nearest"]
        assert p.default is False, name
    assert inspect.signature(api.unrectify_sol).parameters["nearest"].default is False
    rec = Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    ctx = api.Context.__new__(api.Context)
    ctx._h = ctypes.c_void_p()
    pts, off = FakeTensor((10, 4), torch.float32), FakeTensor((3,), torch.int32)
    sparse, depth, out = FakeTensor((2, 4, 5), torch.float32), FakeTensor((2, 6, 7), torch.float32), FakeTensor((2, 4, 5), torch.float32)
    ptab, rtab = FakeTensor((2, 96), torch.uint8, 1), FakeTensor((2, 136), torch.uint8, 1)
    T, P = np.eye(4, dtype=f32), np.eye(3, 4, dtype=f32)
    frame = np.ones((6, 7), f32)
    want = []
    for nearest, tag in ((False, ""), (True, "_nearest")):
        kw = {"nearest": True} if nearest else {}
        ctx.project_points_dev(pts, off, T, P, 4, 5, sparse, stream=0, **kw)
        ctx.project_points_calib_dev(pts, off, ptab, 4, 5, sparse, stream=0, **kw)
        ctx.reproject_depth_dev(depth, 4, 5, None, out, stream=0, **kw)
        ctx.reproject_depth_calib_dev(depth, 4, 5, rtab, out, stream=0, **kw)
        ctx.reproject_depth(frame, 4, 5, **kw)
        want += [f"dcmt_project_points{tag}_dev", f"dcmt_project_points{tag}_calib_dev", f"dcmt_reproject_depth{tag}_dev",
                 f"dcmt_reproject_depth{tag}_calib_dev", f"dcmt_reproject_depth{tag}"]
    assert [c for c in rec.calls if not c.startswith("dcmt_default_")] == want
    # unrectify_sol hands the keyword to Context.reproject_depth
    seen = []
    monkeypatch.setattr(api, "_ctx_for", lambda *a, **k: ctx)
    monkeypatch.setattr(api.Context, "reproject_depth", lambda self, a, r, c, p, nearest=False: seen.append(nearest) or np.zeros((r, c), f32))
    api.unrectify_sol(frame, (4, 5), np.eye(4))
    api.unrectify_sol(frame, (4, 5), np.eye(4), nearest=True)
    assert seen == [False, True]
    ctx._h = ctypes.c_void_p()
