"""The ragged-batch crop and the uint16 export (dcmt_crop_frames_dev, dcmt_depth_to_u16*, make_crop_table, kitti_crop_origin,
pack_ragged, plan_crop, plan_depth_to_u16): everything that needs no GPU.  Both are restated in numpy in tests/crop_restatement.py;
the pins below were computed once, on a CPU.  The GPU side is tests/test_gpu_crop_export.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import crop_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

CSRC = os.path.join(ROOT, "depth_completion_mt_amd", "csrc")
NEW = ("dcmt_crop_frames_dev", "dcmt_depth_to_u16_dev", "dcmt_depth_to_u16")


def test_entry_points_are_exported_and_reject_bad_arguments_without_gpu():
    nm = subprocess.run(["nm", "-D", "--defined-only", L.build()], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name in L.EXPORTS and f" T {name}\n" in nm, name
    lib = L.lib()
    assert lib.dcmt_version() == 120
    buf = np.zeros(4096, np.uint8)
    a = buf.ctypes.data
    src, table, dst = a, a + 1024, a + 2048
    # no context: nothing is looked at, nothing is written (the checks on the buffers themselves: tests/plan_crop_test.cpp)
    assert lib.dcmt_crop_frames_dev(None, src, 1024, table, 2, dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_crop_frames_dev(None, None, 1024, table, 2, dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_crop_frames_dev(None, src, 1024, None, 2, dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_crop_frames_dev(None, src, 1024, table, 2, None, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_crop_frames_dev(None, src, 0, table, 2, dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_crop_frames_dev(None, src, 1024, table, 0, dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_crop_frames_dev(None, src, 1024, table, 5, dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_crop_frames_dev(None, src, 1024, table + 4, 2, dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_crop_frames_dev(None, src, 1024, table, 2, src + 8, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_crop_frames_dev(None, src, 1024, table, 2, dst, 1 << 20, 1 << 20, 70000, None) == L.E_INVALID
    f32 = ctypes.c_float
    assert lib.dcmt_depth_to_u16_dev(None, src, f32(256.0), dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_depth_to_u16_dev(None, None, f32(256.0), dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_depth_to_u16_dev(None, src, f32(256.0), None, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_depth_to_u16_dev(None, src, f32(0.0), dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_depth_to_u16_dev(None, src, f32(-1.0), dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_depth_to_u16_dev(None, src, f32(float("inf")), dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_depth_to_u16_dev(None, src, f32(float("nan")), dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_depth_to_u16_dev(None, src + 2, f32(256.0), dst, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_depth_to_u16_dev(None, src, f32(256.0), dst + 1, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_depth_to_u16_dev(None, src, f32(256.0), src + 8, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_depth_to_u16(None, src, 16, f32(256.0), dst, 8, 4, 4) == L.E_INVALID
    assert lib.dcmt_depth_to_u16(None, None, 16, f32(256.0), dst, 8, 4, 4) == L.E_INVALID
    assert lib.dcmt_depth_to_u16(None, src, 16, f32(256.0), None, 8, 4, 4) == L.E_INVALID
    assert not buf.any()


def test_crop_record_layout():
    assert ctypes.sizeof(L.CropSrc) == 32
    offs = {n: getattr(L.CropSrc, n).offset for n, _ in L.CropSrc._fields_}
    assert offs == {"offset": 0, "row_stride": 8, "rows": 12, "cols": 16, "x0": 20, "y0": 24, "reserved": 28}
    d = api.CROP_SRC_DTYPE
    assert d.itemsize == 32 and {n: d.fields[n][1] for n in d.names} == offs
    assert [d.fields[n][0].str for n in d.names] == ["<u8", "<u4", "<i4", "<i4", "<i4", "<i4", "<u4"]


def test_kitti_crop_origin():
    assert [api.kitti_crop_origin(r, c) for r, c in R.KITTI_SIZES] == [(23, 13), (18, 4), (22, 11), (18, 5), (24, 12)] == R.KITTI_ORIGINS
    assert api.kitti_crop_origin(352, 1216) == (0, 0)
    assert api.kitti_crop_origin(100, 60, 10, 21) == (90, 19)
    for (r, c), (y0, x0) in zip(R.KITTI_SIZES, R.KITTI_ORIGINS):        # bottom rows, centred with the odd column on the right
        assert y0 + 352 == r and 0 <= (c - 1216 - x0) - x0 <= 1


def test_pack_ragged_and_the_table_defaults():
    frames = [R.noise(s, np.uint16, 3 + i) for i, s in enumerate([(5, 7), (4, 9), (6, 6)])]
    flat, shapes, offsets = api.pack_ragged(frames)
    assert flat.dtype == np.uint8 and flat.size == 2 * (35 + 36 + 36) and shapes == [(5, 7), (4, 9), (6, 6)] and offsets == [0, 70, 142]
    for f, o in zip(frames, offsets):
        assert flat[o:o + f.nbytes].tobytes() == f.tobytes()
    t = api.make_crop_table(shapes, (3, 4), 2)
    assert t.dtype == api.CROP_SRC_DTYPE and t["offset"].tolist() == offsets and t["row_stride"].tolist() == [14, 18, 12]
    assert t["rows"].tolist() == [5, 4, 6] and t["cols"].tolist() == [7, 9, 6] and not t["reserved"].any()
    assert list(zip(t["y0"].tolist(), t["x0"].tolist())) == [(2, 1), (1, 2), (3, 1)]
    got = R.crop_frames(flat, t, 2, 3, 4).view(np.uint16)
    for f, (y0, x0) in enumerate([(2, 1), (1, 2), (3, 1)]):
        assert np.array_equal(got[f], frames[f][y0:y0 + 3, x0:x0 + 4])
    bgr = [R.noise(s + (3,), np.uint8, 9 + i) for i, s in enumerate([(5, 7), (4, 9)])]
    flat, shapes, offsets = api.pack_ragged(bgr)
    assert shapes == [(5, 7), (4, 9)] and offsets == [0, 105]
    got = R.crop_frames(flat, api.make_crop_table(shapes, (2, 3), 3, origins=[(0, 4), (2, 0)]), 3, 2, 3).reshape(2, 2, 3, 3)
    assert np.array_equal(got[0], bgr[0][0:2, 4:7]) and np.array_equal(got[1], bgr[1][2:4, 0:3])
    # explicit offsets, pitches and a source size
    t = api.make_crop_table([(5, 7)], (5, 7), 2, offsets=[3], row_strides=[20], origins=[(0, 0)], src_bytes=3 + 4 * 20 + 14)
    assert t[0].tolist() == (3, 20, 5, 7, 0, 0, 0)


def test_make_crop_table_refuses_what_the_device_would_zero():
    ok = dict(shapes=[(10, 20)], out_shape=(4, 8), elem_bytes=2, origins=[(3, 5)])
    assert R.record_ok(api.make_crop_table(**ok)[0], 2, 4, 8, 400)
    bad = [dict(origins=[(3, 13)]), dict(origins=[(7, 5)]), dict(origins=[(-1, 5)]), dict(origins=[(3, -1)]), dict(shapes=[(0, 20)]),
           dict(shapes=[(10, 0)]), dict(row_strides=[39]), dict(src_bytes=399), dict(offsets=[1], src_bytes=400), dict(elem_bytes=5),
           dict(elem_bytes=0), dict(out_shape=(0, 8)), dict(offsets=[-1]), dict(row_strides=[1 << 32]), dict(offsets=[0, 0])]
    for change in bad:
        with pytest.raises(ValueError):
            api.make_crop_table(**{**ok, **change})
    api.make_crop_table(**{**ok, "src_bytes": 400})
    api.make_crop_table(**{**ok, "origins": [(6, 12)]})                 # touching the bottom and the right border


def test_restatement_of_the_record_test():
    rec = np.zeros(1, api.CROP_SRC_DTYPE)
    rec[0] = (0, 40, 10, 20, 5, 3, 0)
    assert R.record_ok(rec[0], 2, 4, 8, 400) and not R.record_ok(rec[0], 2, 4, 8, 399)
    for field, value in (("x0", 13), ("y0", 7), ("x0", -1), ("y0", -1), ("rows", 0), ("cols", 0), ("row_stride", 39), ("offset", 1),
                         ("offset", (1 << 64) - 1), ("x0", 0x7fffffff)):
        r = rec.copy()
        r[0][field] = value
        assert not R.record_ok(r[0], 2, 4, 8, 400), (field, value)
    assert not R.crop_frames(np.ones(400, np.uint8), r, 2, 4, 8).any()


def test_restatement_of_the_export():
    v = np.arange(65536, dtype=np.uint32)
    x = v.astype(np.float32) * np.float32(1.0 / 256.0)
    assert x.dtype == np.float32 and np.array_equal(R.depth_to_u16(x, 256.0), v.astype(np.uint16))
    got = R.depth_to_u16(np.array(R.EXPORT_PROBES, np.float32), 256.0)
    assert got.dtype == np.uint16 and got.tolist() == [0, 0, 0, 2, 2, 65535, 65535, 65535, 0] == R.EXPORT_WANT
    assert R.depth_to_u16(np.float32([3.4e38]), 256.0).tolist() == [65535]           # the product overflows to +Inf
    assert R.depth_to_u16(np.float32([65534.5, 65534.49, 65535.5]), 1.0).tolist() == [65534, 65534, 65535]
    assert np.float32(65535.0).view(np.uint32) == 0x477FFF00                          # the kernel's saturation bound, as bits


def test_cutting_records_and_plans(tmp_path):
    exe = str(tmp_path / "plan_crop_test")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + CSRC, os.path.join(ROOT, "tests", "plan_crop_test.cpp"),
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def test_python_layer_exports_the_new_functions():
    import depth_completion_mt_amd as pkg
    for name in ("depth_to_u16", "kitti_crop_origin", "make_crop_table", "pack_ragged"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(api, name)
    assert callable(api.Context.crop_frames_dev) and callable(api.Context.depth_to_u16_dev) and callable(api.Context.depth_to_u16)
