"""JET colourisation of depth planes (dcmt_colorize*, dcmt_colormap_jet, api.Context.colorize_dev / colorize, to_color_image,
dcmt_shim::to_color_image): the reference mains' toColorImage (DC_lidar_only/main.cpp:6-14)
    cv::normalize(r_img, n, 1.0, 0, NORM_MINMAX);  n.convertTo(u8, CV_8UC1, 255.0);  cv::applyColorMap(u8, out, COLORMAP_JET).
Expected bytes come from the numpy restatement below: the recorded palette tests/golden/jet_lut.json, the f64 -> f32 coefficient
steps of include/dcmt.h and the f32 operations one rounding at a time."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT, assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

with open(os.path.join(GOLDEN_DIR, "jet_lut.json")) as _f:
    LUT = np.array(json.load(_f)["bgr"], dtype=np.uint8)          # [256][B, G, R]
DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "color_test.cpp")
f32 = np.float32


# ---------------------------------------------------------------- numpy restatement
def np_coef(frame):
    """cv::normalize(.., 1.0, 0, NORM_MINMAX) into CV_32F: (scale, shift) as f32, computed in f64 and rounded as OpenCV does."""
    x = np.asarray(frame, dtype=f32)
    smin, smax = float(x.min()), float(x.max())
    d = smax - smin
    scale = (1.0 - 0.0) * (1.0 / d if d > np.finfo(np.float64).eps else 0.0)
    scale = float(f32(scale))
    shift = float(f32(0.0)) - float(f32(smin * scale))
    return f32(scale), f32(shift)


def np_index(frame, fma=False):
    """Palette index per pixel.  fma=False: v = x * scale + shift in two f32 roundings (what the library does); fma=True: one
    rounding of the exact x * scale (f64 holds it) plus shift, the form an AVX2 OpenCV build takes."""
    x = np.asarray(frame, dtype=f32)
    s, h = np_coef(x)
    if fma:
        v = (x.astype(np.float64) * float(s) + float(h)).astype(f32)
    else:
        v = x * s + h
    t = v * f32(255.0)
    return np.clip(np.rint(t), 0, 255).astype(np.intp)       # saturate_cast<uchar>(float): round half to even, saturate


def np_colorize(frame):
    return LUT[np_index(frame)]


def frames_for(b, rows, cols, seed):
    """Per frame a different kind of content: sparse depth (zeros in it), the same with no zero (shift != 0), negative values,
    a constant frame, a narrow and a wide range -- neighbours in a batch have very different extrema."""
    base = synth.synth_batch(b, rows, cols, seed)
    rng = np.random.default_rng(seed)
    out = np.empty_like(base)
    for i in range(b):
        k = i % 6
        if k == 0:
            out[i] = base[i]
        elif k == 1:
            out[i] = base[i] + f32(0.37)
        elif k == 2:
            out[i] = base[i] * f32(3.0) - f32(40.0)
        elif k == 3:
            out[i] = f32(7.25)
        elif k == 4:
            out[i] = f32(50.0) + (rng.random((rows, cols)) * 1e-3).astype(f32)
        else:
            out[i] = base[i] * f32(1e4) + f32(1.0)
    return out


# ---------------------------------------------------------------- CPU
def test_colormap_jet_equals_the_recorded_fixture():
    buf = (ctypes.c_uint8 * 768)()
    L.lib().dcmt_colormap_jet(buf)
    assert bytes(buf) == LUT.tobytes()
    assert LUT.shape == (256, 3) and LUT[0].tolist() == [128, 0, 0] and LUT[255].tolist() == [0, 0, 128]   # B, G, R
    assert api.JET_BGR.shape == (256, 3) and api.JET_BGR.dtype == np.uint8 and np.array_equal(api.JET_BGR, LUT)
    assert not api.JET_BGR.flags.writeable
    import depth_completion_mt_amd as pkg
    assert pkg.JET_BGR is api.JET_BGR


def test_colorize_entry_points_reject_bad_arguments_without_gpu():
    for name in ("dcmt_colorize_dev", "dcmt_colorize", "dcmt_colormap_jet"):
        assert name in L.EXPORTS and getattr(L.lib(), name) is not None
    lib = L.lib()
    src = (ctypes.c_float * 16)()
    out = (ctypes.c_uint8 * 48)()
    assert lib.dcmt_colorize_dev(None, src, 4, 4, 1, out, None) == L.E_INVALID
    assert lib.dcmt_colorize_dev(None, None, 4, 4, 1, None, None) == L.E_INVALID
    assert lib.dcmt_colorize_dev(None, src, 1 << 20, 1 << 20, 70000, out, None) == L.E_INVALID
    assert lib.dcmt_colorize(None, src, 16, 4, 4, out, 12) == L.E_INVALID
    assert lib.dcmt_colorize(None, None, 16, 4, 4, None, 12) == L.E_INVALID
    assert lib.dcmt_colorize(None, src, 16, 1 << 20, 1 << 20, out, 3 << 20) == L.E_INVALID
    lib.dcmt_colormap_jet(None)                                    # ignored, no crash


def test_shim_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "tests", "mock_opencv"), "-c", DRIVER, "-o", str(tmp_path / "color_test.o")],
                   check=True, capture_output=True)


def test_restatement_extremes_constant_frames_and_the_fma_form():
    rng = np.random.default_rng(3)
    for k in range(40):
        x = (rng.standard_normal((37, 53)) * 10.0 ** rng.integers(-3, 5)).astype(f32)
        if k % 2:
            x[rng.random(x.shape) < 0.3] = 0
        if k % 3 == 0:
            x = np.abs(x) + f32(1.5)                               # no zero pixel: shift != 0
        idx = np_index(x)
        assert (idx[x == x.min()] == 0).all() and (idx[x == x.max()] == 255).all(), k
        c = np_colorize(x)
        assert (c[x == x.min()] == LUT[0]).all() and (c[x == x.max()] == LUT[255]).all()
        fm = np_index(x, fma=True)
        assert np.abs(fm - idx).max() <= 1, k                      # the FMA form moves a pixel by one index at most
        if (x == 0).any() and x.min() == 0:
            assert np.array_equal(fm, idx), k                      # shift == 0: both forms are one rounding of x * scale
    for v in (0.0, -3.5, 7.25, 1e30):
        x = np.full((5, 9), v, dtype=f32)
        assert np_coef(x)[0] == 0 and (np_colorize(x) == LUT[0]).all()
    # a two-valued frame: exactly entries 0 and 255
    x = np.array([[2.0, 5.0, 2.0]], dtype=f32)
    assert np_index(x).tolist() == [[0, 255, 0]]


# ---------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, 375, 1242, 17)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_frames(got, frames, what):
    assert got.shape == frames.shape + (3,) and got.dtype == np.uint8, (what, got.shape, got.dtype)
    for i in range(frames.shape[0]):
        want = np_colorize(frames[i])
        if not np.array_equal(got[i], want):
            bad = np.argwhere((got[i] != want).any(-1))
            raise AssertionError(f"{what} frame {i}: {len(bad)} pixels differ, first at {tuple(bad[0])}: "
                                 f"{got[i][tuple(bad[0])]} vs {want[tuple(bad[0])]}")


@gpu
def test_bit_exact_against_the_restatement(ctx):
    for rows, cols in ((352, 1216), (375, 1242)):
        for b, seed in ((1, 10), (3, 11), (17, 12)):
            frames = frames_for(b, rows, cols, seed)
            if b == 1:
                frames[0] += f32(0.5)                              # the single frame without a zero
            got = ctx.colorize_dev(dev(frames)).cpu().numpy()
            check_frames(got, frames, f"{rows}x{cols} batch {b}")
            two = ctx.colorize_dev(dev(frames[0])).cpu().numpy()   # a [rows][cols] tensor -> [rows][cols][3]
            assert two.shape == (rows, cols, 3) and np.array_equal(two, got[0])


@gpu
def test_tiny_shapes(ctx):
    rng = np.random.default_rng(5)
    for rows, cols in ((1, 1), (1, 5), (7, 3), (1, 3), (3, 1), (2, 2), (5, 7), (1, 1242), (375, 1)):
        for b in (1, 3, 17):
            frames = (rng.standard_normal((b, rows, cols)) * 20.0).astype(f32)
            frames[rng.random(frames.shape) < 0.25] = 0
            frames[::4] = f32(3.0)                                # constant frames among them
            got = ctx.colorize_dev(dev(frames)).cpu().numpy()
            check_frames(got, frames, f"{rows}x{cols} batch {b}")


@gpu
def test_frame_bytes_do_not_depend_on_batch_position_or_alignment(ctx):
    import torch
    rows, cols = 375, 1242                                        # rows * cols % 4 == 2: groups straddle frames
    n = rows * cols
    frames = frames_for(7, rows, cols, 20)
    d = dev(frames)
    full = ctx.colorize_dev(d).cpu().numpy()
    check_frames(full, frames, "batch 7")
    assert np.array_equal(ctx.colorize_dev(d).cpu().numpy(), full)
    flat_src = torch.zeros(7 * n + 8, dtype=torch.float32, device="cuda")
    flat_out = torch.zeros(3 * 7 * n + 16, dtype=torch.uint8, device="cuda")
    for i in range(7):
        assert np.array_equal(ctx.colorize_dev(d[i]).cpu().numpy(), full[i]), f"frame {i} alone"
        for pos in (1, 2):
            order = [(i + 1) % 7, (i + 3) % 7]
            order.insert(pos, i)
            three = ctx.colorize_dev(d[order].contiguous()).cpu().numpy()
            assert np.array_equal(three[pos], full[i]), f"frame {i} at position {pos} of 3"
    # source at an element offset (4-byte aligned only), output at odd byte offsets: the narrow form of the map kernel
    for soff, ooff in ((1, 0), (0, 1), (3, 5)):
        s = flat_src[soff:soff + 3 * n].view(3, rows, cols)
        s.copy_(d[2:5])
        o = flat_out[ooff:ooff + 3 * 3 * n].view(3, rows, cols, 3)
        ctx.colorize_dev(s, d_bgr=o)
        assert np.array_equal(o.cpu().numpy(), full[2:5]), (soff, ooff)


@gpu
def test_guard_bytes_and_source_untouched(ctx):
    import torch
    for rows, cols, b in ((375, 1242, 17), (7, 3, 17), (1, 5, 3), (352, 1216, 2)):
        frames = frames_for(b, rows, cols, 30)
        nb = 3 * b * rows * cols
        d = dev(frames)
        for off in (0, 1):
            buf = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
            o = buf[off:off + nb].view(b, rows, cols, 3)
            ctx.colorize_dev(d, d_bgr=o)
            h = buf.cpu().numpy()
            assert (h[:off] == 0xA5).all() and (h[off + nb:] == 0xA5).all(), (rows, cols, b, off)
            check_frames(h[off:off + nb].reshape(b, rows, cols, 3), frames, f"{rows}x{cols} batch {b} offset {off}")
        assert_bit_equal(d.cpu().numpy(), frames, "source after colourisation")


@gpu
def test_argument_checks_on_a_live_context(ctx):
    import torch
    lib = L.lib()
    src = torch.zeros((2, 8, 8), dtype=torch.float32, device="cuda")
    out = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    args = dict(s=src.data_ptr(), r=8, c=8, b=2, o=out.data_ptr())
    call = lambda **kw: lib.dcmt_colorize_dev(ctx._h, *[dict(args, **kw)[k] for k in "srcbo"], None)
    assert call() == L.OK
    for bad in (dict(s=None), dict(o=None), dict(b=18), dict(b=0), dict(r=376), dict(c=1243), dict(c=0), dict(s=src.data_ptr() + 2)):
        assert call(**bad) == L.E_INVALID, bad
    h = np.zeros((8, 8), f32)
    hb = np.zeros((8, 8, 3), np.uint8)
    assert lib.dcmt_colorize(ctx._h, h.ctypes.data, 32, 8, 8, hb.ctypes.data, 24) == L.OK
    assert lib.dcmt_colorize(ctx._h, h.ctypes.data, 28, 8, 8, hb.ctypes.data, 24) == L.E_INVALID
    assert lib.dcmt_colorize(ctx._h, h.ctypes.data, 32, 8, 8, hb.ctypes.data, 23) == L.E_INVALID
    torch.cuda.synchronize()


@gpu
def test_chained_behind_a_completion_and_the_normalised_path_keeps_its_bits():
    from oracle import oracle as O
    import torch
    frames = synth.synth_batch(16, 352, 1216, 40)
    norm = api.make_params(normalize=(0, 80))
    with api.Context(0, 352, 1216, 16) as c:
        d = dev(frames)
        n1 = c.complete_dev(d, params=norm)
        torch.cuda.synchronize()
        n1 = n1.cpu().numpy()
        dense = c.complete_dev(d)
        col = c.colorize_dev(dense)                              # same stream, no synchronisation in between
        n2 = c.complete_dev(d, params=norm)                      # a normalised completion behind the colourisation
        torch.cuda.synchronize()
        dense, col, n2 = dense.cpu().numpy(), col.cpu().numpy(), n2.cpu().numpy()
    assert np.array_equal(n1.view(np.uint32), n2.view(np.uint32))
    for i in (0, 7, 15):
        want = O.img_completion(frames[i])
        assert_bit_equal(dense[i], want, f"completion frame {i}")
        assert np.array_equal(col[i], np_colorize(want)), f"colourised completion frame {i}"
        assert_bit_equal(n2[i], O.img_completion(O.normalize_minmax(frames[i], 0, 80)), f"normalised completion frame {i}")


@gpu
def test_host_entry_python_and_cpp_shim_equal_the_device_call(ctx, tmp_path):
    import torch
    rows, cols = 375, 1242
    frames = frames_for(2, rows, cols, 50)                        # one with zeros, one without
    want = ctx.colorize_dev(dev(frames)).cpu().numpy()
    check_frames(want, frames, "device")
    exe = tmp_path / "color_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv"),
                    DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, capture_output=True)
    for i in range(2):
        wide = np.full((rows, cols + 37), -9.0, f32)
        wide[:, :cols] = frames[i]
        assert np.array_equal(ctx.colorize(wide[:, :cols]), want[i]), f"dcmt_colorize frame {i}"
        assert np.array_equal(api.to_color_image(frames[i]), want[i]), f"to_color_image(numpy) frame {i}"
        t = api.to_color_image(dev(frames[i]))
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), want[i]), f"to_color_image(cuda) frame {i}"
        frames[i].tofile(tmp_path / "in.f32")
        r = subprocess.run([str(exe), str(rows), str(cols), str(tmp_path / "in.f32"), str(tmp_path / "out.u8")],
                           capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        got = np.fromfile(tmp_path / "out.u8", dtype=np.uint8).reshape(rows, cols, 3)
        assert np.array_equal(got, want[i]), f"dcmt_shim::to_color_image frame {i}"
    torch.cuda.synchronize()
