"""dcmt_bgr_convert_dev / dcmt_bgr_convert on the GPU (api.Context.bgr_convert_dev / bgr_convert, bgr_to_lab, bgr_to_gray, the
shim's bgr_to_lab / bgr_to_gray): every case bit-exact against the numpy restatement of tests/bgr_restatement.py.  What needs no
GPU is in tests/test_bgr_convert.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bgr_restatement as R
from conftest import ROOT, assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "bgr_test.cpp")
SHA_CUBE_LAB = "2f00e5b9a30983704f83a0a5aa4e39f5f5794b8e2ba161e8218a53f92ffddcf3"
SHA_CUBE_GRAY = "6d4f6d7f4301c52d2672db66451b4a06a5502bef956dd81b577660f956f410ae"
MODES = ((True, False), (False, True), (True, True))            # (lab, gray)


def _plan_constant(name):
    with open(os.path.join(ROOT, "depth_completion_mt_amd", "csrc", "dcmt_tiles.h")) as f:
        return int(re.search(r"constexpr \w+ " + name + r" = (\d+)u?;", f.read()).group(1))


PX_PER_PASS = 4 * _plan_constant("kBgrGroupsPerLane") * _plan_constant("kBgrThreads")    # kBgrPxPerPass: a workgroup's share in a small run
MAX_COLS = PX_PER_PASS + 1


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, 375, MAX_COLS, 3)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def image(b, rows, cols, seed):
    """A batch of B, G, R frames: uniform noise, so that every table entry is as likely as any other, over a smooth ramp in the
    first frame (equal neighbours: the lookups that broadcast)."""
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, (b, rows, cols, 3), dtype=np.uint8)
    img[0, :, : cols // 2] = (np.arange(rows)[:, None, None] * 3 + np.arange(cols // 2)[None, :, None] // 4 + np.array([0, 40, 90])) % 256
    return img


def check(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape, got.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


def convert_and_check(c, img, lab, gray, what):
    out = c.bgr_convert_dev(dev(img), lab=lab, gray=gray)
    o_lab, o_gray = out if lab and gray else (out, None) if lab else (None, out)
    if lab:
        check(o_lab.cpu().numpy(), R.bgr_to_lab(img), what + " Lab")
    if gray:
        check(o_gray.cpu().numpy(), R.bgr_to_gray(img), what + " grey")


def test_whole_colour_cube():
    """Every colour once: every table entry that can be reached, every arithmetic path.  16 frames of 1024 x 1024 holding pixel
    k = B | G << 8 | R << 16; Lab and grey from one call."""
    cube = R.cube_reference()
    img = R.colour_cube().reshape(16, 1024, 1024, 3)
    with api.Context(0, 1024, 1024, 16) as c:
        lab, gray = c.bgr_convert_dev(dev(img), lab=True, gray=True)
        lab, gray = lab.cpu().numpy(), gray.cpu().numpy()
    check(lab.reshape(-1, 3), cube["lab"], "cube Lab")
    check(gray.reshape(-1), cube["gray"], "cube grey")
    assert R.sha256(lab) == SHA_CUBE_LAB and R.sha256(gray) == SHA_CUBE_GRAY


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 3), (3, 5), (7, 9), (375, 1242), (352, 1216), (1, PX_PER_PASS - 1), (1, PX_PER_PASS + 1),
                                        (1, PX_PER_PASS)])
def test_shapes_where_the_indexing_can_go_wrong(ctx, rows, cols):
    """Tiny frames, 375 x 1242 (an odd pixel count: groups of 4 straddle frames), the KITTI crop, and frames one pixel short of, at
    and one pixel past a workgroup's share; batch 1 and 3; Lab only, grey only, both."""
    for b in (1, 3):
        img = image(b, rows, cols, 100 * b + rows)
        for lab, gray in MODES:
            convert_and_check(ctx, img, lab, gray, f"{rows}x{cols} batch {b}")
        one = ctx.bgr_convert_dev(dev(img[0]), lab=True)                            # a [rows][cols][3] tensor: a batch of one
        assert tuple(one.shape) == (rows, cols, 3)
        check(one.cpu().numpy(), R.bgr_to_lab(img[0]), f"{rows}x{cols} single frame")


def test_every_alignment_of_every_buffer(ctx):
    """Each of d_bgr, d_lab, d_gray at byte offsets 0..3 inside a larger allocation: the outputs equal those of the aligned call and
    the 64 guard bytes either side of each output keep their fill value."""
    import torch
    rows, cols, b = 7, 701, 3                                                      # 14721 pixels: three full passes and a partial one
    n = b * rows * cols
    img = image(b, rows, cols, 7)
    want_lab, want_gray = R.bgr_to_lab(img), R.bgr_to_gray(img)
    src = torch.zeros(3 * n + 8, dtype=torch.uint8, device="cuda")
    flat = dev(img.reshape(-1))
    for ob in range(4):
        s = src[ob:ob + 3 * n]
        s.copy_(flat)
        for ol in range(4):
            for og in range(4):
                lab_buf = torch.full((3 * n + 136,), 0xA5, dtype=torch.uint8, device="cuda")
                gray_buf = torch.full((n + 136,), 0x5A, dtype=torch.uint8, device="cuda")
                o_lab, o_gray = lab_buf[64 + ol:64 + ol + 3 * n], gray_buf[64 + og:64 + og + n]
                assert (s.data_ptr() % 4, o_lab.data_ptr() % 4, o_gray.data_ptr() % 4) == (ob, ol, og)
                ctx.bgr_convert_dev(s.view(b, rows, cols, 3), d_lab=o_lab.view(b, rows, cols, 3), d_gray=o_gray.view(b, rows, cols))
                hl, hg = lab_buf.cpu().numpy(), gray_buf.cpu().numpy()
                what = f"offsets bgr {ob} lab {ol} grey {og}"
                assert (hl[:64 + ol] == 0xA5).all() and (hl[64 + ol + 3 * n:] == 0xA5).all(), what
                assert (hg[:64 + og] == 0x5A).all() and (hg[64 + og + n:] == 0x5A).all(), what
                check(hl[64 + ol:64 + ol + 3 * n].reshape(img.shape), want_lab, what + " Lab")
                check(hg[64 + og:64 + og + n].reshape(img.shape[:-1]), want_gray, what + " grey")
        # one output alone at this source offset (the other pointer NULL takes no part in the choice)
        for lab, gray in MODES[:2]:
            out = ctx.bgr_convert_dev(s.view(b, rows, cols, 3), lab=lab, gray=gray).cpu().numpy()
            check(out, want_lab if lab else want_gray, f"source offset {ob} single output")
        check(s.cpu().numpy().reshape(img.shape), img, "source after the calls")


def test_in_place(ctx):
    import torch
    lib = L.lib()
    for b, rows, cols in ((1, 7, 9), (1, 352, 1216), (3, 352, 1216), (3, 375, 1242)):     # up to 342 workgroups
        img = image(b, rows, cols, 31 + b)
        want_lab, want_gray = R.bgr_to_lab(img), R.bgr_to_gray(img)
        for off in (0, 1):                                                         # the wide and the per-pixel form
            buf = torch.zeros(img.size + 8, dtype=torch.uint8, device="cuda")
            d = buf[off:off + img.size].view(img.shape)
            d.copy_(dev(img))
            got = ctx.bgr_convert_dev(d, d_lab=d)
            assert got.data_ptr() == d.data_ptr()
            check(d.cpu().numpy(), want_lab, f"in place {rows}x{cols} batch {b} offset {off}")
            d.copy_(dev(img))
            _, g = ctx.bgr_convert_dev(d, d_lab=d, gray=True)                      # in place with the grey plane beside it
            check(d.cpu().numpy(), want_lab, f"in place + grey {rows}x{cols} batch {b} offset {off}")
            check(g.cpu().numpy(), want_gray, f"grey beside in place {rows}x{cols} batch {b} offset {off}")
    # a partially overlapping d_lab and a d_gray inside d_bgr: refused, nothing written
    b, rows, cols = 2, 16, 24
    n = b * rows * cols
    img = image(b, rows, cols, 3)
    buf = torch.full((8 * n,), 0xC3, dtype=torch.uint8, device="cuda")
    d = buf[n:4 * n]
    d.copy_(dev(img.reshape(-1)))
    before = buf.cpu().numpy()
    call = lambda lab, gray: lib.dcmt_bgr_convert_dev(ctx._h, d.data_ptr(), rows, cols, b, lab, gray, None)
    far = buf[5 * n:].data_ptr()
    for lab, gray in ((d.data_ptr() + 3, None), (d.data_ptr() - 3, None), (d.data_ptr() + 3 * n - 1, None), (None, d.data_ptr()),
                      (None, d.data_ptr() + 2 * n), (None, d.data_ptr() - n + 1), (far, far + 3 * n - 1), (far, far), (d.data_ptr(), d.data_ptr() + n)):
        assert call(lab, gray) == L.E_INVALID, (lab, gray)
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before)
    assert call(d.data_ptr() + 3 * n, d.data_ptr() - n) == L.OK                    # touching is not overlapping
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    check(h[4 * n:7 * n].reshape(img.shape), R.bgr_to_lab(img), "Lab right behind the source")
    check(h[:n].reshape(img.shape[:-1]), R.bgr_to_gray(img), "grey right in front of the source")
    assert np.array_equal(h[n:4 * n], before[n:4 * n]) and (h[7 * n:] == 0xC3).all()


def test_argument_checks_on_a_live_context(ctx):
    import torch
    lib = L.lib()
    src = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    lab, gray = torch.zeros_like(src), torch.zeros((2, 8, 8), dtype=torch.uint8, device="cuda")
    args = dict(s=src.data_ptr(), r=8, c=8, b=2, l=lab.data_ptr(), g=gray.data_ptr())
    call = lambda **kw: lib.dcmt_bgr_convert_dev(ctx._h, *[dict(args, **kw)[k] for k in "srcblg"], None)
    assert call() == L.OK and call(l=None) == L.OK and call(g=None) == L.OK
    for bad in (dict(s=None), dict(l=None, g=None), dict(b=4), dict(b=0), dict(r=376), dict(r=0), dict(c=MAX_COLS + 1), dict(c=-1)):
        assert call(**bad) == L.E_INVALID, bad
    h, hl, hg = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.uint8)
    host = lambda bs, ls, gs, lab=hl.ctypes.data, gray=hg.ctypes.data: lib.dcmt_bgr_convert(ctx._h, h.ctypes.data, bs, 8, 8, lab, ls, gray, gs)
    assert host(24, 24, 8) == L.OK
    assert host(23, 24, 8) == L.E_INVALID and host(24, 23, 8) == L.E_INVALID and host(24, 24, 7) == L.E_INVALID
    assert host(24, 0, 8, lab=None) == L.OK and host(24, 24, 0, gray=None) == L.OK            # the stride of a NULL output is ignored
    assert host(24, 0, 0, lab=None, gray=None) == L.E_INVALID
    torch.cuda.synchronize()


def test_stream_order(ctx):
    """On a non-default stream, behind kernels that keep that stream busy and then fill d_bgr on it, with no synchronisation in
    between: the conversion reads what the fill wrote."""
    import torch
    b, rows, cols = 3, 352, 1216
    img = image(b, rows, cols, 77)
    mask = np.uint8(0x5C)
    masked = dev(img ^ mask)
    d = torch.zeros(img.shape, dtype=torch.uint8, device="cuda")
    busy = torch.ones((2048, 2048), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):
            busy = busy @ busy * 1e-4
        torch.bitwise_xor(masked, int(mask), out=d)                                # d = img, written by a kernel on s
        lab, gray = ctx.bgr_convert_dev(d, lab=True, gray=True)                    # torch's current stream: s
        lab2 = ctx.bgr_convert_dev(d, d_lab=d, stream=s.cuda_stream)               # and in place behind it, the stream given
    s.synchronize()
    assert lab2.data_ptr() == d.data_ptr()
    check(lab.cpu().numpy(), R.bgr_to_lab(img), "stream Lab")
    check(gray.cpu().numpy(), R.bgr_to_gray(img), "stream grey")
    check(d.cpu().numpy(), R.bgr_to_lab(img), "stream Lab in place")


def test_chain_into_slic(ctx):
    """bgr_convert_dev -> slic_labels_dev with no host copy in between equals slic_labels_dev on the restatement's Lab; 96 x 160,
    the shape and (step, nc) of the recorded SLIC chain."""
    rows, cols, step, nc = 96, 160, 7, 40
    img = np.stack([synth.synth_lab(rows, cols, 11 + f) for f in range(2)])         # smooth colour regions with edges: read as B, G, R
    labels, n, centers = ctx.slic_labels_dev(ctx.bgr_convert_dev(dev(img)), step, nc, return_centers=True)
    want, wn, wcent = ctx.slic_labels_dev(dev(R.bgr_to_lab(img)), step, nc, return_centers=True)
    assert n == wn and n > 0
    assert np.array_equal(labels.cpu().numpy(), want.cpu().numpy())
    assert np.array_equal(centers.cpu().numpy().view(np.uint64), wcent.cpu().numpy().view(np.uint64))
    assert len(np.unique(want.cpu().numpy())) > 1                                  # a segmentation, not one label


def test_chain_into_stereo_refine(ctx):
    """bgr_convert_dev on the left and the right image -> stereo_refine_dev, no host copy in between, equals the same call on the
    restatement's grey planes; 96 x 160, batch 2."""
    rows, cols = 96, 160
    pairs = [synth.synth_stereo(rows, cols, 5 + f) for f in range(2)]
    colour = lambda g: np.stack([g, (g.astype(np.int32) * 3 // 4 + 40).astype(np.uint8), 255 - g], axis=-1)   # B, G, R from a grey texture
    left = np.stack([colour(p[0]) for p in pairs])
    right = np.stack([colour(p[1]) for p in pairs])
    depth = dev(np.stack([p[2] for p in pairs]))
    lab, lgray = ctx.bgr_convert_dev(dev(left), lab=True, gray=True)                # the left image feeds SLIC too: both from one read
    rgray = ctx.bgr_convert_dev(dev(right), lab=False, gray=True)
    got = ctx.stereo_refine_dev(depth, lgray, rgray)
    want = ctx.stereo_refine_dev(depth, dev(R.bgr_to_gray(left)), dev(R.bgr_to_gray(right)))
    check(lab.cpu().numpy(), R.bgr_to_lab(left), "left Lab")
    assert_bit_equal(got.cpu().numpy(), want.cpu().numpy(), "refined depth")
    assert (want.cpu().numpy() != depth.cpu().numpy()).any()                       # the refinement moved something


def test_host_entry_python_and_cpp_shim_equal_the_restatement(ctx, tmp_path):
    import torch
    lib = L.lib()
    rows, cols = 75, 131
    img = image(2, rows, cols, 50)
    want_lab, want_gray = R.bgr_to_lab(img), R.bgr_to_gray(img)
    exe = tmp_path / "bgr_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv"),
                    DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, capture_output=True)
    for i in range(2):
        # the C ABI with every row stride larger than its row, odd ones among them; the padding is not the call's to touch
        src = np.full((rows, 3 * cols + 37), 0xEE, np.uint8)
        src[:, :3 * cols] = img[i].reshape(rows, -1)
        o_lab, o_gray = np.full((rows, 3 * cols + 5), 0x11, np.uint8), np.full((rows, cols + 3), 0x22, np.uint8)
        for lab, gray in MODES:
            o_lab[:], o_gray[:] = 0x11, 0x22
            st = lib.dcmt_bgr_convert(ctx._h, src.ctypes.data, src.strides[0], rows, cols, o_lab.ctypes.data if lab else None, o_lab.strides[0],
                                      o_gray.ctypes.data if gray else None, o_gray.strides[0])
            assert st == L.OK
            check(o_lab[:, :3 * cols].reshape(rows, cols, 3), want_lab[i] if lab else np.full((rows, cols, 3), 0x11, np.uint8), f"pitched Lab frame {i}")
            check(o_gray[:, :cols], want_gray[i] if gray else np.full((rows, cols), 0x22, np.uint8), f"pitched grey frame {i}")
            assert (o_lab[:, 3 * cols:] == 0x11).all() and (o_gray[:, cols:] == 0x22).all() and (src[:, 3 * cols:] == 0xEE).all()
        # api.Context.bgr_convert on a strided view, and the module functions on numpy and on CUDA input
        view = np.lib.stride_tricks.as_strided(src, (rows, cols, 3), (src.strides[0], 3, 1))
        both = ctx.bgr_convert(view, lab=True, gray=True)
        check(both[0], want_lab[i], f"Context.bgr_convert Lab frame {i}")
        check(both[1], want_gray[i], f"Context.bgr_convert grey frame {i}")
        check(api.bgr_to_lab(img[i]), want_lab[i], f"bgr_to_lab(numpy) frame {i}")
        check(api.bgr_to_gray(img[i]), want_gray[i], f"bgr_to_gray(numpy) frame {i}")
        t_lab, t_gray = api.bgr_to_lab(dev(img[i])), api.bgr_to_gray(dev(img[i]))
        assert t_lab.is_cuda and t_gray.is_cuda
        check(t_lab.cpu().numpy(), want_lab[i], f"bgr_to_lab(cuda) frame {i}")
        check(t_gray.cpu().numpy(), want_gray[i], f"bgr_to_gray(cuda) frame {i}")
        # the cv::Mat shim, through the C ABI
        img[i].tofile(tmp_path / "in.bgr")
        r = subprocess.run([str(exe), str(rows), str(cols), str(tmp_path / "in.bgr"), str(tmp_path / "out.lab"), str(tmp_path / "out.gray")],
                           capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        check(np.fromfile(tmp_path / "out.lab", dtype=np.uint8).reshape(rows, cols, 3), want_lab[i], f"dcmt_shim::bgr_to_lab frame {i}")
        check(np.fromfile(tmp_path / "out.gray", dtype=np.uint8).reshape(rows, cols), want_gray[i], f"dcmt_shim::bgr_to_gray frame {i}")
    batch = api.bgr_to_lab(dev(img))                                               # [batch][rows][cols][3] through the module function
    check(batch.cpu().numpy(), want_lab, "bgr_to_lab(cuda batch)")
    torch.cuda.synchronize()
