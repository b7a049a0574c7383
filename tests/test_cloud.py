"""Back-projection of depth planes to ordered point clouds and the unmasked 5x5 Gaussian in front of it (dcmt_depth_to_cloud*,
dcmt_gaussian5*, api.Context.depth_to_cloud_dev / depth_to_cloud / gaussian5_dev / gaussian5, reproject_pc_colors, reproject_pc,
write_pcd / read_pcd, dcmt_shim::depth_to_cloud / gaussian_blur5): what DC_stereo_lidar/main_sl.cpp:1251-1270 does with the
refined depth.  Every comparison is bit for bit.  The cloud's yardstick is the numpy restatement np_cloud below (numpy's f64
-, *, / and the cast are the IEEE operations the reference's C statements compile to); the Gaussian's is oracle.gaussian5."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "cloud_test.cpp")
f32 = np.float32
FX, FY, CX, CY = 9.597910e+02, 9.569251e+02, 6.960217e+02, 2.241806e+02       # main_sl.cpp:927-930
TINY = ((1, 1), (1, 5), (7, 3), (3, 1), (2, 2), (5, 7), (1, 1242), (375, 1))


# ---------------------------------------------------------------- numpy restatement
def np_cloud(d, bgr=None, fx=FX, fy=FY, cx=CX, cy=CY):
    r, c = d.shape; m = d > 0; z = d.astype(np.float64)
    xs = ((np.arange(c, dtype=np.float64) - cx)[None, :] * z / fx).astype(np.float32)
    ys = ((np.arange(r, dtype=np.float64) - cy)[:, None] * z / fy).astype(np.float32)
    rec = np.zeros(int(m.sum()), dtype=[("x","<f4"),("y","<f4"),("z","<f4"),("b","u1"),("g","u1"),("r","u1"),("a","u1")])
    rec["x"], rec["y"], rec["z"] = xs[m], ys[m], d[m]                      # boolean indexing is row-major: the push_back order
    if bgr is None: rec.view(np.uint32).reshape(-1, 4)[:, 3] = np.float32(1).view(np.uint32)
    else: rec["b"], rec["g"], rec["r"], rec["a"] = bgr[m][:, 0], bgr[m][:, 1], bgr[m][:, 2], 255
    return rec


def words(rec):
    """Records (structured, or f32 [n, 4]) as uint32 [n, 4]."""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 4)


def np_colorize(frame, lut):
    """test_colorize.py's restatement of toColorImage, restated here: min-max to [0, 1] (scale computed in f64 and rounded to f32,
    x * scale + shift in two f32 roundings), * 255 rounded half to even and saturated, the JET palette."""
    x = np.asarray(frame, dtype=f32)
    smin, smax = float(x.min()), float(x.max())
    d = smax - smin
    scale = float(f32(1.0 / d if d > np.finfo(np.float64).eps else 0.0))
    shift = f32(float(f32(0.0)) - float(f32(smin * scale)))
    v = x * f32(scale) + shift
    return lut[np.clip(np.rint(v * f32(255.0)), 0, 255).astype(np.intp)]


KINDS = ("zero", "sparse", "dense", "allpos", "neg")


def frame_of(kind, rows, cols, seed, dense_pool):
    rng = np.random.default_rng(1000 + seed)
    if kind == "zero":
        return np.zeros((rows, cols), f32)
    if kind == "sparse":
        return synth.synth_frame(rows, cols, seed)                      # about 4 % valid
    if kind == "dense":
        return dense_pool[seed % len(dense_pool)].copy()
    if kind == "allpos":
        return (rng.random((rows, cols)) * 80.0 + 0.5).astype(f32)
    x = (rng.standard_normal((rows, cols)) * 30.0).astype(f32)           # negatives, zeros and -0.0 among positives
    x[rng.random((rows, cols)) < 0.2] = 0.0
    x[rng.random((rows, cols)) < 0.1] = -0.0
    return x


def batch_of(kinds, rows, cols, seed, dense_pool):
    return np.stack([frame_of(k, rows, cols, seed + i, dense_pool) for i, k in enumerate(kinds)])


def want_cloud(frames, bgr=None, **kw):
    recs = [np_cloud(frames[i], None if bgr is None else bgr[i], **kw) for i in range(frames.shape[0])]
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int32)
    return (np.concatenate(recs) if recs else np.zeros(0, api.CLOUD_DTYPE)), off


# ---------------------------------------------------------------- CPU
def test_exports_struct_sizes_defaults_and_bad_arguments_without_gpu():
    lib = L.lib()
    for name in ("dcmt_default_cloud_params", "dcmt_depth_to_cloud_dev", "dcmt_depth_to_cloud", "dcmt_gaussian5_dev", "dcmt_gaussian5"):
        assert name in L.EXPORTS and getattr(lib, name) is not None
    assert ctypes.sizeof(L.CloudPoint) == 16 and ctypes.sizeof(L.CloudParams) == 32 and api.CLOUD_DTYPE.itemsize == 16
    p = api.make_cloud_params()
    assert (p.fx, p.fy, p.cx, p.cy) == (9.597910e+02, 9.569251e+02, 6.960217e+02, 2.241806e+02)
    q = api.make_cloud_params(fx=700.0, cy=100.5)
    assert (q.fx, q.fy, q.cx, q.cy) == (700.0, FY, CX, 100.5)
    lib.dcmt_default_cloud_params(None)                            # ignored, no crash
    src = (ctypes.c_float * 16)()
    bgr = (ctypes.c_uint8 * 48)()
    pts = (L.CloudPoint * 16)()
    off = (ctypes.c_int32 * 2)()
    n = ctypes.c_int64(0)
    pp = ctypes.byref(p)
    assert lib.dcmt_depth_to_cloud_dev(None, src, bgr, 4, 4, 1, pp, pts, 16, off, None) == L.E_INVALID
    assert lib.dcmt_depth_to_cloud_dev(None, None, None, 4, 4, 1, None, None, 16, None, None) == L.E_INVALID
    assert lib.dcmt_depth_to_cloud_dev(None, src, bgr, 1 << 20, 1 << 20, 70000, pp, pts, 16, off, None) == L.E_INVALID
    assert lib.dcmt_depth_to_cloud(None, src, 16, bgr, 12, 4, 4, pp, pts, 16, ctypes.byref(n)) == L.E_INVALID
    assert lib.dcmt_depth_to_cloud(None, None, 16, None, 12, 4, 4, None, None, 16, None) == L.E_INVALID
    assert lib.dcmt_depth_to_cloud(None, src, 4 << 20, bgr, 3 << 20, 1 << 20, 1 << 20, pp, pts, 16, ctypes.byref(n)) == L.E_INVALID
    assert lib.dcmt_gaussian5_dev(None, src, src, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_gaussian5_dev(None, None, None, 4, 4, 1, None) == L.E_INVALID
    assert lib.dcmt_gaussian5_dev(None, src, src, 1 << 20, 1 << 20, 70000, None) == L.E_INVALID
    assert lib.dcmt_gaussian5(None, src, 16, src, 16, 4, 4) == L.E_INVALID
    assert lib.dcmt_gaussian5(None, None, 16, None, 16, 4, 4) == L.E_INVALID
    assert lib.dcmt_gaussian5(None, src, 4 << 20, src, 4 << 20, 1 << 20, 1 << 20) == L.E_INVALID
    import depth_completion_mt_amd as pkg
    for name in ("make_cloud_params", "reproject_pc_colors", "reproject_pc", "write_pcd", "read_pcd", "CLOUD_DTYPE"):
        assert getattr(pkg, name) is getattr(api, name)


def test_known_answers_of_the_restatement():
    one = np_cloud(np.array([[1.0]], f32))
    assert len(one) == 1
    assert one["x"][0] == f32(-696.0217 / 959.791) and one["y"][0] == f32(-224.1806 / 956.9251) and one["z"][0] == f32(1.0)
    assert words(one)[0, 3] == 0x3f800000
    # -0.0, 0, a negative and one positive value: one record
    d = np.array([[-0.0, 0.0], [-3.5, 2.5]], f32)
    col = np.arange(12, dtype=np.uint8).reshape(2, 2, 3)
    rec = np_cloud(d, col)
    assert len(rec) == 1 and rec["z"][0] == f32(2.5)
    assert (rec["b"][0], rec["g"][0], rec["r"][0], rec["a"][0]) == (9, 10, 11, 255)
    assert rec["x"][0] == f32((1.0 - CX) * 2.5 / FX) and rec["y"][0] == f32((1.0 - CY) * 2.5 / FY)
    assert words(rec)[0, 3] == 9 | 10 << 8 | 11 << 16 | 255 << 24
    # row-major order of a 2 x 3 plane: z carries the pixel's number
    d = np.arange(1, 7, dtype=f32).reshape(2, 3)
    rec = np_cloud(d)
    assert rec["z"].tolist() == [1, 2, 3, 4, 5, 6]
    assert np.array_equal(rec["x"], ((np.tile(np.arange(3.0), 2) - CX) * np.arange(1.0, 7.0) / FX).astype(f32))
    assert np.array_equal(rec["y"], ((np.repeat(np.arange(2.0), 3) - CY) * np.arange(1.0, 7.0) / FY).astype(f32))
    assert np_cloud(np.zeros((3, 4), f32)).shape == (0,)


def test_shim_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "tests", "mock_opencv"), "-c", DRIVER, "-o", str(tmp_path / "cloud_test.o")],
                   check=True, capture_output=True)


def test_pcd_round_trip(tmp_path):
    rng = np.random.default_rng(7)
    d = (rng.random((9, 13)) * 40.0).astype(f32)
    d[rng.random(d.shape) < 0.4] = 0
    col = rng.integers(0, 256, (9, 13, 3), dtype=np.uint8)
    for rec in (np_cloud(d, col), np_cloud(d), np_cloud(np.zeros((2, 2), f32))):
        path = tmp_path / "cloud.pcd"
        api.write_pcd(path, rec)
        blob = path.read_bytes()
        head = blob[:blob.index(b"DATA binary\n") + 12].decode("ascii")
        n = len(rec)
        assert f"\nPOINTS {n}\n" in head and f"\nWIDTH {n}\n" in head and "\nHEIGHT 1\n" in head and head.endswith("DATA binary\n")
        assert "\nFIELDS x y z rgb\n" in head and "\nSIZE 4 4 4 4\n" in head and "\nCOUNT 1 1 1 1\n" in head
        assert len(blob) == len(head) + 16 * n and blob[len(head):] == rec.tobytes()
        back = api.read_pcd(path)
        assert back.dtype == api.CLOUD_DTYPE and np.array_equal(words(back), words(rec))
        api.write_pcd(path, words(rec).view(f32))                     # the [n, 4] float32 form the device call returns
        assert np.array_equal(words(api.read_pcd(path)), words(rec))


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


_dense = {}


def dense_pool(ctx, rows, cols):
    """A few dense planes: what complete_dev makes of sparse frames."""
    if (rows, cols) not in _dense:
        _dense[(rows, cols)] = ctx.complete_dev(dev(synth.synth_batch(4, rows, cols, 77))).cpu().numpy()
    return _dense[(rows, cols)]


def run_cloud(ctx, frames, bgr=None, **kw):
    """The device call; returns (records uint32 [total, 4], offsets int32 [b + 1])."""
    pts, off = ctx.depth_to_cloud_dev(dev(frames), None if bgr is None else dev(bgr), **kw)
    off = off.cpu().numpy()
    assert pts.shape[1] == 4 and off[-1] <= pts.shape[0]
    return words(pts[:off[-1]].cpu().numpy()), off


def check_cloud(got, off, frames, bgr, what, **kw):
    want, woff = want_cloud(frames, bgr, **kw)
    assert off.dtype == np.int32 and np.array_equal(off, woff), (what, off, woff)
    w = words(want)
    if not np.array_equal(got, w):
        bad = np.argwhere((got != w).any(1))[:, 0]
        raise AssertionError(f"{what}: {len(bad)} of {len(w)} records differ, first at {bad[0]}: {got[bad[0]]} vs {w[bad[0]]}")


@gpu
def test_bit_exact_against_the_restatement(ctx):
    rng = np.random.default_rng(1)
    for rows, cols in ((352, 1216), (375, 1242)):
        pool = dense_pool(ctx, rows, cols)
        cases = [(k,) for k in KINDS]
        cases += [("zero", "dense", "sparse"), ("neg", "zero", "allpos"), ("sparse", "dense", "zero")]
        cases += [tuple(KINDS[i % 5] for i in range(16)) + ("zero",)]            # zero first, in the middle (5, 10, 15) and last
        for ci, kinds in enumerate(cases):
            frames = batch_of(kinds, rows, cols, 10 * ci, pool)
            bgr = rng.integers(0, 256, frames.shape + (3,), dtype=np.uint8)
            got, off = run_cloud(ctx, frames, bgr)
            check_cloud(got, off, frames, bgr, f"{rows}x{cols} {kinds} colour")
            for i, k in enumerate(kinds):
                if k == "zero":
                    assert off[i + 1] == off[i]
                if k == "allpos":
                    assert off[i + 1] - off[i] == rows * cols
            got, off = run_cloud(ctx, frames)
            check_cloud(got, off, frames, None, f"{rows}x{cols} {kinds} no colour")
            assert (got[:, 3] == 0x3f800000).all()
    # non-default intrinsics, and a [rows][cols] tensor as a batch of one
    rows, cols = 375, 1242
    frames = batch_of(("dense", "neg", "sparse"), rows, cols, 90, dense_pool(ctx, rows, cols))
    bgr = rng.integers(0, 256, frames.shape + (3,), dtype=np.uint8)
    kw = dict(fx=721.5377, fy=-707.0912, cx=609.5593, cy=172.854)
    got, off = run_cloud(ctx, frames, bgr, params=api.make_cloud_params(**kw))
    check_cloud(got, off, frames, bgr, "non-default intrinsics", **kw)
    got, off = run_cloud(ctx, frames[1], bgr[1])
    check_cloud(got, off, frames[1:2], bgr[1:2], "2-d tensor")


@gpu
def test_tiny_shapes(ctx):
    rng = np.random.default_rng(5)
    for rows, cols in TINY:
        for b in (1, 3, 17):
            frames = (rng.standard_normal((b, rows, cols)) * 20.0).astype(f32)
            frames[rng.random(frames.shape) < 0.25] = 0
            frames[::4] = np.abs(frames[::4]) + f32(1.0)                          # all-positive frames among them
            if b > 1:
                frames[1] = 0
            bgr = rng.integers(0, 256, frames.shape + (3,), dtype=np.uint8)
            got, off = run_cloud(ctx, frames, bgr)
            check_cloud(got, off, frames, bgr, f"{rows}x{cols} batch {b} colour")
            got, off = run_cloud(ctx, frames)
            check_cloud(got, off, frames, None, f"{rows}x{cols} batch {b}")


@gpu
def test_frame_records_do_not_depend_on_batch_position_alignment_or_run(ctx):
    import torch
    rows, cols = 375, 1242                                        # rows * cols % 4 == 2
    n = rows * cols
    rng = np.random.default_rng(20)
    kinds = tuple(KINDS[(i + 1) % 5] for i in range(17))
    frames = batch_of(kinds, rows, cols, 200, dense_pool(ctx, rows, cols))
    bgr = rng.integers(0, 256, frames.shape + (3,), dtype=np.uint8)
    d, dc = dev(frames), dev(bgr)
    pts, off = ctx.depth_to_cloud_dev(d, dc)
    off = off.cpu().numpy()
    full = words(pts[:off[-1]].cpu().numpy())
    check_cloud(full, off, frames, bgr, "batch 17")
    pts2, off2 = ctx.depth_to_cloud_dev(d, dc)                   # two runs: the same bytes
    assert np.array_equal(off2.cpu().numpy(), off) and np.array_equal(words(pts2[:off[-1]].cpu().numpy()), full)
    own = lambda i: full[off[i]:off[i + 1]]
    for i in (0, 1, 2, 3, 4):                                     # one frame of every kind
        p1, o1 = ctx.depth_to_cloud_dev(d[i], dc[i])
        o1 = o1.cpu().numpy()
        assert o1.tolist() == [0, off[i + 1] - off[i]] and np.array_equal(words(p1[:o1[1]].cpu().numpy()), own(i)), f"frame {i} alone"
        for pos in (0, 1, 2):
            order = [(i + 5) % 17, (i + 7) % 17]
            order.insert(pos, i)
            p3, o3 = ctx.depth_to_cloud_dev(d[order].contiguous(), dc[order].contiguous())
            o3 = o3.cpu().numpy()
            assert np.array_equal(words(p3[o3[pos]:o3[pos + 1]].cpu().numpy()), own(i)), f"frame {i} at position {pos} of 3"
    # depth at element offsets 1 and 3 (dword-aligned only), colour at byte offsets 1 and 5
    flat_d = torch.zeros(3 * n + 8, dtype=torch.float32, device="cuda")
    flat_c = torch.zeros(3 * 3 * n + 16, dtype=torch.uint8, device="cuda")
    want3 = full[off[2]:off[5]]
    for doff, coff in ((1, 0), (3, 1), (0, 5), (1, 5)):
        s = flat_d[doff:doff + 3 * n].view(3, rows, cols)
        s.copy_(d[2:5])
        c = flat_c[coff:coff + 9 * n].view(3, rows, cols, 3)
        c.copy_(dc[2:5])
        p3, o3 = ctx.depth_to_cloud_dev(s, c)
        o3 = o3.cpu().numpy()
        assert np.array_equal(o3, off[2:6] - off[2]) and np.array_equal(words(p3[:o3[-1]].cpu().numpy()), want3), (doff, coff)


@gpu
def test_guards_capacity_and_sources_untouched(ctx):
    import torch
    rng = np.random.default_rng(30)
    for rows, cols, kinds in ((375, 1242, tuple(KINDS[i % 5] for i in range(17))), (7, 3, ("allpos",) * 17), (1, 5, ("allpos", "neg", "allpos")),
                              (352, 1216, ("dense", "sparse"))):
        b = len(kinds)
        frames = batch_of(kinds, rows, cols, 300, dense_pool(ctx, rows, cols) if rows > 300 else [np.ones((rows, cols), f32)])
        bgr = rng.integers(0, 256, frames.shape + (3,), dtype=np.uint8)
        want, woff = want_cloud(frames, bgr)
        total = int(woff[-1])
        assert total >= 2
        d, dc = dev(frames), dev(bgr)
        room = b * rows * cols
        for cap in (room, total // 2):
            buf = torch.full((16 * room + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
            pts = buf[:16 * room].view(torch.float32).view(room, 4)
            _, off = ctx.depth_to_cloud_dev(d, dc, d_points=pts, capacity=cap)
            h = buf.cpu().numpy()
            assert np.array_equal(off.cpu().numpy(), woff), (rows, cols, cap)        # the true counts, also on overflow
            kept = min(total, cap)
            assert np.array_equal(h[:16 * kept].view(np.uint32).reshape(-1, 4), words(want)[:kept]), (rows, cols, cap)
            assert (h[16 * kept:] == 0xA5).all(), (rows, cols, cap)
        assert_bit_equal(d.cpu().numpy(), frames, "depth after the cloud call")
        assert np.array_equal(dc.cpu().numpy(), bgr)


@gpu
def test_argument_checks_on_a_live_context(ctx):
    import torch
    lib = L.lib()
    src = torch.ones((2, 8, 8), dtype=torch.float32, device="cuda")
    col = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    pts = torch.zeros((128, 4), dtype=torch.float32, device="cuda")
    off = torch.zeros((3,), dtype=torch.int32, device="cuda")
    p = api.make_cloud_params()
    args = dict(d=src.data_ptr(), g=col.data_ptr(), r=8, c=8, b=2, k=ctypes.addressof(p), o=pts.data_ptr(), n=128, f=off.data_ptr())
    call = lambda **kw: lib.dcmt_depth_to_cloud_dev(ctx._h, *[dict(args, **kw)[k] for k in "dgrcbkonf"], None)
    assert call() == L.OK
    assert call(g=None) == L.OK
    assert call(n=0) == L.OK
    zero_fx, inf_fy = api.make_cloud_params(fx=0.0), api.make_cloud_params(fy=float("inf"))
    for bad in (dict(d=None), dict(o=None), dict(f=None), dict(k=None), dict(b=0), dict(b=18), dict(r=376), dict(c=1243), dict(r=0),
                dict(o=pts.data_ptr() + 8), dict(d=src.data_ptr() + 2), dict(n=-1), dict(k=ctypes.addressof(zero_fx)),
                dict(k=ctypes.addressof(inf_fy))):
        assert call(**bad) == L.E_INVALID, bad
    torch.cuda.synchronize()
    assert off.cpu().numpy().tolist() == [0, 64, 128]
    dst = torch.zeros_like(src)
    g = lambda s, t, r=8, c=8, b=2: lib.dcmt_gaussian5_dev(ctx._h, s, t, r, c, b, None)
    assert g(src.data_ptr(), dst.data_ptr()) == L.OK
    assert g(src.data_ptr(), src.data_ptr()) == L.OK
    for bad in ((None, dst.data_ptr()), (src.data_ptr(), None), (src.data_ptr() + 2, dst.data_ptr())):
        assert g(*bad) == L.E_INVALID, bad
    for kw in (dict(b=0), dict(b=18), dict(r=376), dict(c=1243)):
        assert g(src.data_ptr(), dst.data_ptr(), **kw) == L.E_INVALID, kw
    h = np.ones((8, 8), f32)
    out = np.zeros((8, 8), f32)
    rec = np.zeros(64, api.CLOUD_DTYPE)
    n = ctypes.c_int64(0)
    assert lib.dcmt_gaussian5(ctx._h, h.ctypes.data, 32, out.ctypes.data, 32, 8, 8) == L.OK
    assert lib.dcmt_gaussian5(ctx._h, h.ctypes.data, 28, out.ctypes.data, 32, 8, 8) == L.E_INVALID
    assert lib.dcmt_depth_to_cloud(ctx._h, h.ctypes.data, 32, None, 0, 8, 8, ctypes.byref(p), rec.ctypes.data, 10, ctypes.byref(n)) == L.OK
    assert n.value == 64 and (rec["z"][:10] == 1).all() and (rec["z"][10:] == 0).all()          # the true count; 10 records written
    assert lib.dcmt_depth_to_cloud(ctx._h, h.ctypes.data, 28, None, 0, 8, 8, ctypes.byref(p), rec.ctypes.data, 64, ctypes.byref(n)) == L.E_INVALID
    torch.cuda.synchronize()


@gpu
def test_gaussian5_against_the_oracle(ctx):
    from oracle import oracle as O
    import torch
    rng = np.random.default_rng(40)

    def check(frames, what):
        d = dev(frames)
        out = ctx.gaussian5_dev(d)
        got = out.cpu().numpy()
        for i in range(frames.shape[0]):
            assert_bit_equal(got[i], O.gaussian5(frames[i]), f"{what} frame {i}")
        assert_bit_equal(d.cpu().numpy(), frames, f"{what}: source")
        same = ctx.gaussian5_dev(d, d_dst=d)                              # in place: the bits of the out-of-place call
        assert same is d
        assert_bit_equal(d.cpu().numpy(), got, f"{what} in place")

    for rows, cols in ((352, 1216), (375, 1242)):
        pool = dense_pool(ctx, rows, cols)
        for b in (1, 3, 17):
            kinds = tuple(("dense", "sparse", "neg")[i % 3] for i in range(b))
            check(batch_of(kinds, rows, cols, 400 + b, pool), f"{rows}x{cols} batch {b}")
    for rows, cols in TINY:
        for b in (1, 3, 17):
            check((rng.standard_normal((b, rows, cols)) * 20.0).astype(f32), f"{rows}x{cols} batch {b}")
    # a destination shifted by one row overlaps the source: rejected
    flat = torch.zeros(4 * 8 * 16, dtype=torch.float32, device="cuda")
    s, t = flat[:3 * 8 * 16], flat[16:16 + 3 * 8 * 16]
    assert L.lib().dcmt_gaussian5_dev(ctx._h, s.data_ptr(), t.data_ptr(), 8, 16, 3, None) == L.E_INVALID
    assert L.lib().dcmt_gaussian5_dev(ctx._h, t.data_ptr(), s.data_ptr(), 8, 16, 3, None) == L.E_INVALID
    torch.cuda.synchronize()


@gpu
def test_the_chain_of_the_stereo_lidar_main_on_one_stream():
    """main_sl.cpp:1246-1270 on the device: completion -> GaussianBlur (in place) -> toColorImage -> reproject_pc_colors, then a
    normalised completion behind it; no synchronisation in between."""
    from oracle import oracle as O
    import torch
    frames = synth.synth_batch(16, 352, 1216, 40)
    norm = api.make_params(normalize=(0, 80))
    lut = np.asarray(api.JET_BGR)
    with api.Context(0, 352, 1216, 16) as c:
        d = dev(frames)
        n1 = c.complete_dev(d, params=norm)
        torch.cuda.synchronize()
        n1 = n1.cpu().numpy()
        dense = c.complete_dev(d)
        keep = dense.clone()
        path = c.last_path()
        blur = c.gaussian5_dev(dense, d_dst=dense)
        col = c.colorize_dev(blur)
        pts, off = c.depth_to_cloud_dev(blur, col)
        assert c.last_path() == path
        n2 = c.complete_dev(d, params=norm)
        torch.cuda.synchronize()
        keep, blur, col, off, n2 = keep.cpu().numpy(), blur.cpu().numpy(), col.cpu().numpy(), off.cpu().numpy(), n2.cpu().numpy()
        got = words(pts[:off[-1]].cpu().numpy())
    assert np.array_equal(n1.view(np.uint32), n2.view(np.uint32))
    for i in range(16):
        if i in (0, 7, 15):                                           # the oracle's whole cascade: three frames of it
            assert_bit_equal(keep[i], O.img_completion(frames[i]), f"completion frame {i}")
            assert_bit_equal(n2[i], O.img_completion(O.normalize_minmax(frames[i], 0, 80)), f"normalised completion frame {i}")
        assert_bit_equal(blur[i], O.gaussian5(keep[i]), f"blur frame {i}")
        assert np.array_equal(col[i], np_colorize(blur[i], lut)), f"colour frame {i}"
    check_cloud(got, off, blur, col, "cloud of the chain")


@gpu
def test_cloud_goes_straight_back_into_the_projection(ctx):
    from oracle import oracle as O
    rows, cols = 352, 1216
    frames = synth.synth_batch(3, rows, cols, 60)
    pts, off = ctx.depth_to_cloud_dev(dev(frames))
    h_off = off.cpu().numpy()
    want, woff = want_cloud(frames)
    assert np.array_equal(h_off, woff)
    T = np.eye(4, dtype=f32)
    P = np.array([[FX, 0, CX, 0], [0, FY, CY, 0], [0, 0, 1, 0]], dtype=f32)
    sparse = ctx.project_points_dev(pts[:int(h_off[-1])], off, T, P, rows, cols).cpu().numpy()
    w = words(want).view(f32)
    for i in range(3):
        assert_bit_equal(sparse[i], O.project_points(w[woff[i]:woff[i + 1]], T, P, rows, cols), f"frame {i}")
        assert (sparse[i] > 0).sum() > 0.5 * (frames[i] > 0).sum()


@gpu
def test_host_entry_python_and_cpp_shim_equal_the_device_call(ctx, tmp_path):
    from oracle import oracle as O
    import torch
    rows, cols = 375, 1242
    rng = np.random.default_rng(50)
    frames = batch_of(("dense", "neg"), rows, cols, 500, dense_pool(ctx, rows, cols))
    bgr = rng.integers(0, 256, frames.shape + (3,), dtype=np.uint8)
    exe = tmp_path / "cloud_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv"),
                    DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, capture_output=True)
    blur_dev = ctx.gaussian5_dev(dev(frames)).cpu().numpy()
    for i in range(2):
        for colour in (bgr[i], None):
            what = f"frame {i} {'colour' if colour is not None else 'no colour'}"
            want, off = run_cloud(ctx, frames[i], colour)
            check_cloud(want, off, frames[i:i + 1], None if colour is None else colour[None], what)
            wide = np.full((rows, cols + 37), -9.0, f32)
            wide[:, :cols] = frames[i]
            wcol = None
            if colour is not None:
                wcol = np.zeros((rows, cols + 11, 3), np.uint8)
                wcol[:, :cols] = colour
                wcol = wcol[:, :cols]
            rec = ctx.depth_to_cloud(wide[:, :cols], wcol)
            assert rec.dtype == api.CLOUD_DTYPE and np.array_equal(words(rec), want), f"dcmt_depth_to_cloud {what}"
            fn = (lambda x: api.reproject_pc(x)) if colour is None else (lambda x: api.reproject_pc_colors(x, colour if isinstance(x, np.ndarray) else dev(colour)))
            assert np.array_equal(words(fn(frames[i])), want), f"reproject (numpy) {what}"
            t = fn(dev(frames[i]))
            assert t.is_cuda and np.array_equal(words(t.cpu().numpy()), want), f"reproject (cuda) {what}"
            frames[i].tofile(tmp_path / "in.f32")
            if colour is not None:
                colour.tofile(tmp_path / "in.bgr")
            r = subprocess.run([str(exe), str(rows), str(cols), str(tmp_path / "in.f32"), str(tmp_path / "in.bgr") if colour is not None else "-",
                                str(tmp_path / "blur.f32"), str(tmp_path / "cloud.bin")], capture_output=True, text=True)
            assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
            got = np.fromfile(tmp_path / "cloud.bin", dtype=np.uint32).reshape(-1, 4)
            assert np.array_equal(got, want), f"dcmt_shim::depth_to_cloud {what}"
            assert_bit_equal(np.fromfile(tmp_path / "blur.f32", dtype=f32).reshape(rows, cols), blur_dev[i], f"dcmt_shim::gaussian_blur5 {what}")
        assert_bit_equal(blur_dev[i], O.gaussian5(frames[i]), f"gaussian5_dev frame {i}")
        wide = np.full((rows, cols + 37), -9.0, f32)
        wide[:, :cols] = frames[i]
        assert_bit_equal(ctx.gaussian5(wide[:, :cols]), blur_dev[i], f"dcmt_gaussian5 frame {i}")
    torch.cuda.synchronize()
