"""Reprojection of depth planes into another camera (dcmt_reproject_depth*, api.Context.reproject_depth_dev / reproject_depth,
api.unrectify_sol, dcmt_shim::unrectify_sol): the data part of unrectify_sol, DC_stereo_lidar/main_sl.cpp:967-1028.  Every comparison
is bit for bit against the numpy restatement np_reproject below: f64 numpy for x_, y_ (numpy's f64 -, *, / and the cast are the IEEE
operations the reference's C statements compile to), f32 numpy arrays op by op for the rest (numpy rounds each f32 operation once
and never fuses), the winner chosen explicitly as the largest source index per destination pixel."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "reproject_test.cpp")
f32 = np.float32
FX, FY, CX, CY = 9.597910e+02, 9.569251e+02, 6.960217e+02, 2.241806e+02       # main_sl.cpp:969-972
CAMERA_MAT = np.array([[9.597910e+02, 0, 6.960217e+02], [0, 9.569251e+02, 2.241806e+02], [0, 0, 1]], f32)   # :974-976
EYE = np.eye(4, dtype=f32)
# KITTI 2011_09_26 calib_cam_to_cam.txt, R_rect_02, as the 4x4 the reference builds (main_sl.cpp:207-220) ...
R_RECT_02 = np.array([[9.998817e-01, 1.511453e-02, -2.841595e-03, 0], [-1.511724e-02, 9.998853e-01, -9.338510e-04, 0],
                      [2.827154e-03, 9.766976e-04, 9.999955e-01, 0], [0, 0, 0, 1]], np.float64)
# ... and the f32 rounding of its f64 inverse
R_RECT_02_INV = np.array([[0.9998817443847656, -0.015117238275706768, 0.0028271544724702835, 0.0],
                          [0.01511453278362751, 0.9998852610588074, 0.000976697658188641, 0.0],
                          [-0.00284159486182034, -0.0009338509989902377, 0.9999955296516418, 0.0],
                          [0.0, 0.0, 0.0, 1.0]], f32)
TINY = ((1, 1), (1, 5), (7, 3), (3, 1), (2, 2), (5, 7), (1, 1242), (375, 1))
# intrinsics at the scale of the tiny shapes, so that rotations and bounds matter there
SMALL = dict(fx=3.5, fy=4.25, cx=1.5, cy=0.75, K=np.array([[3.5, 0, 1.5], [0, 4.25, 0.75], [0, 0, 1]], f32))


def rot(ax, ay, t=(0.0, 0.0, 0.0)):
    """Rotation about x by ax, then about y by ay (radians), and a translation, as a row-major f32 4x4."""
    rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx
    m[:3, 3] = t
    return m.astype(f32)


MATS = {"identity": EYE, "small": rot(0.02, -0.015), "behind": rot(0.1, math.radians(65.0)), "shift": rot(0.01, 0.02, (0.3, -0.2, 1.5))}


# ---------------------------------------------------------------- numpy restatement
def _project(d, M, K, fx, fy, cx, cy):
    """uf, vf, t_2 of every source pixel, the reference's operations one by one (:986-1001); garbage where t_2 <= 0."""
    r, c = d.shape
    z = np.ascontiguousarray(d, dtype=f32)
    zd = z.astype(np.float64)
    xs = ((np.arange(c, dtype=np.float64) - cx)[None, :] * zd / fx).astype(f32)
    ys = ((np.arange(r, dtype=np.float64) - cy)[:, None] * zd / fy).astype(f32)
    M, K = np.asarray(M, f32).reshape(4, 4), np.asarray(K, f32).reshape(3, 3)
    t = [((M[i, 0] * xs + M[i, 1] * ys) + M[i, 2] * z) + M[i, 3] for i in range(3)]
    assert all(a.dtype == f32 for a in t)
    with np.errstate(all="ignore"):
        uf = ((K[0, 0] * t[0] + K[0, 1] * t[1]) + K[0, 2] * t[2]) / t[2]
        vf = ((K[1, 0] * t[0] + K[1, 1] * t[1]) + K[1, 2] * t[2]) / t[2]
    assert uf.dtype == f32 and vf.dtype == f32
    return uf, vf, t[2]


def np_reproject(d, orows, ocols, M=EYE, K=CAMERA_MAT, fx=FX, fy=FY, cx=CX, cy=CY, info=None):
    uf, vf, t2 = _project(d, M, K, fx, fy, cx, cy)
    with np.errstate(invalid="ignore"):
        land = (t2 > 0) & (uf >= 0) & (uf < f32(ocols)) & (vf >= 0) & (vf < f32(orows))       # :999, :1008-1009
    idx = np.flatnonzero(land.ravel())                                                    # source indices, ascending = reference order
    flat = vf.ravel()[idx].astype(np.int64) * ocols + uf.ravel()[idx].astype(np.int64)     # (int) truncates
    winner = np.full(orows * ocols, -1, np.int64)
    np.maximum.at(winner, flat, idx)                                                      # the last writer = the largest source index
    out = np.zeros(orows * ocols, f32)
    hit = winner >= 0
    out[hit] = t2.ravel()[winner[hit]]
    if info is not None:
        info["landed"], info["distinct"] = len(idx), int(hit.sum())
    return out.reshape(orows, ocols)


def loop_reproject(d, orows, ocols, M=EYE, K=CAMERA_MAT, fx=FX, fy=FY, cx=CX, cy=CY):
    """The reference's double loop in its own order (:984-1021): a later source pixel simply overwrites."""
    M, K = np.asarray(M, f32).reshape(4, 4), np.asarray(K, f32).reshape(3, 3)
    out = np.zeros((orows, ocols), f32)
    for y in range(d.shape[0]):
        for x in range(d.shape[1]):
            z = f32(d[y, x])
            x_ = f32((float(x) - cx) * float(z) / fx)
            y_ = f32((float(y) - cy) * float(z) / fy)
            t = [f32(f32(f32(f32(M[i, 0] * x_) + f32(M[i, 1] * y_)) + f32(M[i, 2] * z)) + M[i, 3]) for i in range(3)]
            if not t[2] > 0:
                continue
            c = [f32(f32(f32(K[i, 0] * t[0]) + f32(K[i, 1] * t[1])) + f32(K[i, 2] * t[2])) for i in range(2)]
            with np.errstate(all="ignore"):
                uf, vf = f32(c[0] / t[2]), f32(c[1] / t[2])
            if uf >= 0 and uf < f32(ocols) and vf >= 0 and vf < f32(orows):
                out[int(vf), int(uf)] = t[2]
    return out


def want_batch(frames, orows, ocols, **kw):
    return np.stack([np_reproject(f, orows, ocols, **kw) for f in frames])


def mixed_frames(rng, b, rows, cols):
    """Positive depths with zeros, negatives and -0.0 among them; frame 1 of a batch is all zero."""
    x = (rng.random((b, rows, cols)) * 60.0 + 0.5).astype(f32)
    x[rng.random(x.shape) < 0.15] = 0.0
    x[rng.random(x.shape) < 0.1] = -0.0
    neg = rng.random(x.shape) < 0.1
    x[neg] = -x[neg]
    if b > 1:
        x[1] = 0
    return x


# ---------------------------------------------------------------- CPU
def test_exports_struct_size_defaults_and_bad_arguments_without_gpu():
    lib = L.lib()
    for name in ("dcmt_default_reproject_params", "dcmt_reproject_depth_dev", "dcmt_reproject_depth"):
        assert name in L.EXPORTS and getattr(lib, name) is not None
    assert ctypes.sizeof(L.ReprojectParams) == 136                     # 4 doubles, 16 + 9 floats, padded to 8
    p = api.make_reproject_params()
    assert (p.fx, p.fy, p.cx, p.cy) == (FX, FY, CX, CY)
    assert np.array_equal(np.array(p.M[:], f32).reshape(4, 4), EYE)
    assert np.array_equal(np.array(p.K[:], f32).reshape(3, 3), CAMERA_MAT)
    q = api.make_reproject_params(M=MATS["shift"], K=SMALL["K"], fx=700.0, cy=100.5)
    assert (q.fx, q.fy, q.cx, q.cy) == (700.0, FY, CX, 100.5)
    assert np.array_equal(np.array(q.M[:], f32).reshape(4, 4), MATS["shift"]) and np.array_equal(np.array(q.K[:], f32).reshape(3, 3), SMALL["K"])
    lib.dcmt_default_reproject_params(None)                             # ignored, no crash
    src = (ctypes.c_float * 16)()
    dst = (ctypes.c_float * 16)()
    pp = ctypes.byref(p)
    assert lib.dcmt_reproject_depth_dev(None, src, 4, 4, 1, pp, dst, 4, 4, None) == L.E_INVALID
    assert lib.dcmt_reproject_depth_dev(None, None, 4, 4, 1, None, None, 4, 4, None) == L.E_INVALID
    assert lib.dcmt_reproject_depth_dev(None, src, 1 << 20, 1 << 20, 70000, pp, dst, 1 << 20, 1 << 20, None) == L.E_INVALID
    assert lib.dcmt_reproject_depth(None, src, 16, 4, 4, pp, dst, 16, 4, 4) == L.E_INVALID
    assert lib.dcmt_reproject_depth(None, None, 16, 4, 4, None, None, 16, 4, 4) == L.E_INVALID
    assert lib.dcmt_reproject_depth(None, src, 4 << 20, 1 << 20, 1 << 20, pp, dst, 4 << 20, 1 << 20, 1 << 20) == L.E_INVALID
    import depth_completion_mt_amd as pkg
    for name in ("make_reproject_params", "unrectify_sol"):
        assert getattr(pkg, name) is getattr(api, name)


def test_known_answers_of_the_restatement():
    kw = dict(fx=2.0, fy=2.0, cx=0.0, cy=0.0, K=np.diag([2, 2, 1]).astype(f32))
    # every pixel maps to itself; 0 and the negative give t_2 <= 0 and are skipped
    got = np_reproject(np.array([[1, 2, 4], [8, 0, -1]], f32), 2, 3, **kw)
    assert_bit_equal(got, np.array([[1, 2, 4], [8, 0, 0]], f32), "identity")
    # no depth > 0 filter: with M[2][3] = 5 every pixel of an all-zero plane has t = (0, 0, 5), all six collide on (0, 0)
    M = EYE.copy()
    M[2, 3] = 5
    info = {}
    got = np_reproject(np.zeros((2, 3), f32), 2, 3, M=M, info=info, **kw)
    assert_bit_equal(got, np.array([[5, 0, 0], [0, 0, 0]], f32), "all-zero plane behind a translation")
    assert info == {"landed": 6, "distinct": 1}
    # a distinguishable winner: with M[0][3] = 1, depth 1 at column 0 goes to uf = 2 * (0 + 1) / 1 = 2 and depth 2 at column 1 to
    # uf = 2 * (1 + 1) / 2 = 2 as well; the later source pixel (depth 2) stays, whichever of the two depths is the larger
    M = EYE.copy()
    M[0, 3] = 1
    info = {}
    got = np_reproject(np.array([[1, 2, 0]], f32), 1, 3, M=M, info=info, **kw)
    assert_bit_equal(got, np.array([[0, 0, 2]], f32), "later source wins")
    assert info == {"landed": 2, "distinct": 1}
    got = np_reproject(np.array([[4, 2, 0]], f32), 1, 3, M=M, **kw)          # column 0: uf = 2 * (0 + 1) / 4 = 0.5 -> pixel 0
    assert_bit_equal(got, np.array([[4, 0, 2]], f32), "no collision")
    M[0, 3] = 2                                                              # depth 2 at column 0: uf = 2 * 2 / 2 = 2, depth 1 at column 1: uf = 2 * (1 + 2) = 6: out
    got = np_reproject(np.array([[2, 1, 1]], f32), 1, 3, M=M, **kw)
    assert_bit_equal(got, np.array([[0, 0, 2]], f32), "out of bounds to the right")


def test_vectorised_restatement_equals_the_loop_in_the_reference_order():
    rng = np.random.default_rng(3)
    d = mixed_frames(rng, 1, 12, 20)[0]
    half = CAMERA_MAT.copy()
    half[0, 0] *= 0.5
    half[1, 1] *= 0.5
    cases = [dict(M=m) for m in MATS.values()] + [dict(M=MATS["small"], K=half), dict(M=MATS["shift"], **SMALL), dict(M=MATS["behind"], **SMALL)]
    collided = 0
    for kw in cases:
        for orows, ocols in ((12, 20), (9, 25), (5, 7)):
            info = {}
            got = np_reproject(d, orows, ocols, info=info, **kw)
            assert_bit_equal(got, loop_reproject(d, orows, ocols, **kw), f"{orows}x{ocols}")
            collided += info["landed"] - info["distinct"]
    assert collided > 0


def test_inverse_helper_is_the_f32_rounding_of_the_f64_inverse():
    got = api.inverse_f32(R_RECT_02)
    assert got.dtype == f32 and got.shape == (4, 4)
    assert_bit_equal(got, R_RECT_02_INV, "inverse of R_rect_02")
    assert_bit_equal(got, np.linalg.inv(R_RECT_02).astype(f32), "numpy's f64 inverse, rounded")
    assert np.abs(got.astype(np.float64) @ R_RECT_02 - np.eye(4)).max() < 1e-7
    assert_bit_equal(api.inverse_f32(np.eye(4)), EYE, "identity")


def test_shim_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "tests", "mock_opencv"), "-c", DRIVER, "-o", str(tmp_path / "reproject_test.o")],
                   check=True, capture_output=True)


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


def params_of(**kw):
    return api.make_reproject_params(**kw)


def run(ctx, frames, orows, ocols, **kw):
    return ctx.reproject_depth_dev(dev(frames), orows, ocols, params_of(**kw)).cpu().numpy()


_dense = {}


def dense_pool(ctx, rows, cols):
    """A few dense planes: what complete_dev makes of sparse frames."""
    if (rows, cols) not in _dense:
        _dense[(rows, cols)] = ctx.complete_dev(dev(synth.synth_batch(3, rows, cols, 77))).cpu().numpy()
    return _dense[(rows, cols)]


@gpu
def test_tiny_shapes(ctx):
    rng = np.random.default_rng(5)
    pairs = [(s, s) for s in TINY]
    pairs += [((1, 5), (7, 3)), ((7, 3), (1, 5)), ((5, 7), (2, 2)), ((2, 2), (5, 7)), ((1, 1242), (375, 1)), ((375, 1), (1, 1242)),
              ((1, 1), (5, 7)), ((5, 7), (1, 1)), ((3, 1), (1, 5)), ((1, 5), (3, 1))]
    mods = set()
    for (rows, cols), (orows, ocols) in pairs:
        for b in (1, 3, 17):
            frames = mixed_frames(rng, b, rows, cols)
            mods.add(b * orows * ocols % 4)
            for name, M in MATS.items():
                for kw in (dict(M=M, **SMALL), dict(M=M)):
                    got = run(ctx, frames, orows, ocols, **kw)
                    assert_bit_equal(got, want_batch(frames, orows, ocols, **kw), f"{rows}x{cols} -> {orows}x{ocols} batch {b} {name} {sorted(kw)}")
    assert mods == {0, 1, 2, 3}
    # a [rows][cols] tensor is a batch of one
    one = mixed_frames(rng, 1, 5, 7)[0]
    got = ctx.reproject_depth_dev(dev(one), 7, 3, params_of(M=MATS["small"], **SMALL)).cpu().numpy()
    assert got.shape == (7, 3)
    assert_bit_equal(got, np_reproject(one, 7, 3, M=MATS["small"], **SMALL), "2-d tensor")


@gpu
def test_collisions(ctx):
    rng = np.random.default_rng(6)
    frames = mixed_frames(rng, 3, 64, 96)
    frames[2] = np.abs(frames[2]) + f32(0.5)
    kw0 = dict(fx=80.0, fy=78.0, cx=47.5, cy=31.0)
    for scale, least in ((0.5, 3.0), (0.1, 50.0)):
        K = np.array([[80.0 * scale, 0, 47.5 * scale], [0, 78.0 * scale, 31.0 * scale], [0, 0, 1]], f32)
        for name in ("identity", "small", "shift"):
            kw = dict(M=MATS[name], K=K, **kw0)
            info = {}
            np_reproject(frames[2], 64, 96, info=info, **kw)
            assert info["landed"] >= least * info["distinct"] > 0, (scale, name, info)          # several sources per destination
            assert_bit_equal(run(ctx, frames, 64, 96, **kw), want_batch(frames, 64, 96, **kw), f"K x {scale}, {name}")


@gpu
def test_full_size_with_the_kitti_rectification(ctx):
    for (rows, cols), (orows, ocols) in (((352, 1216), (375, 1242)), ((375, 1242), (352, 1216))):
        frames = dense_pool(ctx, rows, cols)
        assert (frames > 0).mean() > 0.99
        info = {}
        np_reproject(frames[0], orows, ocols, M=R_RECT_02_INV, info=info)
        assert info["landed"] > info["distinct"] > 0.8 * min(rows * cols, orows * ocols), info    # the case has collisions
        got = run(ctx, frames, orows, ocols, M=R_RECT_02_INV)
        assert_bit_equal(got, want_batch(frames, orows, ocols, M=R_RECT_02_INV), f"{rows}x{cols} -> {orows}x{ocols}")


@gpu
def test_frame_does_not_depend_on_batch_position_alignment_or_run(ctx):
    import torch
    rng = np.random.default_rng(20)
    rows, cols, orows, ocols = 61, 97, 59, 101                       # 17 * 59 * 101 is odd: single-dword stores for the whole batch
    kw = dict(M=MATS["shift"], fx=80.0, fy=78.0, cx=47.5, cy=31.0, K=np.array([[60.0, 0, 50.0], [0, 58.0, 29.0], [0, 0, 1]], f32))
    p = params_of(**kw)
    frames = mixed_frames(rng, 17, rows, cols)
    want = want_batch(frames, orows, ocols, **kw)
    d = dev(frames)
    full = ctx.reproject_depth_dev(d, orows, ocols, p)
    assert_bit_equal(full.cpu().numpy(), want, "batch 17")
    assert_bit_equal(ctx.reproject_depth_dev(d, orows, ocols, p).cpu().numpy(), want, "second run")
    assert_bit_equal(d.cpu().numpy(), frames, "the source plane")
    for i in (0, 1, 2, 16):
        assert_bit_equal(ctx.reproject_depth_dev(d[i], orows, ocols, p).cpu().numpy(), want[i], f"frame {i} alone")
        for pos in (0, 1, 2, 3):
            order = [(i + 5) % 17, (i + 7) % 17, (i + 9) % 17]
            order.insert(pos, i)                                      # batch 4: 16-byte stores where d_out allows
            got = ctx.reproject_depth_dev(d[order].contiguous(), orows, ocols, p).cpu().numpy()
            assert_bit_equal(got[pos], want[i], f"frame {i} at position {pos} of 4")
    # 4-byte-offset source and destination (every load / store width), with guard bands around d_out
    n, m = rows * cols, orows * ocols
    for b in (4, 2, 3):
        for soff, ooff in ((0, 0), (1, 0), (0, 1), (3, 2), (2, 3)):
            flat_s = torch.zeros(b * n + 8, dtype=torch.float32, device="cuda")
            s = flat_s[soff:soff + b * n].view(b, rows, cols)
            s.copy_(d[2:2 + b])
            buf = torch.full((b * m + 64,), -77.0, dtype=torch.float32, device="cuda")
            o = buf[32 + ooff:32 + ooff + b * m].view(b, orows, ocols)
            ctx.reproject_depth_dev(s, orows, ocols, p, d_out=o)
            h = buf.cpu().numpy()
            assert_bit_equal(h[32 + ooff:32 + ooff + b * m].reshape(b, orows, ocols), want[2:2 + b], f"batch {b}, offsets {soff}, {ooff}")
            assert (h[:32 + ooff] == -77.0).all() and (h[32 + ooff + b * m:] == -77.0).all(), f"guard bands, batch {b}, offsets {soff}, {ooff}"
            assert_bit_equal(s.cpu().numpy(), frames[2:2 + b], "the offset source plane")


@gpu
def test_shares_the_winner_plane_with_the_projection():
    import torch
    rng = np.random.default_rng(30)
    rows, cols = 64, 96
    P = np.array([[80.0, 0, 47.5, 0.5], [0, 78.0, 31.0, -0.25], [0, 0, 1, 0.01]], f32)
    T = rot(0.01, -0.02, (0.1, 0.0, 0.2))

    def cloud(seed, n):
        r = np.random.default_rng(seed)
        pts = np.empty((n, 4), f32)
        pts[:, 2] = r.random(n) * 40.0 + 1.0
        pts[:, 0] = (r.random(n) - 0.5) * 1.4 * pts[:, 2]
        pts[:, 1] = (r.random(n) - 0.5) * 1.0 * pts[:, 2]
        pts[:, 3] = 1.0
        return dev(pts), dev(np.array([0, n // 3, n // 3, n], np.int32))      # three frames, the middle one empty

    clouds = [cloud(31, 30000), cloud(32, 5000)]
    planes = [dev(mixed_frames(rng, 3, rows, cols)), dev(mixed_frames(rng, 2, 48, 80))]
    kws = [dict(M=MATS["shift"], fx=80.0, fy=78.0, cx=47.5, cy=31.0, K=P[:, :3].copy()), dict(M=MATS["small"], fx=70.0, fy=70.0, cx=40.0, cy=24.0, K=P[:, :3].copy())]
    outs = [(60, 100), (rows, cols)]
    steps = [("project", 0), ("reproject", 0), ("project", 1), ("reproject", 1)]

    def step(c, kind, i):
        if kind == "project":
            return c.project_points_dev(clouds[i][0], clouds[i][1], T, P, rows, cols)
        return c.reproject_depth_dev(planes[i], outs[i][0], outs[i][1], params_of(**kws[i]))

    lone = []
    for kind, i in steps:
        with api.Context(0, 64, 100, 3) as c:
            lone.append(step(c, kind, i).cpu().numpy())
    with api.Context(0, 64, 100, 3) as c:
        got = [step(c, kind, i) for kind, i in steps]                 # one context, torch's current stream, nothing in between
        torch.cuda.synchronize()
        got = [g.cpu().numpy() for g in got]
    for (kind, i), g, w in zip(steps, got, lone):
        assert (g != 0).sum() > 100, (kind, i)
        assert_bit_equal(g, w, f"{kind} {i} behind the other kind")
    for i in (0, 1):
        assert_bit_equal(lone[2 * i + 1], want_batch(planes[i].cpu().numpy(), outs[i][0], outs[i][1], **kws[i]), f"reproject {i}")


@gpu
def test_generation_wrap():
    import torch
    kw = dict(fx=6.0, fy=6.0, cx=3.5, cy=3.5, K=np.array([[6.0, 0, 3.5], [0, 6.0, 3.5], [0, 0, 1]], f32))
    lands, spins = params_of(M=EYE, **kw), params_of(M=MATS["behind"], **kw)   # a pure rotation of (0, 0, 0) has t_2 = 0: nothing lands
    base = (np.arange(64, dtype=f32).reshape(8, 8) * f32(0.25) + f32(1.0))
    zero = dev(np.zeros((8, 8), f32))
    with api.Context(0, 8, 8, 1) as c:
        planes = [dev(base + f32(k)) for k in range(0, 300, 2)]
        outs = [c.reproject_depth_dev(planes[k // 2], 8, 8, lands) if k % 2 == 0 else c.reproject_depth_dev(zero, 8, 8, spins) for k in range(300)]
        torch.cuda.synchronize()
        outs = torch.stack(outs).cpu().numpy()
    assert not outs[1::2].any(), np.flatnonzero(outs[1::2].reshape(150, -1).any(1)) * 2 + 1   # every zero-input call: all zeros
    for k in (0, 2, 252, 254, 256, 258, 294, 296, 298):
        want = np_reproject(base + f32(k), 8, 8, **kw)
        assert (want != 0).all()                                      # every pixel lands (on itself)
        assert_bit_equal(outs[k], want, f"call {k}")
    for k in (253, 255, 257, 297, 299):
        assert_bit_equal(outs[k], np.zeros((8, 8), f32), f"call {k}")


def np_round_trip(d, baseline=f32(0.54), focal=f32(9.597910e+02), max_depth=f32(100.0)):
    """stereo_refine with iterations = 0 (get_initial_disparity :846-861, retrieve_optimized_depth :863-885), f32 op by op."""
    bf = baseline * focal
    with np.errstate(all="ignore"):
        disp = np.where(d > 0, bf / d, f32(0))
        o = np.where(disp > 0, np.minimum(bf / disp, max_depth), f32(0))
    return o.astype(f32)


@gpu
def test_the_chain_of_the_stereo_lidar_main_on_one_stream(ctx):
    """main_sl.cpp:1225-1232 on the device: depth -> disparity -> depth, unrectify_sol, evaluate_performances; no synchronisation
    in between."""
    import torch
    rows, cols, orows, ocols = 352, 1216, 375, 1242
    dense = dense_pool(ctx, rows, cols)
    rng = np.random.default_rng(40)
    gt = np.where(rng.random((3, orows, ocols)) < 0.2, rng.random((3, orows, ocols)) * 70.0 + 1.0, 0.0).astype(f32)
    grey = rng.integers(0, 256, (3, rows, cols), dtype=np.uint8)
    p = params_of(M=R_RECT_02_INV)
    d, dg, gl = dev(dense), dev(gt), dev(grey)
    pre = ctx.stereo_refine_dev(d, gl, gl, iterations=0)
    unrect = ctx.reproject_depth_dev(pre, orows, ocols, p)
    sums = ctx.evaluate_dev(dg, unrect, 2.0, "both")
    torch.cuda.synchronize()
    pre, unrect, sums = pre.cpu().numpy(), unrect.cpu().numpy(), sums.cpu().numpy()
    w_pre = np.stack([np_round_trip(f) for f in dense])
    assert_bit_equal(pre, w_pre, "depth_pre_optim")
    w_unrect = want_batch(w_pre, orows, ocols, M=R_RECT_02_INV)
    assert_bit_equal(unrect, w_unrect, "depth_pre_optim_unrect")
    # the sums of the restated planes: the same bits as the evaluation run on them alone, and within the rounding of an f64 sum of
    # n terms in any order (n * 2^-53 * sum |x|, doubled for the second-order terms) of the exactly rounded sum of the f32 terms
    lone = ctx.evaluate_dev(dg, dev(w_unrect), 2.0, "both").cpu().numpy()
    assert np.array_equal(sums.view(np.uint64), lone.view(np.uint64))
    for i in range(3):
        m = (gt[i] > 2) & (w_unrect[i] > 2)
        e = gt[i][m] - w_unrect[i][m]
        ad = np.abs(e)
        assert sums[i][0] == m.sum() > 1000 and sums[i][4] == m.sum()
        for k, term in ((1, e), (2, ad), (3, ad * ad)):
            t64 = term.astype(np.float64)
            assert abs(sums[i][k] - math.fsum(t64.tolist())) <= len(t64) * 2.0 ** -52 * float(np.abs(t64).sum()), (i, k)


@gpu
def test_host_entry_python_and_cpp_shim_equal_the_device_call(ctx, tmp_path):
    import torch
    rows, cols, orows, ocols = 352, 1216, 375, 1242
    frame = dense_pool(ctx, rows, cols)[1]
    want = run(ctx, frame[None], orows, ocols, M=R_RECT_02_INV)[0]
    assert_bit_equal(want, np_reproject(frame, orows, ocols, M=R_RECT_02_INV), "device call")
    wide = np.full((rows, cols + 37), -9.0, f32)
    wide[:, :cols] = frame
    assert_bit_equal(ctx.reproject_depth(wide[:, :cols], orows, ocols, params_of(M=R_RECT_02_INV)), want, "dcmt_reproject_depth")
    assert_bit_equal(api.unrectify_sol(frame, (orows, ocols), R_RECT_02), want, "unrectify_sol")
    exe = tmp_path / "reproject_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv"),
                    DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"],
                   check=True, capture_output=True)
    frame.tofile(tmp_path / "in.f32")
    R_RECT_02_INV.tofile(tmp_path / "minv.f32")
    r = subprocess.run([str(exe), str(rows), str(cols), str(tmp_path / "in.f32"), str(tmp_path / "minv.f32"), str(orows), str(ocols),
                        str(tmp_path / "out.f32")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert_bit_equal(np.fromfile(tmp_path / "out.f32", dtype=f32).reshape(orows, ocols), want, "dcmt_shim::unrectify_sol")
    torch.cuda.synchronize()


@gpu
def test_argument_checks_on_a_live_context(ctx):
    import torch
    lib = L.lib()
    flat = torch.ones(4 * 8 * 16, dtype=torch.float32, device="cuda")
    src, dst = flat[:2 * 8 * 16], flat[2 * 8 * 16:]
    p = params_of()
    args = dict(d=src.data_ptr(), r=8, c=16, b=2, k=ctypes.addressof(p), o=dst.data_ptr(), R=8, C=16)
    call = lambda **kw: lib.dcmt_reproject_depth_dev(ctx._h, *[dict(args, **kw)[k] for k in "drcbkoRC"], None)
    assert call() == L.OK
    assert call(R=5, C=7) == L.OK
    nan_m, inf_k, zero_fx, zero_fy, inf_cx = params_of(), params_of(), params_of(fx=0.0), params_of(fy=0.0), params_of(cx=float("inf"))
    nan_m.M[6] = float("nan")
    inf_k.K[1] = float("inf")
    ignored = params_of()
    ignored.M[13] = float("nan")                                       # the 4th row of M is never read
    assert call(k=ctypes.addressof(ignored)) == L.OK
    for bad in (dict(d=None), dict(o=None), dict(k=None), dict(b=0), dict(b=18), dict(r=376), dict(c=1243), dict(R=376), dict(C=1243),
                dict(r=0), dict(C=0), dict(d=src.data_ptr() + 2), dict(o=dst.data_ptr() + 2),
                dict(k=ctypes.addressof(nan_m)), dict(k=ctypes.addressof(inf_k)), dict(k=ctypes.addressof(zero_fx)),
                dict(k=ctypes.addressof(zero_fy)), dict(k=ctypes.addressof(inf_cx)),
                dict(o=src.data_ptr()),                                                        # in place
                dict(o=src.data_ptr() + 4 * 16), dict(d=dst.data_ptr() - 4 * 16),              # d_out starts inside d_depth
                dict(d=src.data_ptr() + 4 * 16, o=src.data_ptr()),                             # d_depth starts inside d_out
                dict(o=dst.data_ptr() - 4)):                                                   # one element of overlap
        assert call(**bad) == L.E_INVALID, bad
    h = np.ones((8, 16), f32)
    out = np.zeros((8, 16), f32)
    hp = ctypes.byref(p)
    assert lib.dcmt_reproject_depth(ctx._h, h.ctypes.data, 64, 8, 16, hp, out.ctypes.data, 64, 8, 16) == L.OK
    assert lib.dcmt_reproject_depth(ctx._h, h.ctypes.data, 60, 8, 16, hp, out.ctypes.data, 64, 8, 16) == L.E_INVALID
    assert lib.dcmt_reproject_depth(ctx._h, h.ctypes.data, 64, 8, 16, hp, out.ctypes.data, 60, 8, 16) == L.E_INVALID
    assert lib.dcmt_reproject_depth(ctx._h, h.ctypes.data, 64, 376, 16, hp, out.ctypes.data, 64, 8, 16) == L.E_INVALID
    assert lib.dcmt_reproject_depth(ctx._h, h.ctypes.data, 64, 8, 16, hp, out.ctypes.data, 64, 8, 1243) == L.E_INVALID
    assert lib.dcmt_reproject_depth(ctx._h, h.ctypes.data, 64, 8, 16, ctypes.byref(nan_m), out.ctypes.data, 64, 8, 16) == L.E_INVALID
    torch.cuda.synchronize()
