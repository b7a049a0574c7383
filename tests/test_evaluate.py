"""Accuracy metrics against ground truth (dcmt_evaluate*, api.evaluate_dev / evaluate / eval_summary / evaluate_performance): the
reference's evaluate_performance(s) (LO main.cpp:16-34, LC main_lc.cpp:85-116, SL main_sl.cpp:1031-1061) plus the inverse-depth terms
of main_lc.cpp:96.  Expected values come from numpy: per-pixel terms in f32 / f64 exactly as include/dcmt.h states them, summed with
math.fsum."""
import ctypes
import math

import numpy as np
import pytest

from conftest import assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

FIELDS = api.EVAL_FIELDS


# ---------------------------------------------------------------- numpy restatement
def np_terms(gt, pred, thresh, mode):
    """The masked per-pixel terms of one frame: (n, [e, d, d*d] f32, n_inv, [di, di*di] f64)."""
    g = np.ascontiguousarray(gt, dtype=np.float32).ravel()
    p = np.ascontiguousarray(pred, dtype=np.float32).ravel()
    t = np.float32(thresh)
    m = g > t
    if mode == "both":
        m &= p > t
    e = g[m] - p[m]                                   # f32 difference
    d = np.abs(e)
    sq = d * d                                        # f32 product
    inv = m & (p > 0)
    di = np.abs(1.0 / g[inv].astype(np.float64) - 1.0 / p[inv].astype(np.float64))
    return int(m.sum()), [e, d, sq], int(inv.sum()), [di, di * di]


def check_sums(got, gt, pred, thresh, mode, what=""):
    n, t3, n_inv, t2 = np_terms(gt, pred, thresh, mode)
    got = np.asarray(got, dtype=np.float64).reshape(7)
    assert got[0] == n and got[4] == n_inv, f"{what}: counts {got[0]}, {got[4]} vs {n}, {n_inv}"
    for k, (cnt, term) in zip((1, 2, 3, 5, 6), [(n, x) for x in t3] + [(n_inv, x) for x in t2]):
        want = math.fsum(term.astype(np.float64).tolist())
        tol = cnt * 2.0 ** -50 * float(np.abs(term.astype(np.float64)).sum())
        assert abs(got[k] - want) <= tol, f"{what}: {FIELDS[k]} {got[k]!r} vs fsum {want!r} (tol {tol})"


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- CPU
def test_eval_frame_struct_and_exports():
    assert ctypes.sizeof(L.EvalFrame) == 56
    assert [f for f, _ in L.EvalFrame._fields_] == list(FIELDS)
    for name in ("dcmt_evaluate_dev", "dcmt_evaluate_u16_dev", "dcmt_evaluate"):
        assert name in L.EXPORTS and getattr(L.lib(), name) is not None
    assert (L.EVAL_GT, L.EVAL_BOTH) == (0, 1)


def test_evaluate_entry_points_reject_bad_arguments_without_gpu():
    lib = L.lib()
    fr = L.EvalFrame()
    buf = (ctypes.c_float * 16)()
    for thresh, mode in ((0.0, 1), (-1.0, 1), (0.0, 2), (0.0, -1)):
        assert lib.dcmt_evaluate_dev(None, buf, buf, 4, 4, 1, thresh, mode, ctypes.byref(fr), None) == L.E_INVALID
        assert lib.dcmt_evaluate_u16_dev(None, buf, 1.0 / 256, buf, 4, 4, 1, thresh, mode, ctypes.byref(fr), None) == L.E_INVALID
        assert lib.dcmt_evaluate(None, buf, 16, buf, 16, 4, 4, thresh, mode, ctypes.byref(fr)) == L.E_INVALID
    assert lib.dcmt_evaluate_dev(None, None, None, 4, 4, 1, 0.0, 1, None, None) == L.E_INVALID
    assert lib.dcmt_evaluate_u16_dev(None, None, 1.0, None, 4, 4, 1, 0.0, 0, None, None) == L.E_INVALID
    assert lib.dcmt_evaluate(None, None, 16, None, 16, 4, 4, 0.0, 0, None) == L.E_INVALID
    with pytest.raises(ValueError):
        api._eval_mode("rmse")
    with pytest.raises(ValueError):
        api.reference_performance(np.zeros(7), "kitti")


def test_eval_summary_units_nan_and_batch_aggregates():
    sums = np.array([[4, -2.0, 6.0, 10.0, 2, 0.004, 0.00001],
                     [0, 0, 0, 0, 0, 0, 0],                           # empty mask
                     [2, 1.0, 1.0, 0.5, 2, 0.002, 0.000002]], dtype=np.float64)
    s = api.eval_summary(sums)
    pf = s["per_frame"]
    assert np.allclose(pf["me"][[0, 2]], [-0.5, 0.5]) and np.allclose(pf["mae"][[0, 2]], [1.5, 0.5])
    assert np.allclose(pf["rmse"][[0, 2]], [math.sqrt(2.5), 0.5])
    assert np.allclose(pf["imae"][[0, 2]], [2.0, 1.0])                 # 1/m -> 1/km
    assert np.allclose(pf["irmse"][[0, 2]], [1000 * math.sqrt(0.000005), 1.0])
    for k in ("me", "mae", "rmse", "imae", "irmse"):
        assert math.isnan(pf[k][1]), k
    assert list(pf["n"]) == [4, 0, 2] and list(pf["n_inv"]) == [2, 0, 2]
    pw = s["pixel_weighted"]
    assert math.isclose(pw["me"], -1 / 6) and math.isclose(pw["mae"], 7 / 6) and math.isclose(pw["rmse"], math.sqrt(10.5 / 6))
    assert math.isclose(pw["imae"], 1000 * 0.006 / 4) and math.isclose(pw["irmse"], 1000 * math.sqrt(0.000012 / 4))
    fm = s["frame_mean"]                                                # the empty frame does not count
    assert math.isclose(fm["me"], 0.0, abs_tol=1e-15) and math.isclose(fm["mae"], 1.0)
    assert math.isclose(fm["rmse"], (math.sqrt(2.5) + 0.5) / 2) and math.isclose(fm["imae"], 1.5)
    one = api.eval_summary(sums[0])                                     # a single frame's [7]
    assert one["per_frame"]["mae"].shape == (1,) and one["pixel_weighted"]["mae"] == 1.5
    empty = api.eval_summary(np.zeros(7))
    assert all(math.isnan(v) for v in empty["pixel_weighted"].values()) and all(math.isnan(v) for v in empty["frame_mean"].values())


def test_reference_presets_do_their_final_arithmetic_in_f32():
    f32 = np.float32
    s = np.array([7, -1.0 / 7.0, 1.0 / 7.0, 2.0 ** 24 + 1.0, 7, 0, 0])
    lo = api.reference_performance(s, "lidar_only")
    assert isinstance(lo, np.float32) and lo == f32(-1.0 / 7.0) / f32(7)
    rmse, mae = api.reference_performance(s, "lidar_camera")          # LC returns (mse = RMSE, mae)
    assert mae == f32(1.0 / 7.0) / f32(7) and mae != f32(1.0 / 49.0)   # float(sum) / count, not the f64 quotient rounded
    assert rmse == np.sqrt(f32(2.0 ** 24) / f32(7))                    # float(2^24 + 1) == 2^24: the f64 sum is rounded first
    mae2, rmse2 = api.reference_performance(s, "stereo_lidar")         # SL returns (mae, rmse)
    assert (mae2, rmse2) == (mae, rmse) and rmse2.dtype == np.float32
    with np.errstate(invalid="ignore"):
        assert np.isnan(api.reference_performance(np.zeros(7), "lidar_only"))
    batch = api.reference_performance(np.stack([s, np.zeros(7), s]), "stereo_lidar")
    assert batch[0].shape == (3,) and np.isnan(batch[0][1]) and batch[0][2] == mae
    assert api.EVAL_PRESETS == {"lidar_only": ("gt", 0.0), "lidar_camera": ("both", 0.0), "stereo_lidar": ("both", 2.0)}


# ---------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, 375, 1242, 16)
    yield c
    c.close()


def preds_for(c, gt):
    """A dense plane per GT frame: the GT with 25-85 % of its valid pixels dropped (varied per frame), through the cascade."""
    import torch
    sub = gt.copy()
    for i in range(sub.shape[0]):
        rng = np.random.default_rng(100 + i)
        sub[i][rng.random(sub[i].shape) < 0.25 + 0.04 * i] = 0
    out = c.complete_dev(torch.from_numpy(sub).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@gpu
def test_counts_and_sums_against_fsum(ctx):
    import torch
    for rows, cols in ((352, 1216), (375, 1242)):
        gt = synth.synth_batch(16, rows, cols, 40) * np.linspace(0.8, 1.2, 16, dtype=np.float32)[:, None, None]
        gt[5, :100] = 0
        gt[9] = 0                                                       # empty mask
        pred = preds_for(ctx, gt)
        pred[3, 200:220] = 0
        pred[4, 10:30, 100:300] = -1.5                                  # pred <= 0 inside the GT mask
        dg, dp = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
        for mode in ("gt", "both"):
            for thresh in (0.0, 2.0):
                got = ctx.evaluate_dev(dg, dp, thresh, mode).cpu().numpy()
                assert got.shape == (16, 7) and got.dtype == np.float64
                for i in range(16):
                    check_sums(got[i], gt[i], pred[i], thresh, mode, f"{rows}x{cols} {mode} {thresh} frame {i}")
                assert not got[9].any()


def ref_lo(G, R):
    """Literal port of LO main.cpp:16-34 (float running sum, row-major)."""
    tol = 0
    s, count = np.float32(0), 0
    for i in range(G.shape[0]):
        for j in range(G.shape[1]):
            gv = G[i, j]
            if gv > np.float32(tol):
                s = np.float32(s + np.float32(gv - R[i, j]))
                count += 1
    return np.float32(s / np.float32(count))


def ref_lc_sl(G, R, tol):
    """Literal port of LC main_lc.cpp:85-116 (tol = int(0.1) = 0) / SL main_sl.cpp:1031-1061 (tol = 2): (rmse, mae)."""
    s_mse, s_mae, count = np.float32(0), np.float32(0), 0
    for i in range(G.shape[0]):
        for j in range(G.shape[1]):
            gv, rv = G[i, j], R[i, j]
            if gv > np.float32(tol) and rv > np.float32(tol):
                d = np.float32(abs(np.float32(gv - rv)))
                s_mse = np.float32(s_mse + np.float32(d * d))
                s_mae = np.float32(s_mae + d)
                count += 1
    return np.float32(np.sqrt(np.float32(s_mse / np.float32(count)))), np.float32(s_mae / np.float32(count))


@gpu
def test_presets_equal_the_reference_float_loops_where_those_are_exact():
    import torch
    rng = np.random.default_rng(7)
    rows, cols = 40, 56
    gt = (rng.integers(64, 256 * 40, size=(rows, cols)) / 256.0).astype(np.float32)
    gt[rng.random((rows, cols)) < 0.85] = 0                          # sparse GT
    gt[0, :8] = np.array([1.0, 1.5, 2.0, 2.00390625, 3, 0.5, 1.99609375, 2.5], np.float32)
    pred = (gt + rng.integers(-4, 5, size=(rows, cols)) / 256.0).astype(np.float32)
    pred[rng.random((rows, cols)) < 0.1] = 0                          # LO counts these, LC / SL do not
    pred[0, :8] = np.array([2.5, 1.0, 3.0, 2.0, 1.5, 0.0, 2.00390625, 2.5], np.float32)
    want = {"lidar_only": ref_lo(gt, pred), "lidar_camera": ref_lc_sl(gt, pred, int(0.1))}
    r, m = ref_lc_sl(gt, pred, 2)
    want["stereo_lidar"] = (m, r)
    dg, dp = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
    for preset, w in want.items():
        for got in (api.evaluate_performance(gt, pred, preset), api.evaluate_performance(dg, dp, preset)):
            assert np.array_equal(np.atleast_1d(np.asarray(got, np.float32)).view(np.uint32),
                                  np.atleast_1d(np.asarray(w, np.float32)).view(np.uint32)), (preset, got, w)


@gpu
def test_sums_do_not_depend_on_batch_position_alignment_or_run():
    import torch
    rows, cols = 375, 1242                                           # rows * cols % 4 == 2: frame starts alternate 16 / 8-byte alignment
    n = rows * cols
    gt = synth.synth_batch(7, rows, cols, 60)
    pred = synth.synth_batch(7, rows, cols, 61) + np.float32(0.25)
    with api.Context(0, rows, cols, 7) as c:
        dg, dp = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
        full = c.evaluate_dev(dg, dp).cpu().numpy()
        again = c.evaluate_dev(dg, dp).cpu().numpy()
        assert np.array_equal(bits64(full), bits64(again))
        # a flat buffer with the frames at element offsets 1 and 3 (4-byte aligned starts)
        fg = torch.zeros(8 * n + 8, dtype=torch.float32, device="cuda")
        fp = torch.zeros(8 * n + 8, dtype=torch.float32, device="cuda")
        for i in range(7):
            one = c.evaluate_dev(dg[i], dp[i]).cpu().numpy()
            assert np.array_equal(bits64(one[0]), bits64(full[i])), f"frame {i} alone"
            for pos in (1, 2):
                order = [(i + 1) % 7, (i + 2) % 7]
                order.insert(pos, i)
                three = c.evaluate_dev(dg[order].contiguous(), dp[order].contiguous()).cpu().numpy()
                assert np.array_equal(bits64(three[pos]), bits64(full[i])), f"frame {i} at position {pos} of 3"
            for off in (1, 3):
                g1 = fg[off:off + n].view(rows, cols)
                p1 = fp[off:off + n].view(rows, cols)
                g1.copy_(dg[i]); p1.copy_(dp[i])
                odd = c.evaluate_dev(g1, p1).cpu().numpy()
                assert np.array_equal(bits64(odd[0]), bits64(full[i])), f"frame {i} at element offset {off}"
        for i in (0, 3, 6):
            check_sums(full[i], gt[i], pred[i], 0.0, "both", f"frame {i}")


@gpu
def test_uint16_ground_truth_equals_the_converted_plane():
    import torch
    rows, cols = 352, 1216
    u16 = np.round(synth.synth_batch(4, rows, cols, 80) * 256.0).astype(np.uint16)
    u16[0, 100, 100:110] = 0
    u16[1, 200, 300:310] = 1
    u16[2, 150, 10:20] = 65535
    u16[3] = 0
    pred = synth.synth_batch(4, rows, cols, 81) + np.float32(0.5)
    dp = torch.from_numpy(pred).cuda()
    with api.Context(0, rows, cols, 4) as c:
        for scale in (1.0 / 256.0, 1.0 / 100.0):
            conv = (u16.astype(np.float32) * np.float32(scale)).astype(np.float32)
            for mode, thresh in (("gt", 0.0), ("both", 0.0), ("both", 2.0)):
                got16 = c.evaluate_dev(torch.from_numpy(u16.view(np.int16)).cuda(), dp, thresh, mode, gt_scale=scale).cpu().numpy()
                got32 = c.evaluate_dev(torch.from_numpy(conv).cuda(), dp, thresh, mode).cpu().numpy()
                assert np.array_equal(bits64(got16), bits64(got32)), (scale, mode, thresh)
                check_sums(got16[2], conv[2], pred[2], thresh, mode, f"u16 scale {scale}")
            assert not got16[3].any()


@gpu
def test_odd_shapes_and_edge_cases(ctx):
    import torch
    rng = np.random.default_rng(11)
    for rows, cols in ((1, 1), (1, 1216), (352, 1), (5, 7), (3, 3), (2, 5), (7, 11), (1, 3), (375, 1242)):
        b = 3
        gt = (rng.integers(0, 256 * 30, size=(b, rows, cols)) / 256.0).astype(np.float32)
        gt[rng.random(gt.shape) < 0.5] = 0
        pred = (rng.random((b, rows, cols)) * 30.0).astype(np.float32)
        pred[rng.random(gt.shape) < 0.2] = 0
        gt[:, 0, 0] = 5.0                                            # at least one masked pixel per frame
        dg, dp = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
        for mode in ("gt", "both"):
            got = ctx.evaluate_dev(dg, dp, 0.0, mode).cpu().numpy()
            for i in range(b):
                check_sums(got[i], gt[i], pred[i], 0.0, mode, f"{rows}x{cols} {mode} frame {i}")
    x = synth.synth_batch(2, 352, 1216, 90)
    dx = torch.from_numpy(x).cuda()
    z = torch.zeros_like(dx)
    assert not ctx.evaluate_dev(z, dx, 0.0, "gt").cpu().numpy().any()              # all-zero GT: all zeros
    same = ctx.evaluate_dev(dx, dx, 0.0, "both").cpu().numpy()                       # gt == pred: no error
    assert (same[:, 0] == (x > 0).reshape(2, -1).sum(1)).all() and (same[:, 0] == same[:, 4]).all()
    assert not same[:, [1, 2, 3, 5, 6]].any()
    pz = x.copy()
    pz[:, 100:200] = 0
    pz[:, 200:210] = -3.0
    g = ctx.evaluate_dev(dx, torch.from_numpy(pz).cuda(), 0.0, "gt").cpu().numpy()   # GT mode: pred <= 0 counts in n, not in n_inv
    nz = (x > 0).reshape(2, -1).sum(1)
    assert (g[:, 0] == nz).all()
    assert (g[:, 4] == ((x > 0) & (pz > 0)).reshape(2, -1).sum(1)).all() and (g[:, 4] < g[:, 0]).all()
    for i in range(2):
        check_sums(g[i], x[i], pz[i], 0.0, "gt", f"pred <= 0 frame {i}")
    # argument checks on a live context
    lib = L.lib()
    out = torch.zeros((2, 8), dtype=torch.float64, device="cuda")
    args = lambda **kw: dict(dict(g=dx.data_ptr(), p=dx.data_ptr(), r=352, c=1216, b=2, t=0.0, m=1, o=out.data_ptr()), **kw)
    def call(a):
        return lib.dcmt_evaluate_dev(ctx._h, a["g"], a["p"], a["r"], a["c"], a["b"], ctypes.c_float(a["t"]), a["m"], a["o"], None)
    assert call(args()) == L.OK
    for bad in (dict(t=-0.5), dict(m=2), dict(o=out.data_ptr() + 4), dict(o=None), dict(g=None), dict(p=None), dict(b=17),
                dict(r=376), dict(c=0), dict(t=float("inf"))):
        assert call(args(**bad)) == L.E_INVALID, bad
    torch.cuda.synchronize()


@gpu
def test_host_entry_with_padded_rows_equals_the_device_entry(ctx):
    import torch
    gt = synth.synth_batch(2, 375, 1242, 95)
    pred = synth.synth_batch(2, 375, 1242, 96) + np.float32(1.0)
    for i in range(2):
        wg = np.zeros((375, 1300), np.float32)
        wp = np.full((375, 1280), 7.0, np.float32)
        wg[:, :1242] = gt[i]
        wp[:, :1242] = pred[i]
        for mode, thresh in (("gt", 0.0), ("both", 2.0)):
            host = ctx.evaluate(wg[:, :1242], wp[:, :1242], thresh, mode)
            dev = ctx.evaluate_dev(torch.from_numpy(gt[i]).cuda(), torch.from_numpy(pred[i]).cuda(), thresh, mode).cpu().numpy()[0]
            assert np.array_equal(bits64(host), bits64(dev)), (i, mode)
            check_sums(host, gt[i], pred[i], thresh, mode, f"host frame {i}")


@gpu
def test_chained_behind_completions_on_one_stream_keeps_the_context_state(monkeypatch):
    from oracle import oracle as O
    import torch
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")                    # read by dcmt_create: the 16-bit form at batch 16
    n = 16
    frames = synth.synth_batch(n, 352, 1216, 1300)
    assert np.array_equal(np.round(frames * 256) / 256, frames)       # on the KITTI grid
    gt = synth.synth_batch(n, 352, 1216, 1400)
    labs = np.stack([synth.synth_labels(352, 1216, 1200, 1300 + i)[0] for i in range(n)])
    nl = synth.synth_labels(352, 1216, 1200, 1300)[1]
    with api.Context(0, 352, 1216, n) as c:
        d, dg, dl = torch.from_numpy(frames).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(labs).cuda()
        o1 = c.complete_dev(d)
        assert "k_fp_q" in c.last_path(), c.last_path()
        e1 = c.evaluate_dev(dg, o1, 0.0, "both")
        o2 = c.complete_dev(d)
        assert "k_fp_q" in c.last_path(), c.last_path()               # the evaluation did not move the 16-bit state
        e2 = c.evaluate_dev(dg, o2, 2.0, "gt")
        o3 = c.complete_dev(d, params=api.make_params(normalize=(0, 80)))
        e3 = c.evaluate_dev(dg, o3, 2.0, "both")
        o4 = c.complete_dev(d, d_labels=dl, n_labels=nl)
        e4 = c.evaluate_dev(dg, o4, 0.0, "gt")
        torch.cuda.synchronize()
        outs = [o.cpu().numpy() for o in (o1, o2, o3, o4)]
        evs = [e.cpu().numpy() for e in (e1, e2, e3, e4)]
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    for i in (0, 15):
        want = O.img_completion(frames[i])
        assert_bit_equal(outs[0][i], want, f"first completion frame {i}")
        assert_bit_equal(outs[1][i], want, f"completion behind an evaluation frame {i}")
        assert_bit_equal(outs[2][i], O.img_completion(O.normalize_minmax(frames[i], 0, 80)), f"normalised completion frame {i}")
        assert_bit_equal(outs[3][i], O.interpolate_with_superpixels(frames[i], labs[i], nl), f"labeled completion frame {i}")
    for k, (thresh, mode) in enumerate(((0.0, "both"), (2.0, "gt"), (2.0, "both"), (0.0, "gt"))):
        for i in (0, 7, 15):
            check_sums(evs[k][i], gt[i], outs[k][i], thresh, mode, f"evaluation {k} frame {i}")
