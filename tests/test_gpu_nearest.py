"""Nearest-wins projection and reprojection on the device (dcmt_project_points_nearest*, dcmt_reproject_depth_nearest* through the
`nearest=True` keyword of api.Context).  Every comparison is bit for bit against the numpy restatement of
tests/nearest_restatement.py on its tiny inputs; tests/test_nearest.py shows without a GPU that on these inputs the two rules give
the same occupancy and differ in at least half of the occupied pixels, so a device that still answered last-wins would fail here.

Shapes: outputs of 3 x 5x7 = 105 pixels (odd: the scalar fix-up), 3 x 6x7 = 126 (pairs), 3 x 8x16 = 384 (quads), and the last one
4 bytes off a 16-byte boundary (the alignment fallback); sweeps of 800, 0 and 700 points (six scatter workgroups, an empty sweep, a
frame boundary inside the wave of points 768..831); reprojection sources of 9x13 and 16x24 (one scatter workgroup per frame)."""
import ctypes

import numpy as np
import pytest

import nearest_restatement as R
import test_gpu_stream_order as SO
from conftest import assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

gpu = pytest.mark.gpu
f32 = np.float32
FILL = -77.0


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, 64, 96, 8)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the shared inputs are read-only)


def host(t):
    return t.cpu().numpy()


def offset_view(shape, off, guard=32):
    """(buffer, view): a filled f32 buffer and a view of `shape` that starts `off` elements behind a 16-byte boundary."""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard + 8,), FILL, dtype=torch.float32, device="cuda")
    view = buf[guard + off:guard + off + n].view(*shape)
    assert view.data_ptr() % 16 == 4 * off
    return buf, view


def check_guards(buf, view, what):
    h = host(buf)
    first = (view.data_ptr() - buf.data_ptr()) // 4
    assert (h[:first] == FILL).all() and (h[first + view.numel():] == FILL).all(), f"{what}: written outside the output"


def project_table(records):
    return api.make_project_calib(np.stack([r[0] for r in records]), np.stack([r[1] for r in records]))


def reproject_table(recs):
    return api.make_reproject_calib(np.stack([r["M"] for r in recs]), np.stack([r["K"] for r in recs]), [r["fx"] for r in recs],
                                    [r["fy"] for r in recs], [r["cx"] for r in recs], [r["cy"] for r in recs])


def params_of(rec):
    return api.make_reproject_params(**rec)


def reproject_records(src, dst, mat):
    return R.reproject_record(src, dst, mat), [R.reproject_record(src, dst, m, k) for k, m in enumerate((mat, "small", "shift"))]


# ---------------------------------------------------------------------------------------------------------------- projection
@gpu
@pytest.mark.parametrize("rows,cols,off", [(5, 7, 0), (6, 7, 0), (8, 16, 0), (8, 16, 1)])
def test_projection_uniform_and_table_against_the_restatement(ctx, rows, cols, off):
    inp = R.project_inputs(rows, cols)
    pts, offsets, recs = inp["points"], inp["offsets"], inp["records"]
    d_pts, d_off = dev(pts), dev(offsets)
    what = f"{rows}x{cols}, output offset {off}"
    # one record for all sweeps
    buf, view = offset_view((3, rows, cols), off)
    ctx.project_points_dev(d_pts, d_off, *recs[0], rows, cols, view, nearest=True)
    uniform = host(view)
    assert_bit_equal(uniform, R.project_batch(pts, offsets, *recs[0], rows, cols), f"{what}: uniform call")
    check_guards(buf, view, what)
    assert not uniform[1].any()
    # a record per sweep; frame f is the uniform call on frame f alone with record f
    Ts, Ps = [r[0] for r in recs], [r[1] for r in recs]
    want = R.project_batch(pts, offsets, Ts, Ps, rows, cols)
    table = project_table(recs)
    buf, view = offset_view((3, rows, cols), off)
    ctx.project_points_calib_dev(d_pts, d_off, api.calib_to_device(table), rows, cols, view, nearest=True)
    got = host(view)
    assert_bit_equal(got, want, f"{what}: table call")
    check_guards(buf, view, what)
    for f in range(3):
        n = int(offsets[f + 1] - offsets[f])
        one = dev(pts[offsets[f]:offsets[f + 1]]) if n else dev(np.zeros((1, 4), f32))[:0]
        alone = host(ctx.project_points_dev(one, dev(np.array([0, n], np.int32)), *recs[f], rows, cols, nearest=True))[0]
        assert_bit_equal(got[f], alone, f"{what}: frame {f} against the uniform call on the frame alone")
    # a NaN in record 2: that frame is zero, the others are unchanged
    table["P"][2, 6] = np.nan
    bad = host(ctx.project_points_calib_dev(d_pts, d_off, api.calib_to_device(table), rows, cols, nearest=True))
    assert want[2].any() and not bad[2].any()
    assert_bit_equal(bad[:2], want[:2], f"{what}: the frames beside a bad record")
    assert_bit_equal(host(d_pts), pts, "the points")


@gpu
def test_projection_without_points_gives_zeros(ctx):
    import torch
    rows, cols = 5, 7
    T, P = R.project_record(rows, cols)
    empty = torch.zeros((1, 4), dtype=torch.float32, device="cuda")[:0]
    for b in (1, 3):
        off = dev(np.zeros(b + 1, np.int32))
        buf, view = offset_view((b, rows, cols), 0)
        ctx.project_points_dev(empty, off, T, P, rows, cols, view, nearest=True)
        assert not host(view).view(np.uint32).any()
        check_guards(buf, view, "no points")
        out = host(ctx.project_points_calib_dev(empty, off, api.calib_to_device(project_table([(T, P)] * b)), rows, cols, nearest=True))
        assert not out.view(np.uint32).any()


# ---------------------------------------------------------------------------------------------------------------- reprojection
@gpu
@pytest.mark.parametrize("src,dst", R.REPROJECT_SHAPES)
@pytest.mark.parametrize("mat", list(R.REPROJECT_MATS))
def test_reprojection_uniform_and_table_against_the_restatement(ctx, src, dst, mat):
    frames = R.reproject_inputs(src)
    one, recs = reproject_records(src, dst, mat)
    d_src = dev(frames)
    what = f"{src} -> {dst}, {mat}"
    for off in (0, 1):
        buf, view = offset_view((3,) + dst, off)
        ctx.reproject_depth_dev(d_src, *dst, params_of(one), view, nearest=True)
        assert_bit_equal(host(view), R.reproject_batch(frames, *dst, one), f"{what}: uniform call, output offset {off}")
        check_guards(buf, view, what)
    want = R.reproject_batch(frames, *dst, recs)
    table = reproject_table(recs)
    buf, view = offset_view((3,) + dst, 0)
    ctx.reproject_depth_calib_dev(d_src, *dst, api.calib_to_device(table), view, nearest=True)
    got = host(view)
    assert_bit_equal(got, want, f"{what}: table call")
    check_guards(buf, view, what)
    for f in range(3):
        alone = host(ctx.reproject_depth_dev(dev(frames[f]), *dst, params_of(recs[f]), nearest=True))
        assert_bit_equal(got[f], alone, f"{what}: frame {f} against the uniform call on the frame alone")
    # record 2 with a NaN in M: that frame is zero, the others are unchanged; record 0 with fx = 0 likewise
    for f, field, at, value in ((2, "M", 9, np.nan), (0, "fx", None, 0.0)):
        t = table.copy()
        if at is None:
            t[field][f] = value
        else:
            t[field][f, at] = value
        bad = host(ctx.reproject_depth_calib_dev(d_src, *dst, api.calib_to_device(t), nearest=True))
        assert not bad[f].any()
        keep = [g for g in range(3) if g != f]
        assert_bit_equal(bad[keep], want[keep], f"{what}: the frames beside bad record {f}")
    assert want[2].any()
    assert_bit_equal(host(d_src), frames, "the source planes")


# ---------------------------------------------------------------------------------------------------------------- refusals
@gpu
def test_overlapping_and_misaligned_buffers_are_refused_and_nothing_is_written(ctx):
    import torch
    lib = L.lib()
    rows, cols, b, n = 8, 16, 3, 1500
    T, P = (np.ascontiguousarray(m).ravel() for m in R.project_record(rows, cols))
    arena = torch.full((1 << 16,), FILL, dtype=torch.float32, device="cuda")
    a = arena.data_ptr()
    assert a % 16 == 0
    pts, off, tab, depth, out = a, a + 0x8000, a + 0x9000, a + 0xA000, a + 0x10000
    ob, pb, fb = 4 * b * rows * cols, 16 * n, 4 * (b + 1)
    tp, pp = T.ctypes.data, P.ctypes.data

    def proj(points, offsets, sparse, table=None):
        if table is None:
            return lib.dcmt_project_points_nearest_dev(ctx._h, points, offsets, n, b, tp, pp, sparse, rows, cols, None)
        return lib.dcmt_project_points_nearest_calib_dev(ctx._h, points, offsets, n, b, table, sparse, rows, cols, None)

    for args in ((pts, off, pts), (pts, off, pts + pb - 4), (pts, off, pts + 1600), (pts + ob - 16, off, pts), (pts, off, off), (pts, off, off + fb - 4),
                 (pts, off + ob - 4, off), (pts, off, tab, tab), (pts, off, tab + 96 * b - 4, tab), (pts, off, tab - ob + 16, tab),
                 (pts + 4, off, out), (pts, off + 2, out), (pts, off, out + 2), (pts, off, out, tab + 8), (0, off, out), (pts, 0, out), (pts, off, 0)):
        assert proj(*args) == L.E_INVALID, [hex(x - a) if x else x for x in args]
    rp = params_of(R.reproject_record((16, 24), (rows, cols)))
    db = 4 * b * 16 * 24

    def reproj(src, dst, table=None):
        if table is None:
            return lib.dcmt_reproject_depth_nearest_dev(ctx._h, src, 16, 24, b, ctypes.byref(rp), dst, rows, cols, None)
        return lib.dcmt_reproject_depth_nearest_calib_dev(ctx._h, src, 16, 24, b, table, dst, rows, cols, None)

    for args in ((depth, depth), (depth, depth + db - 4), (depth, depth + 400), (depth + ob - 4, depth), (depth, tab, tab), (depth, tab + 136 * b - 4, tab),
                 (depth, tab - ob + 8, tab), (depth + 2, out), (depth, out + 2), (depth, out, tab + 4), (0, out), (depth, 0)):
        assert reproj(*args) == L.E_INVALID, [hex(x - a) if x else x for x in args]
    bad = api.make_reproject_params(M=R.REPROJECT_MATS["small"])
    bad.M[6] = float("nan")
    assert lib.dcmt_reproject_depth_nearest_dev(ctx._h, depth, 16, 24, b, ctypes.byref(bad), out, rows, cols, None) == L.E_INVALID
    assert lib.dcmt_reproject_depth_nearest_dev(ctx._h, depth, 16, 24, 9, ctypes.byref(rp), out, rows, cols, None) == L.E_INVALID      # beyond max_batch
    assert lib.dcmt_project_points_nearest_dev(ctx._h, pts, off, n, b, tp, pp, out, 65, cols, None) == L.E_INVALID                    # beyond max_rows
    torch.cuda.synchronize()
    assert (host(arena) == FILL).all(), "a refused call wrote something"
    # the neighbours of every refusal above are accepted: the output right behind and right in front of an input
    arena.zero_()
    assert proj(pts, off, pts + pb) == L.OK and proj(pts, off, off + fb) == L.OK and proj(pts, off, tab + 96 * b, tab) == L.OK
    assert reproj(depth, depth + db) == L.OK and reproj(depth + ob, depth) == L.OK and reproj(depth, tab + 136 * b + 8, tab + 8) == L.OK
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- carried state
@gpu
def test_nearest_calls_leave_the_carried_state_alone_and_mix_with_last_wins_calls():
    """One context; last, nearest, last, nearest, ... of both kinds, in both orders, repeatedly, with one last-wins reprojection
    into a larger plane in between (the winner plane grows: reallocated, cleared, its generation starts again).  Every output is its
    own restatement's, and what the cascade left -- dcmt_last_path, the fill-iteration and hole probes -- is what it was."""
    import torch
    rows, cols = 8, 16
    src, dst = (16, 24), (8, 16)
    inp = R.project_inputs(rows, cols)
    pts, offsets, (T, P) = inp["points"], inp["offsets"], inp["records"][0]
    frames = R.reproject_inputs(src)
    rec = R.reproject_record(src, dst, "shift")
    big = R.reproject_record(src, (40, 70), "small")
    want = {("p", True): R.project_batch(pts, offsets, T, P, rows, cols), ("p", False): R.project_last(pts, offsets, T, P, rows, cols),
            ("r", True): R.reproject_batch(frames, *dst, rec), ("r", False): R.reproject_last(frames, *dst, rec)}
    want_big = R.reproject_last(frames, 40, 70, big)
    d_pts, d_off, d_src = dev(pts), dev(offsets), dev(frames)
    x = synth.synth_batch(3, 48, 64, 5)
    with api.Context(0, 48, 96, 3) as c:
        c.complete_dev(dev(x))
        torch.cuda.synchronize()
        probes = lambda: (c.last_path(), c.last_fill_iters(3), c.last_holes_after_extend(3))
        before = probes()
        assert before[0]

        def call(kind, nearest):
            if kind == "p":
                return c.project_points_dev(d_pts, d_off, T, P, rows, cols, nearest=nearest)
            return c.reproject_depth_dev(d_src, *dst, params_of(rec), nearest=nearest)

        outs = []
        for rnd, order in enumerate((("p", "r"), ("r", "p"), ("p", "r"))):
            for first in (False, True):                                # last, nearest, last, nearest ... then nearest, last, ...
                for kind in order:
                    for nearest in (first, not first):
                        outs.append(((kind, nearest), call(kind, nearest)))
                        if nearest:
                            assert probes() == before, "a nearest call changed what the probes report"
            if rnd == 0:
                outs.append(("big", c.reproject_depth_dev(d_src, 40, 70, params_of(big))))
        torch.cuda.synchronize()
        assert len(outs) == 25
        for i, (k, t) in enumerate(outs):
            assert_bit_equal(host(t), want_big if k == "big" else want[k], f"call {i}: {k}")
        assert probes() == before
    assert not np.array_equal(want[("p", True)].view(np.uint32), want[("p", False)].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- host forms
@gpu
def test_host_forms_equal_the_device_call_and_leave_pitched_padding_alone(ctx):
    lib = L.lib()
    rows, cols = 5, 7
    inp = R.project_inputs(rows, cols)
    pts, offsets, (T, P) = inp["points"], inp["offsets"], inp["records"][0]
    sweep = np.ascontiguousarray(pts[:offsets[1]])
    want = host(ctx.project_points_dev(dev(sweep), dev(np.array([0, len(sweep)], np.int32)), T, P, rows, cols, nearest=True))[0]
    assert_bit_equal(want, R.project_frame(sweep, T, P, rows, cols), "device call on the sweep")
    t, p = np.ascontiguousarray(T, f32).ravel(), np.ascontiguousarray(P, f32).ravel()
    wide = np.full((rows, cols + 3), FILL, f32)
    st = lib.dcmt_project_points_nearest(ctx._h, sweep.ctypes.data, len(sweep), t.ctypes.data, p.ctypes.data, wide.ctypes.data, wide.strides[0], rows, cols)
    assert st == L.OK
    assert_bit_equal(wide[:, :cols], want, "dcmt_project_points_nearest, pitched rows")
    assert (wide[:, cols:] == FILL).all(), "the padding of the pitched rows was written"
    st = lib.dcmt_project_points_nearest(ctx._h, None, 0, t.ctypes.data, p.ctypes.data, wide.ctypes.data, wide.strides[0], rows, cols)
    assert st == L.OK and not wide[:, :cols].any() and (wide[:, cols:] == FILL).all()

    src, dst = (9, 13), (5, 7)
    frame = R.reproject_inputs(src)[0]
    rec = R.reproject_record(src, dst, "shift")
    want = host(ctx.reproject_depth_dev(dev(frame), *dst, params_of(rec), nearest=True))
    assert_bit_equal(want, R.reproject_frame(frame, *dst, rec), "device call on the frame")
    pitched = np.full((src[0], src[1] + 5), 1e30, f32)
    pitched[:, :src[1]] = frame
    assert_bit_equal(ctx.reproject_depth(pitched[:, :src[1]], *dst, params_of(rec), nearest=True), want, "Context.reproject_depth(nearest=True)")
    wide = np.full((dst[0], dst[1] + 3), FILL, f32)
    rp = params_of(rec)
    st = lib.dcmt_reproject_depth_nearest(ctx._h, pitched.ctypes.data, pitched.strides[0], *src, ctypes.byref(rp), wide.ctypes.data, wide.strides[0], *dst)
    assert st == L.OK
    assert_bit_equal(wide[:, :dst[1]], want, "dcmt_reproject_depth_nearest, pitched rows")
    assert (wide[:, dst[1]:] == FILL).all(), "the padding of the pitched rows was written"
    assert not np.array_equal(want.view(np.uint32), ctx.reproject_depth(frame, *dst, params_of(rec)).view(np.uint32)), "nearest and last-wins coincide"


@gpu
def test_unrectify_sol_nearest_equals_the_device_call(tmp_path):
    import os
    import subprocess
    import test_reproject as TR
    from conftest import ROOT
    frame = (R.reproject_inputs((16, 24))[0] * f32(0.5) + f32(3.0)).astype(f32)
    orows, ocols = 12, 20
    got = api.unrectify_sol(frame, (orows, ocols), TR.R_RECT_02, nearest=True)
    rec = dict(M=api.inverse_f32(TR.R_RECT_02), K=TR.CAMERA_MAT, fx=TR.FX, fy=TR.FY, cx=TR.CX, cy=TR.CY)
    with api.Context(0, 16, 24, 1) as c:
        want = host(c.reproject_depth_dev(dev(frame), orows, ocols, api.make_reproject_params(M=rec["M"]), nearest=True))
    assert_bit_equal(got, want, "unrectify_sol(nearest=True)")
    assert_bit_equal(got, R.reproject_frame(frame, orows, ocols, rec), "unrectify_sol(nearest=True) against the restatement")
    # ... and the cv::Mat shim, in a process of its own
    exe, lib_dir = tmp_path / "reproject_nearest_test", os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv"),
                    os.path.join(ROOT, "tests", "mock_opencv", "reproject_nearest_test.cpp"), "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip",
                    "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    frame.tofile(tmp_path / "in.f32")
    rec["M"].tofile(tmp_path / "minv.f32")
    r = subprocess.run([str(exe), "16", "24", str(tmp_path / "in.f32"), str(tmp_path / "minv.f32"), str(orows), str(ocols), str(tmp_path / "out.f32")],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert_bit_equal(np.fromfile(tmp_path / "out.f32", dtype=f32).reshape(orows, ocols), want, "dcmt_shim::unrectify_sol_nearest")


# ---------------------------------------------------------------------------------------------------------------- stream order
def dirty_then(t, name, st, fn):
    """Makes the output dirty ON THE CALL'S STREAM right in front of the call: a clear that escaped to another stream runs before
    this fill (the stream is held up by the delay), and the scatter then takes its maximum against the fill's bits."""
    import torch
    s = torch.cuda.current_stream() if st is None else (torch.cuda.ExternalStream(st) if st else torch.cuda.default_stream())
    with torch.cuda.stream(s):
        t[name].fill_(SO.fill_of(f32))
    fn()


def stream_project_case(table):
    rows, cols = 8, 16
    recs = [R.project_record(rows, cols, k) for k in range(3)]
    T, P = recs[0]
    tab_bytes = project_table(recs).view(np.uint8).reshape(3, 96)
    offs = {0: np.array([0, 800, 800, 1500], np.int32), 1: np.array([0, 500, 1500, 1500], np.int32),      # the empty sweep moves
            2: np.array([0, 0, 700, 1500], np.int32), 3: np.array([0, 400, 1100, 1500], np.int32)}        # (further sets: tests/test_gpu_graph_replay.py)

    def inputs(which):
        d = {"pts": np.array(R.project_inputs(rows, cols, seed=which)["points"]), "off": offs[which]}
        if table:
            d["tab"] = tab_bytes
        return d

    def call(ctx, t, st):
        if table:
            dirty_then(t, "sparse", st, lambda: ctx.project_points_calib_dev(t["pts"], t["off"], t["tab"], rows, cols, t["sparse"], stream=st, nearest=True))
        else:
            dirty_then(t, "sparse", st, lambda: ctx.project_points_dev(t["pts"], t["off"], T, P, rows, cols, t["sparse"], stream=st, nearest=True))

    def expect(inp):
        Ts, Ps = ([r[0] for r in recs], [r[1] for r in recs]) if table else (T, P)
        return {"sparse": R.project_batch(inp["pts"], inp["off"], Ts, Ps, rows, cols)}

    return SO.Case(f"project_points nearest {'table' if table else 'uniform'}", (rows, cols, 3), inputs, {"sparse": SO.Out((3, rows, cols), f32)}, call, expect)


def stream_reproject_case(table):
    src, dst = (16, 24), (8, 16)
    one, recs = reproject_records(src, dst, "shift")
    tab_bytes = reproject_table(recs).view(np.uint8).reshape(3, 136)

    def inputs(which):
        x = np.array(R.reproject_inputs(src, seed=which))
        x[1] = x[2][::-1, ::-1] + f32(1.0)                                # (no all-zero frame: real and decoy must differ in every frame)
        d = {"depth": x}
        if table:
            d["tab"] = tab_bytes
        return d

    def call(ctx, t, st):
        if table:
            dirty_then(t, "out", st, lambda: ctx.reproject_depth_calib_dev(t["depth"], *dst, t["tab"], t["out"], stream=st, nearest=True))
        else:
            dirty_then(t, "out", st, lambda: ctx.reproject_depth_dev(t["depth"], *dst, params_of(one), t["out"], stream=st, nearest=True))

    def expect(inp):
        return {"out": R.reproject_batch(inp["depth"], *dst, recs if table else one)}

    return SO.Case(f"reproject_depth nearest {'table' if table else 'uniform'}", (src[0], src[1], 3), inputs, {"out": SO.Out((3,) + dst, f32)}, call, expect)


STREAM_CASES = {"project uniform": lambda: stream_project_case(False), "project table": lambda: stream_project_case(True),
                "reproject uniform": lambda: stream_reproject_case(False), "reproject table": lambda: stream_reproject_case(True)}


@gpu
@pytest.mark.parametrize("name", list(STREAM_CASES))
def test_nearest_call_queued_behind_a_delay_on_a_side_stream(name):
    """The scheme of tests/test_gpu_stream_order.py: a non-default stream held up by a delay, producer copy -> fill of the output ->
    call -> consumer copy, decoys and the fill restored behind it, no host synchronisation until the end.  The marker behind the delay
    must still be pending when the call returns."""
    SO.run_ordered(STREAM_CASES[name]())


# ---------------------------------------------------------------------------------------------------------------- repeatability
@gpu
def test_the_same_call_twice_gives_the_same_bits(ctx):
    rows, cols = 8, 16
    inp = R.project_inputs(rows, cols)
    d_pts, d_off = dev(inp["points"]), dev(inp["offsets"])
    T, P = inp["records"][0]
    a = ctx.project_points_dev(d_pts, d_off, T, P, rows, cols, nearest=True)
    _, view = offset_view((3, rows, cols), 1)
    ctx.project_points_dev(d_pts, d_off, T, P, rows, cols, view, nearest=True)
    assert_bit_equal(host(a), host(view), "projection twice, two buffers, two alignments")
    src, dst = (16, 24), (8, 16)
    d_src, rec = dev(R.reproject_inputs(src)), R.reproject_record(src, dst, "small")
    a = ctx.reproject_depth_dev(d_src, *dst, params_of(rec), nearest=True)
    _, view = offset_view((3,) + dst, 2)
    ctx.reproject_depth_dev(d_src, *dst, params_of(rec), view, nearest=True)
    assert_bit_equal(host(a), host(view), "reprojection twice, two buffers, two alignments")
