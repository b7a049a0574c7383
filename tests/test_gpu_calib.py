"""Per-frame calibration tables on the device: dcmt_project_points_calib_dev, dcmt_depth_to_cloud_calib_dev,
dcmt_reproject_depth_calib_dev, dcmt_stereo_refine_calib_dev through api.Context.*_calib_dev.

Every comparison is bit for bit, twice: against the restatement that pins the uniform call (oracle.project_points,
oracle.stereo_refine, np_reproject, np_cloud), evaluated frame by frame with the frame's own record (calib_cases.py), and against
the uniform device call made on frame f alone with record f.  test_calib.py shows, without a GPU, that every input set used here
gives different bits under any other frame's record, and that the straddling threads hold winners on both sides of a frame boundary.
The shapes are the smallest at which each indexing case occurs; they are named where they are used."""
import ctypes

import numpy as np
import pytest

import calib_cases as C
from conftest import assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

gpu = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, 352, 1216, 6)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def tab(case_or_table):
    return api.calib_to_device(getattr(case_or_table, "table", case_or_table))


def offset_view(shape, off, fill=-77.0, guard=32):
    """(buffer, view): a filled f32 buffer and a view of `shape` that starts `off` elements behind a 16-byte boundary."""
    import torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard + 8,), fill, dtype=torch.float32, device="cuda")
    return buf, buf[guard + off:guard + off + n].view(*shape)


def check_guards(buf, view, what, fill=-77.0, guard=32):
    h = host(buf)
    first = (view.data_ptr() - buf.data_ptr()) // 4
    assert (h[:first] == fill).all() and (h[first + view.numel():] == fill).all(), f"{what}: written outside the output"


# ---------------------------------------------------------------------------------------------------------------- projection
def project_alone(ctx, case, f):
    o = case.offsets
    n = int(o[f + 1] - o[f])
    d_pts = dev(case.points[o[f]:o[f + 1]]) if n else dev(np.zeros((1, 4), f32))[:0]          # (an empty sweep: no record is read)
    return host(ctx.project_points_dev(d_pts, dev(np.array([0, n], np.int32)), case.T[f], case.P[f], case.rows, case.cols))[0]


def check_project(ctx, case, got, what):
    for f in range(case.b):
        assert_bit_equal(got[f], case.want(f), f"{what}: frame {f} against the oracle with its own record")
        assert_bit_equal(got[f], project_alone(ctx, case, f), f"{what}: frame {f} against the uniform call on the frame alone")


@gpu
def test_projection_sweep_boundaries_inside_a_workgroup_and_inside_a_wave(ctx):
    """16x24, sweeps of 100, 0, 300, 37, 256 and 1 points: boundaries at points 100, 400, 437 and 693 of three workgroups, inside
    waves 1, 6, 6 and 10 of the call; one empty sweep; last-writer collisions in the tiny image."""
    case = C.cases()["project sweeps 16x24"]
    got = host(ctx.project_points_calib_dev(dev(case.points), dev(case.offsets), tab(case), case.rows, case.cols))
    check_project(ctx, case, got, case.name)
    assert not got[1].any()


@gpu
def test_projection_resolve_straddling_at_every_store_width(ctx):
    """5x7, batch 4: 140 pixels, so with 16-byte stores the thread of pixels 32..35 has three of frame 0 and one of frame 1; with the
    output one and two elements off a 16-byte boundary the stores are 4 and 8 bytes wide."""
    case = C.cases()["project straddle 5x7"]
    pts, off, t = dev(case.points), dev(case.offsets), tab(case)
    for o in (0, 1, 2):
        buf, view = offset_view((case.b, case.rows, case.cols), o)
        assert view.data_ptr() % 16 == 4 * o
        ctx.project_points_calib_dev(pts, off, t, case.rows, case.cols, d_sparse=view)
        check_project(ctx, case, host(view), f"{case.name}, output offset {o}")
        check_guards(buf, view, f"{case.name}, output offset {o}")


# ---------------------------------------------------------------------------------------------------------------- reprojection
def check_reproject(ctx, case, got, what, alone=True):
    for f in range(case.b):
        assert_bit_equal(got[f], case.want(f), f"{what}: frame {f} against np_reproject with its own record")
        if alone:
            p = api.make_reproject_params(M=case.M[f], K=case.K[f], **case.kw[f])
            one = host(ctx.reproject_depth_dev(dev(case.frames[f]), case.orows, case.ocols, p))
            assert_bit_equal(got[f], one, f"{what}: frame {f} against the uniform call on the frame alone")


@gpu
@pytest.mark.parametrize("name", ["reproject 6x9 -> 5x7", "reproject 40x50 -> 33x41"])
def test_reprojection_resolve_straddling_at_every_store_width(ctx, name):
    """Destinations of 35 and 1353 pixels, batch 4: frames end inside a thread's 4 (2) pixels.  40x50 has two scatter workgroups per
    frame.  Output offsets 0, 1, 2: 16-, 4- and 8-byte stores."""
    case = C.cases()[name]
    src, t = dev(case.frames), tab(case)
    for o in (0, 1, 2):
        buf, view = offset_view((case.b, case.orows, case.ocols), o)
        ctx.reproject_depth_calib_dev(src, case.orows, case.ocols, t, d_out=view)
        check_reproject(ctx, case, host(view), f"{name}, output offset {o}", alone=o == 0)
        check_guards(buf, view, f"{name}, output offset {o}")
    assert_bit_equal(host(src), case.frames, "the source planes")


# ---------------------------------------------------------------------------------------------------------------- cloud
def run_cloud(ctx, case, table=None, **kw):
    pts, off = ctx.depth_to_cloud_calib_dev(dev(case.frames), tab(case if table is None else table), None if case.bgr is None else dev(case.bgr), **kw)
    off = host(off)
    return C.words(host(pts[:min(int(off[-1]), pts.shape[0])])), off


def cloud_alone(ctx, case, f):
    pts, off = ctx.depth_to_cloud_dev(dev(case.frames[f]), None if case.bgr is None else dev(case.bgr[f]), params=api.make_cloud_params(**case.kw[f]))
    off = host(off)
    return C.words(host(pts[:off[1]]))


def check_cloud(ctx, case, got, off, what):
    want, woff = C.cloud_want(case)
    assert off.dtype == np.int32 and np.array_equal(off, woff), (what, off, woff)
    assert np.array_equal(got, want), f"{what}: {(got != want).any(1).sum()} of {len(want)} records differ from np_cloud with each frame's own record"
    for f in range(case.b):
        assert np.array_equal(got[off[f]:off[f + 1]], cloud_alone(ctx, case, f)), f"{what}: frame {f} against the uniform call on the frame alone"


@gpu
@pytest.mark.parametrize("name", ["cloud 96x96 colour", "cloud 96x96"])
def test_cloud_two_chunks_per_frame_with_an_all_zero_frame(ctx, name):
    """96x96 = 9216 pixels: two 8192-pixel chunks per frame, batch 4, frame 2 all zero; then the capacity rule with room for half."""
    import torch
    case = C.cases()[name]
    got, off = run_cloud(ctx, case)
    check_cloud(ctx, case, got, off, name)
    assert off[3] == off[2]
    want, woff = C.cloud_want(case)
    total = int(woff[-1])
    cap = total // 2
    buf = torch.full((16 * total + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    pts = buf[:16 * total].view(torch.float32).view(total, 4)
    _, off2 = ctx.depth_to_cloud_calib_dev(dev(case.frames), tab(case), None if case.bgr is None else dev(case.bgr), d_points=pts, capacity=cap)
    h = host(buf)
    assert np.array_equal(host(off2), woff), "the offsets are the true counts on overflow too"
    assert np.array_equal(h[:16 * cap].view(np.uint32).reshape(-1, 4), want[:cap]) and (h[16 * cap:] == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------------- stereo
def check_stereo(ctx, case, got, what):
    for f in range(case.b):
        assert_bit_equal(got[f], case.want(f), f"{what}: frame {f} against the oracle with its own record")
        one = ctx.stereo_refine_dev(dev(case.depth[f]), dev(case.left[f]), dev(case.right[f]), iterations=case.iterations, **case.rec[f])
        assert_bit_equal(got[f], host(one), f"{what}: frame {f} against the uniform call on the frame alone")


@gpu
@pytest.mark.parametrize("name", ["stereo 6x300 iterations 4", "stereo 6x300 iterations 0"])
def test_stereo_a_thread_walks_more_than_one_column(ctx, name):
    case = C.cases()[name]
    got = ctx.stereo_refine_calib_dev(dev(case.depth), dev(case.left), dev(case.right), tab(case), iterations=case.iterations)
    check_stereo(ctx, case, host(got), name)


@gpu
def test_stereo_row_beyond_lds():
    """3x49160, batch 2: the right-image row does not fit the workgroup's LDS, so the table reaches k_stereo_refine<false> too."""
    case = C.cases()["stereo 3x49160"]
    with api.Context(0, 3, 49160, 2) as c:
        got = c.stereo_refine_calib_dev(dev(case.depth), dev(case.left), dev(case.right), tab(case), iterations=case.iterations)
        check_stereo(c, case, host(got), case.name)


# ---------------------------------------------------------------------------------------------------------------- all-equal table
@gpu
def test_a_table_of_equal_records_gives_the_bits_of_the_uniform_calls(ctx):
    rows, cols, b = 64, 80, 5
    rng = np.random.default_rng(40)
    frames = dev(C.depth_frames(b, rows, cols, 41))
    bgr = dev(rng.integers(0, 256, (b, rows, cols, 3), dtype=np.uint8))
    # projection
    T, P = C.project_records(2, rows, cols)
    pc = C.project_case("equal", rows, cols, (700, 0, 900, 300, 1100), 42)
    pts, off = dev(pc.points), dev(pc.offsets)
    uni = ctx.project_points_dev(pts, off, T[1], P[1], rows, cols)
    got = ctx.project_points_calib_dev(pts, off, tab(api.make_project_calib(np.repeat(T[1:2], b, 0), np.repeat(P[1:2], b, 0))), rows, cols)
    assert (host(uni) != 0).sum() > 500
    assert_bit_equal(host(got), host(uni), "projection")
    # cloud
    kw = C.cloud_records(2, rows, cols)[1]
    up, uo = ctx.depth_to_cloud_dev(frames, bgr, params=api.make_cloud_params(**kw))
    gp, go = ctx.depth_to_cloud_calib_dev(frames, tab(C.cloud_table([kw] * b)), bgr)
    assert np.array_equal(host(go), host(uo)) and host(uo)[-1] > 1000
    n = int(host(uo)[-1])
    assert np.array_equal(C.words(host(gp[:n])), C.words(host(up[:n]))), "cloud"
    # reprojection
    M, K, rk = C.reproject_records(2, rows, cols, 60, 84)
    uni = ctx.reproject_depth_dev(frames, 60, 84, api.make_reproject_params(M=M[1], K=K[1], **rk[1]))
    got = ctx.reproject_depth_calib_dev(frames, 60, 84, tab(C.reproject_table(np.repeat(M[1:2], b, 0), np.repeat(K[1:2], b, 0), [rk[1]] * b)))
    assert (host(uni) != 0).sum() > 1000
    assert_bit_equal(host(got), host(uni), "reprojection")
    # stereo
    sc = C.stereo_case("equal", b, rows, cols, 43, 4)
    d, l, r = dev(sc.depth), dev(sc.left), dev(sc.right)
    uni = ctx.stereo_refine_dev(d, l, r, iterations=4, **sc.rec[1])
    got = ctx.stereo_refine_calib_dev(d, l, r, tab(api.make_stereo_calib([sc.rec[1]["baseline"]] * b, [sc.rec[1]["focal"]] * b)), iterations=4)
    assert_bit_equal(host(got), host(uni), "stereo")


# ---------------------------------------------------------------------------------------------------------------- bad records
def spoiled(table, field, index, value):
    """A copy of the table with record 1's `field` (entry `index` of it, for an array field) set to value."""
    t = table.copy()
    if index is None:
        t[field][1] = value
    else:
        t[field][1, index] = value
    return t


NAN, INF = float("nan"), float("inf")


@gpu
def test_a_bad_record_empties_its_frame_and_no_other(ctx):
    """Frame 1 of 3 holds, in turn, a NaN, an Inf and -- where the record has a focal length -- a zero.  These are defined inputs: the
    kernels test the record's bits before anything is computed from it, so the frame is the empty result and frames 0 and 2 are what
    they are with a good frame 1."""
    pc, rc, cc, sc = (C.cases()[n] for n in ("project 3 sweeps 12x20", "reproject 12x20 -> 10x18 batch 3", "cloud 12x20 batch 3", "stereo 8x40 batch 3"))
    # projection
    pts, off = dev(pc.points), dev(pc.offsets)
    good = host(ctx.project_points_calib_dev(pts, off, tab(pc), pc.rows, pc.cols))
    check_project(ctx, pc, good, pc.name)
    # Frame 1 owns points 256..555: the four waves of workgroup 1 lie in it and take its record on the scalar path (the record of the
    # workgroup's first frame, tested by 24 lanes and a ballot); wave 0 of workgroup 2 holds the boundary at 556 and takes the
    # per-lane path.  P's third row = +Inf is a record that would NOT empty the frame by itself: p.z = +Inf, uf = vf = 0, so every
    # point in front of the camera would land on pixel 0 and the resolve would write Inf there.
    assert pc.offsets.tolist() == [0, 256, 556, 656]
    spoils = [[("T", 5, NAN)], [("T", 11, INF)], [("P", 0, -INF)], [("P", 11, NAN)], [("P", k, INF) for k in (8, 9, 10, 11)], [("T", 0, 3e38), ("T", 1, -3e38)]]
    for spoil in spoils[:-1]:
        table = pc.table
        for field, index, value in spoil:
            table = spoiled(table, field, index, value)
        got = host(ctx.project_points_calib_dev(pts, off, tab(table), pc.rows, pc.cols))
        assert not got[1].any(), spoil
        assert_bit_equal(got[[0, 2]], good[[0, 2]], f"projection, {spoil}")
    # finite but huge: the record passes the test, the arithmetic overflows to Inf - Inf.  Defined behaviour all the same: nothing is
    # written outside the plane (the address is formed behind an integer bound) and the other frames are what they were
    table = pc.table
    for field, index, value in spoils[-1]:
        table = spoiled(table, field, index, value)
    buf, view = offset_view((pc.b, pc.rows, pc.cols), 0)
    ctx.project_points_calib_dev(pts, off, tab(table), pc.rows, pc.cols, d_sparse=view)
    assert_bit_equal(host(view)[[0, 2]], good[[0, 2]], "projection, a finite record whose products overflow")
    check_guards(buf, view, "projection, a finite record whose products overflow")
    # reprojection
    src = dev(rc.frames)
    good = host(ctx.reproject_depth_calib_dev(src, rc.orows, rc.ocols, tab(rc)))
    check_reproject(ctx, rc, good, rc.name)
    for field, index, value in (("fx", None, NAN), ("cy", None, INF), ("M", 7, NAN), ("M", 8, -INF), ("K", 4, INF), ("K", 0, NAN),
                                ("fx", None, 0.0), ("fy", None, -0.0)):
        got = host(ctx.reproject_depth_calib_dev(src, rc.orows, rc.ocols, tab(spoiled(rc.table, field, index, value))))
        assert not got[1].any(), (field, index, value)
        assert_bit_equal(got[[0, 2]], good[[0, 2]], f"reprojection, {field}[{index}] = {value}")
    got = host(ctx.reproject_depth_calib_dev(src, rc.orows, rc.ocols, tab(spoiled(spoiled(rc.table, "M", 13, NAN), "K", 7, INF))))
    assert_bit_equal(got, good, "M's 4th row and K's 3rd are never read")
    # cloud
    good, goff = run_cloud(ctx, cc)
    check_cloud(ctx, cc, good, goff, cc.name)
    for field, value in (("fx", NAN), ("cx", INF), ("fy", -INF), ("cy", NAN), ("fx", 0.0), ("fy", -0.0)):
        got, off3 = run_cloud(ctx, cc, spoiled(cc.table, field, None, value))
        assert off3[2] == off3[1] == goff[1] and off3[3] == goff[1] + goff[3] - goff[2], (field, value, off3, goff)
        assert np.array_equal(got[:off3[1]], good[:goff[1]]) and np.array_equal(got[off3[2]:off3[3]], good[goff[2]:goff[3]]), (field, value)
    # stereo
    d, l, r = dev(sc.depth), dev(sc.left), dev(sc.right)
    good = host(ctx.stereo_refine_calib_dev(d, l, r, tab(sc), iterations=4))
    check_stereo(ctx, sc, good, sc.name)
    for field, value in (("baseline", NAN), ("focal", INF), ("baseline", -INF), ("focal", NAN), ("focal", 0.0), ("focal", -0.0)):
        got = host(ctx.stereo_refine_calib_dev(d, l, r, tab(spoiled(sc.table, field, None, value)), iterations=4))
        assert not got[1].any(), (field, value)
        assert_bit_equal(got[[0, 2]], good[[0, 2]], f"stereo, {field} = {value}")


# ---------------------------------------------------------------------------------------------------------------- winner plane
@gpu
def test_table_and_uniform_calls_share_the_winner_plane():
    """A table projection, a uniform reprojection and a table reprojection on one context, in that order, nothing in between: the
    generations are shared as before."""
    import torch
    pc, rc = C.cases()["project 3 sweeps 12x20"], C.cases()["reproject 12x20 -> 10x18 batch 3"]
    with api.Context(0, 12, 20, 3) as c:
        a = c.project_points_calib_dev(dev(pc.points), dev(pc.offsets), tab(pc), pc.rows, pc.cols)
        src = dev(rc.frames)
        u = c.reproject_depth_dev(src, rc.orows, rc.ocols, api.make_reproject_params(M=rc.M[2], K=rc.K[2], **rc.kw[2]))
        t = c.reproject_depth_calib_dev(src, rc.orows, rc.ocols, tab(rc))
        torch.cuda.synchronize()
        a, u, t = host(a), host(u), host(t)
    for f in range(3):
        assert_bit_equal(a[f], pc.want(f), f"table projection, frame {f}")
        assert_bit_equal(t[f], rc.want(f), f"table reprojection, frame {f}")
        assert_bit_equal(u[f], rc.frame(f, 2), f"uniform reprojection behind the table projection, frame {f}")


# ---------------------------------------------------------------------------------------------------------------- full size
@gpu
def test_one_full_size_frame_pair(ctx):
    """352x1216, batch 2, two KITTI-like records, through the two calls whose load widths depend on size and alignment."""
    cc, rc = C.cases()["cloud 352x1216 pair"], C.cases()["reproject 352x1216 pair"]
    got, off = run_cloud(ctx, cc)
    check_cloud(ctx, cc, got, off, cc.name)
    out = host(ctx.reproject_depth_calib_dev(dev(rc.frames), rc.orows, rc.ocols, tab(rc)))
    check_reproject(ctx, rc, out, rc.name)


# ---------------------------------------------------------------------------------------------------------------- arguments
@gpu
def test_table_checks_on_a_live_context(ctx):
    import torch
    lib = L.lib()
    b, rows, cols = 2, 8, 8
    src = torch.ones((b, rows, cols), dtype=torch.float32, device="cuda")
    img = torch.zeros((b, rows, cols), dtype=torch.uint8, device="cuda")
    out = torch.zeros((b, rows, cols), dtype=torch.float32, device="cuda")
    pts = torch.zeros((b * rows * cols, 4), dtype=torch.float32, device="cuda")
    cpts = torch.ones((16, 4), dtype=torch.float32, device="cuda")
    off = torch.zeros((b + 1,), dtype=torch.int32, device="cuda")
    poff = dev(np.array([0, 8, 16], np.int32))
    table = torch.zeros((1024,), dtype=torch.uint8, device="cuda")
    table.view(torch.float32)[:] = 1.0                      # finite everywhere (as f64: 0.0078125...), so every record is good
    sp = L.StereoParams()
    lib.dcmt_default_stereo_params(ctypes.byref(sp))
    calls = {
        "project": lambda t, o=out.data_ptr(): lib.dcmt_project_points_calib_dev(ctx._h, cpts.data_ptr(), poff.data_ptr(), 16, b, t, o, rows, cols, None),
        "cloud": lambda t, o=pts.data_ptr(), f=off.data_ptr(): lib.dcmt_depth_to_cloud_calib_dev(ctx._h, src.data_ptr(), None, rows, cols, b, t, o, pts.shape[0], f, None),
        "reproject": lambda t, o=out.data_ptr(): lib.dcmt_reproject_depth_calib_dev(ctx._h, src.data_ptr(), rows, cols, b, t, o, rows, cols, None),
        "stereo": lambda t, o=out.data_ptr(): lib.dcmt_stereo_refine_calib_dev(ctx._h, src.data_ptr(), img.data_ptr(), img.data_ptr(), o, rows, cols, b,
                                                                                ctypes.byref(sp), t, None),
    }
    rec = {"project": 96, "cloud": 32, "reproject": 136, "stereo": 8}
    at = table.data_ptr()
    assert at % 16 == 0
    for name, call in calls.items():
        assert call(at) == L.OK, name
        assert call(None) == L.E_INVALID, name
        assert call(at + 4) == L.E_INVALID, name                         # 4-byte aligned only
        if name == "project":
            assert call(at + 8) == L.E_INVALID                           # 16 bytes for the 96-byte records
        else:
            assert call(at + 8) == L.OK, name
        # the table inside the output, and the output's last byte inside the table
        o = out if name != "cloud" else pts
        assert call(o.data_ptr() + 16, o.data_ptr()) == L.E_INVALID, name
        assert call(at, at + b * rec[name] - 16) == L.E_INVALID, name
    assert calls["cloud"](at, pts.data_ptr(), at + 32 * b - 4) == L.E_INVALID      # d_offsets inside the table
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- stream order
def _none(_):
    """A Case's call returns the outputs the wrapper created, or None: here every output is a buffer of the case's."""
    return None


_stream_sets = {}


def _stream_set(kind, which):
    """calib_cases.stream_case(kind, which): sets 0 and 1 are the ones test_calib.py checks without a GPU; further sets (tests/
    test_gpu_graph_replay.py) come from the same generator with further seeds."""
    if which in (0, 1):
        return C.cases()[f"stream {kind} 24x40 {'decoy' if which else 'real'}"]
    if (kind, which) not in _stream_sets:
        _stream_sets[kind, which] = C.stream_case(kind, which)
    return _stream_sets[kind, which]


def _ordered_case(kind, name, dims, inputs_of, outputs, call, expect_of):
    """A test_gpu_stream_order.Case whose inputs (the table among them) are calib_cases.stream_case(kind, which): the sets that
    test_calib.py checks, without a GPU, to tell every frame's record from every other."""
    import test_gpu_stream_order as S
    seen = {}

    def inputs(which):
        c = seen[which] = _stream_set(kind, which)
        d = inputs_of(c)
        d["calib"] = c.table.view(np.uint8).reshape(c.b, -1)
        return d

    def expect(inp):
        for c in seen.values():
            if c.table.tobytes() == inp["calib"].tobytes() and all(np.array_equal(v, inp[k]) for k, v in inputs_of(c).items()):
                return expect_of(c, c.want)
        raise AssertionError("unknown input set")

    return S.Case(name, dims, inputs, outputs, call, expect)


def stream_order_case(which):
    """The stream-order case of one of the four table calls ("project", "cloud", "reproject", "stereo")."""
    import test_gpu_stream_order as S
    rows, cols, b = C.STREAM_ROWS, C.STREAM_COLS, C.STREAM_B
    if which == "project":
        return _ordered_case(which, "project_points_calib 24x40", (rows, cols, b),
                             lambda c: {"pts": c.points, "off": c.offsets}, {"sparse": S.Out((b, rows, cols), f32)},
                             lambda ctx, t, st: _none(ctx.project_points_calib_dev(t["pts"], t["off"], t["calib"], rows, cols, t["sparse"], stream=st)),
                             lambda c, fr: {"sparse": np.stack([fr(f) for f in range(b)])})
    if which == "reproject":
        return _ordered_case(which, "reproject_depth_calib 24x40 -> 20x36", (rows, cols, b),
                             lambda c: {"depth": c.frames}, {"out": S.Out((b, 20, 36), f32)},
                             lambda ctx, t, st: _none(ctx.reproject_depth_calib_dev(t["depth"], 20, 36, t["calib"], t["out"], stream=st)),
                             lambda c, fr: {"out": np.stack([fr(f) for f in range(b)])})
    if which == "stereo":
        return _ordered_case(which, "stereo_refine_calib 24x40", (rows, cols, b),
                             lambda c: {"depth": c.depth, "left": c.left, "right": c.right}, {"out": S.Out((b, rows, cols), f32)},
                             lambda ctx, t, st: _none(ctx.stereo_refine_calib_dev(t["depth"], t["left"], t["right"], t["calib"], t["out"], iterations=4, stream=st)),
                             lambda c, fr: {"out": np.stack([fr(f) for f in range(b)])})

    def cloud_expect(c, fr):
        recs = [fr(f) for f in range(b)]
        pts = np.full((b * rows * cols, 4), S.fill_of(f32), f32)          # rows from offsets[batch] on keep the fill
        allr = np.concatenate(recs)
        pts.view(np.uint32)[:len(allr)] = allr
        return {"points": pts, "offsets": np.concatenate([[0], np.cumsum([len(x) for x in recs])]).astype(np.int32)}

    return _ordered_case(which, "depth_to_cloud_calib 24x40", (rows, cols, b),
                         lambda c: {"depth": c.frames, "bgr": c.bgr},
                         {"points": S.Out((b * rows * cols, 4), f32, per_frame=False), "offsets": S.Out((b + 1,), np.int32, per_frame=False)},
                         lambda ctx, t, st: _none(ctx.depth_to_cloud_calib_dev(t["depth"], t["calib"], t["bgr"], d_points=t["points"], d_offsets=t["offsets"], stream=st)),
                         cloud_expect)


@gpu
@pytest.mark.parametrize("which", ["project", "cloud", "reproject", "stereo"])
def test_table_call_queued_behind_a_delay_reads_its_table_in_stream_order(which):
    """The scheme of test_gpu_stream_order.py (its helpers, imported): the call is queued behind a delay kernel on a stream of its
    own, its inputs -- THE TABLE AMONG THEM -- are copied in on that stream right in front of it and overwritten with decoys right
    behind it, and the marker behind the delay must still be pending when the call returns.  A call that read the table too early or
    too late, or not on its stream, gives the decoy's bits."""
    import test_gpu_stream_order as S
    S.run_ordered(stream_order_case(which))
