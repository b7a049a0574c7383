"""dcmt_joint_bilateral_dev on the device against the two restatements of tests/joint_restatement.py, bit for bit: every listed
shape (tile seams at column 64 / 128 and row 16 / 32 / 64 with holes and valid pixels on both sides), R in {1, 3, 9}, one and three
channels, every flag combination, min_weight 1 and large, the counts; the reach of a lone pixel, one KITTI-sized frame, batches
against each frame alone, frames that must not leak into their neighbours, pointers offset by one element (the guide by one byte)
inside guard bands, tables with entries above 255, the host form with pitched rows, the wrappers' own outputs, the refusals, the call
queued behind other work on a stream and the chain completion -> trust mask -> joint bilateral -> evaluation on one stream.
The tap-major restatement is computed once per case and shared (tests/joint_restatement.py: case); the literal one runs on every pixel
of a small plane and on a few hundred pixels of a large one, the tile seams among them."""
import ctypes

import numpy as np
import pytest

import joint_restatement as J
import support_restatement as S
import test_gpu_stream_order as SO
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

gpu = pytest.mark.gpu
f32, u8, u16, u32 = np.float32, np.uint8, np.uint16, np.uint32
MAX_ROWS, MAX_COLS, MAX_BATCH = 352, 1216, 5
LITERAL_PIXELS = 400
SMALL = [(1, 1), (1, 65), (17, 1), (5, 3)]
LARGE = [(33, 130), (65, 129)]
FLAGS = [(True, False), (False, True), (True, True)]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, MAX_ROWS, MAX_COLS, MAX_BATCH)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()         # (a copy: the shared inputs are read-only)


def host(t):
    return t.cpu().numpy()


def tabdev(tab):
    return api.calib_to_device(np.array(tab))                        # (a copy: the shared records are read-only)


def differ(got, wanted, what):
    assert got.shape == wanted.shape and got.dtype == wanted.dtype, (what, got.shape, got.dtype, wanted.shape, wanted.dtype)
    neq = np.ascontiguousarray(got).view(u32) != np.ascontiguousarray(wanted).view(u32)
    if neq.any():
        first = tuple(np.argwhere(neq)[0])
        raise AssertionError(f"{what}: {int(neq.sum())} elements differ, first at {first}: {got[first]!r} vs {wanted[first]!r}")


def small_plane(rows, cols, seed):
    """A plane of any size: values between 0.5 and 80 m, four pixels in ten holes, and the specials where there is room."""
    g = np.random.Generator(np.random.PCG64(seed))
    z = np.where(g.random((rows, cols)) < 0.4, 0.0, g.uniform(0.5, 80.0, (rows, cols))).astype(f32)
    flat = z.reshape(-1)
    for i, s in enumerate(g.permutation(flat.size)[:flat.size // 3]):
        flat[s] = f32((J.SPECIALS + (0.1, 100.0))[i % 12])
    return z


_want = {}


def want(z, g, tab, **kw):
    """Both restatements of one frame, computed once per input and shared (never modified): (out, filled, left)."""
    key = (z.shape, z.tobytes(), g.tobytes(), tab.tobytes(), tuple(sorted(kw.items())))
    if key not in _want:
        out, filled, left = J.tap_major(z, g, tab, **kw)
        check_literal(z, g, tab, out, (filled, left), **kw)
        out.setflags(write=False)
        _want[key] = (out, filled, left)
    return _want[key]


def check_literal(z, g, tab, out, counts, **kw):
    """The literal restatement against the tap-major one: on every pixel of a small plane, else on LITERAL_PIXELS of them, the ones on
    either side of every tile seam first."""
    rows, cols = z.shape
    if z.size <= LITERAL_PIXELS:
        lit = J.literal(z, g, tab, **kw)
        assert lit[0].tobytes() == out.tobytes() and lit[1:] == counts
        return
    gen = np.random.Generator(np.random.PCG64(z.size))
    seams = [(min(y + dy, rows - 1), min(x + dx, cols - 1)) for y in range(15, rows, 16) for x in range(63, cols, 64) for dy in (0, 1) for dx in (0, 1)]
    rest = [(int(i) // cols, int(i) % cols) for i in gen.permutation(z.size)[:LITERAL_PIXELS - len(seams[:LITERAL_PIXELS // 2])]]
    lit, mask = J.literal(z, g, tab, pixels=seams[:LITERAL_PIXELS // 2] + rest, **kw)
    assert np.array_equal(lit.view(u32)[mask], out.view(u32)[mask])


def run(ctx, zs, gs, tab, what, **kw):
    """The batch through the device call with counts, every frame against the restatements."""
    out, cnt = ctx.joint_bilateral_dev(dev(zs), dev(gs), tabdev(tab), counts=True, **kw)
    out, cnt = host(out), host(cnt)
    assert out.shape == zs.shape and cnt.shape == (len(zs), 2)
    for f in range(len(zs)):
        w = want(zs[f], gs[f], tab, **kw)
        differ(out[f], w[0], f"{what} frame {f}")
        assert tuple(cnt[f]) == w[1:], (what, f, tuple(cnt[f]), w[1:])
    return out, cnt


# ------------------------------------------------------------------------------------------------------------- shapes
@gpu
@pytest.mark.parametrize("rows,cols", SMALL)
def test_small_shapes(ctx, rows, cols):
    z = small_plane(rows, cols, rows * 100 + cols)
    for radius in (1, 3, 9):
        tab = J.as_record(*J.tables(radius, **J.SIGMAS))
        for channels in (1, 3):
            g = J.guide_plane(rows, cols, channels, rows + cols)
            for fill, smooth in FLAGS:
                for mw in (1, 5000):
                    run(ctx, z[None], g[None], tab, f"{rows}x{cols} R {radius} ch {channels} {fill} {smooth} {mw}", radius=radius, fill=fill, smooth=smooth,
                        min_weight=mw)


@gpu
@pytest.mark.parametrize("radius", [1, 3, 9])
@pytest.mark.parametrize("rows,cols", LARGE)
def test_shapes_with_tile_seams(ctx, rows, cols, radius):
    tabd = None
    for channels in (1, 3):
        for fill, smooth in FLAGS:
            for mw in (1, 5000):
                z, g, tab, out, filled, left = J.case(rows, cols, 1, channels, radius, fill, smooth, mw)
                what = f"{rows}x{cols} R {radius} ch {channels} fill {fill} smooth {smooth} min_weight {mw}"
                check_literal(z, g, tab, out, (filled, left), radius=radius, fill=fill, smooth=smooth, min_weight=mw)
                tabd = tabdev(tab) if tabd is None else tabd
                got, cnt = ctx.joint_bilateral_dev(dev(z), dev(g), tabd, counts=True, radius=radius, fill=fill, smooth=smooth, min_weight=mw)
                differ(host(got), out, what)
                assert host(cnt).tolist() == [[filled, left]], what
    ok = J.valid_mask(z)                                              # holes and valid pixels on both sides of every seam
    for yy in range(16, rows, 16):
        assert all((~ok[yy + k]).any() and ok[yy + k].any() for k in (-1, 0))
    for xx in range(64, cols, 64):
        assert all((~ok[:, xx + k]).any() and ok[:, xx + k].any() for k in (-1, 0))


@gpu
def test_the_reach_of_a_lone_pixel_is_exactly_the_disc(ctx):
    z = np.zeros((12, 12), f32)
    z[0, 0] = 42.5
    g = np.random.Generator(np.random.PCG64(1)).integers(0, 256, (12, 12)).astype(u8)
    tab = J.as_record(np.full(128, 255, u16), np.full(768, 255, u16))
    out, cnt = run(ctx, z[None], g[None], tab, "lone pixel", radius=9)
    Y, X = np.mgrid[0:12, 0:12]
    inside = Y * Y + X * X <= 81
    assert ((out[0] == 42.5) == inside).all() and not out[0][~inside].any() and cnt.tolist() == [[int(inside.sum()) - 1, int((~inside).sum())]]
    out, _ = run(ctx, z[None], g[None], J.as_record(*J.tables(9, 100.0, 1000.0)), "lone pixel, tables of R = 9", radius=9)
    assert ((out[0] == 42.5) == inside).all()
    out, _ = run(ctx, z[None], g[None], tab, "lone pixel, R = 3", radius=3)
    assert ((out[0] == 42.5) == (Y * Y + X * X <= 9)).all()


@gpu
def test_one_kitti_frame(ctx):
    rows, cols = 352, 1216
    z, g = J.holed_plane(rows, cols, 3), J.guide_plane(rows, cols, 3, 3)
    tab = J.as_record(*J.tables(6, **J.SIGMAS))
    out, cnt = run(ctx, z[None], g[None], tab, "352x1216", radius=6, smooth=True)
    assert cnt[0, 0] > 50000 and cnt[0].sum() == int((~J.valid_mask(z)).sum())


# ------------------------------------------------------------------------------------------------------------- batches
@gpu
@pytest.mark.parametrize("b", [1, 3, 5])
def test_batches_against_each_frame_alone(ctx, b):
    rows, cols, radius = 33, 130, 3
    for channels, (fill, smooth) in ((1, (True, False)), (3, (True, True))):
        frames = [J.case(rows, cols, 10 + f, channels, radius, fill, smooth, 1) for f in range(b)]
        zs, gs = np.stack([c[0] for c in frames]), np.stack([c[1] for c in frames])
        out, cnt = ctx.joint_bilateral_dev(dev(zs), dev(gs), tabdev(frames[0][2]), counts=True, radius=radius, fill=fill, smooth=smooth)
        for f in range(b):
            differ(host(out)[f], frames[f][3], f"batch {b} frame {f}")
            alone = ctx.joint_bilateral_dev(dev(zs[f]), dev(gs[f]), tabdev(frames[0][2]), radius=radius, fill=fill, smooth=smooth)
            assert host(alone).tobytes() == frames[f][3].tobytes()
        assert host(cnt).tolist() == [[c[4], c[5]] for c in frames]
        assert len({c[3].tobytes() for c in frames}) == b


@gpu
def test_nothing_crosses_a_frame_or_wraps_a_row(ctx):
    """A frame without a valid pixel between two frames that are all valid, at R = 9 with every weight 255: it comes back unchanged,
    left = rows * cols; and a column of valid pixels at the right edge does not reach the left edge of the next row."""
    rows, cols = 20, 70
    holes = np.resize(np.array(J.SPECIALS + (0.0,), f32), (rows, cols)).copy()
    edge = np.zeros((rows, cols), f32)
    edge[:, -1] = 9.0
    zs = np.stack([np.full((rows, cols), 5.0, f32), holes, np.full((rows, cols), 6.0, f32), edge])
    gs = np.zeros((4, rows, cols), u8)
    tab = J.as_record(np.full(128, 255, u16), np.full(768, 255, u16))
    out, cnt = run(ctx, zs, gs, tab, "neighbours", radius=9, smooth=True)
    assert out[1].tobytes() == holes.tobytes() and cnt.tolist()[:3] == [[0, 0], [0, rows * cols], [0, 0]]
    assert out[0].tobytes() == zs[0].tobytes() and out[2].tobytes() == zs[2].tobytes()
    assert (out[3][:, -10:] == 9.0).all() and not out[3][:, :-10].any()


# ------------------------------------------------------------------------------------------------------------- alignment, tables
@gpu
def test_pointers_offset_by_one_element(ctx):
    import torch
    rows, cols, b, radius = 33, 130, 3, 3
    n = b * rows * cols
    for channels in (1, 3):
        frames = [J.case(rows, cols, 20 + f, channels, radius, True, True, 1) for f in range(b)]
        zs, gs, outw = (np.stack([c[k] for c in frames]) for k in (0, 1, 3))
        tabd = tabdev(frames[0][2])
        for oz, og, oo, oc in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1), (3, 2, 1, 3), (0, 3, 2, 1)):
            bz, bo = (torch.full((n + 8,), 37.0, dtype=torch.float32, device="cuda") for _ in range(2))
            bg = torch.full((channels * n + 8,), 0x25, dtype=torch.uint8, device="cuda")
            bc = torch.full((2 * b + 8,), 0x25, dtype=torch.int32, device="cuda")
            vz, vo = bz[oz:oz + n].view(b, rows, cols), bo[oo:oo + n].view(b, rows, cols)
            vg = bg[og:og + channels * n].view(gs.shape)
            vc = bc[oc:oc + 2 * b].view(b, 2)
            vz.copy_(dev(zs)); vg.copy_(dev(gs))
            assert vg.data_ptr() % 4 == (bg.data_ptr() + og) % 4
            ctx.joint_bilateral_dev(vz, vg, tabd, d_out=vo, d_counts=vc, radius=radius, smooth=True)
            differ(host(vo), outw, f"channels {channels} offsets {(oz, og, oo, oc)}")
            assert host(vc).tolist() == [[c[4], c[5]] for c in frames]
            ho, hc = host(bo), host(bc)                               # nothing outside the outputs
            assert (ho[:oo] == 37.0).all() and (ho[oo + n:] == 37.0).all() and (hc[:oc] == 0x25).all() and (hc[oc + 2 * b:] == 0x25).all()


@gpu
def test_a_table_with_entries_above_255(ctx):
    gen = np.random.Generator(np.random.PCG64(5))
    wide = J.as_record(gen.integers(0, 65536, 128).astype(u16), gen.integers(0, 65536, 768).astype(u16))
    clamped = J.as_record(np.minimum(wide["w_space"][0], 255), np.minimum(wide["w_guide"][0], 255))
    z, g = J.holed_plane(33, 130, 2), J.guide_plane(33, 130, 3, 2)
    a, ca = run(ctx, z[None], g[None], wide, "wide entries", radius=3, smooth=True)
    c, cc = run(ctx, z[None], g[None], clamped, "clamped entries", radius=3, smooth=True)
    assert a.tobytes() == c.tobytes() and ca.tolist() == cc.tolist() and ca[0, 0] > 0


# ------------------------------------------------------------------------------------------------------------- host form, wrappers
@gpu
def test_host_entry_point_and_module_level_calls(ctx):
    rows, cols = 33, 130
    for channels in (1, 3):
        z, g, tab, out, filled, left = J.case(rows, cols, 30, channels, 3, True, False, 1)
        got = ctx.joint_bilateral(z, g, tab, radius=3)
        differ(got[0], out, "host form")
        assert got[1:] == (filled, left)
        wide = np.full((rows, 150), 3.0, f32)
        wide[:, :cols] = z
        gwide = np.full((rows, 140) + g.shape[2:], 9, u8)
        gwide[:, :cols] = g
        differ(ctx.joint_bilateral(wide[:, :cols], gwide[:, :cols], tab, radius=3)[0], out, "pitched inputs")
        differ(api.joint_bilateral_fill(z, g, tab, radius=3), out, "joint_bilateral_fill")
    z, g = J.holed_plane(rows, cols, 31), J.guide_plane(rows, cols, 1, 31)
    dflt = J.as_record(*J.tables(**J.SIGMAS))
    differ(api.joint_bilateral_fill(z, g), want(z, g, dflt)[0], "joint_bilateral_fill, every default")
    differ(ctx.joint_bilateral(z, g, radius=9)[0], want(z, g, J.as_record(*J.tables(9, **J.SIGMAS)), radius=9)[0], "the default tables follow the radius")
    # the wrapper's own outputs, a [rows][cols] tensor, a guide with a trailing axis of one
    w = want(z, g, dflt)
    o = ctx.joint_bilateral_dev(dev(z), dev(g), tabdev(dflt))
    assert tuple(o.shape) == (rows, cols)
    differ(host(o), w[0], "allocated output")
    o, n = ctx.joint_bilateral_dev(dev(z[None]), dev(g[None, :, :, None]), tabdev(dflt), counts=True)
    differ(host(o)[0], w[0], "allocated outputs")
    assert host(n).tolist() == [list(w[1:])] and str(n.dtype) == "torch.int32"
    # the C entry point itself: a pitched output, with and without the counts
    p = api.make_joint_params()
    for cnt in ((ctypes.c_uint32 * 2)(77, 77), None):
        pitched = np.full((rows, 200), -3.0, f32)
        st = L.lib().dcmt_joint_bilateral(ctx._h, z.ctypes.data, cols * 4, g.ctypes.data, cols, 1, dflt.ctypes.data, pitched.ctypes.data, 800, rows, cols,
                                          ctypes.byref(p), cnt)
        assert st == L.OK and (cnt is None or tuple(cnt) == w[1:])
        differ(np.ascontiguousarray(pitched[:, :cols]), w[0], "host, pitched output")
        assert (pitched[:, cols:] == -3.0).all()


# ------------------------------------------------------------------------------------------------------------- stream order, the chain
def stream_case(rows=40, cols=133, b=3):
    tab = J.as_record(*J.tables(3, **J.SIGMAS))

    def inputs(which):
        zs = np.stack([J.holed_plane(rows, cols, 700 + 10 * which + f, specials=False) for f in range(b)])       # (no NaN: SO compares values)
        return {"depth": zs, "guide": np.stack([J.guide_plane(rows, cols, 3, 700 + 10 * which + f) for f in range(b)]),
                "tables": tab.view(u8).reshape(1, -1)}

    def call(ctx, t, st):
        ctx.joint_bilateral_dev(t["depth"], t["guide"], t["tables"], d_out=t["out"], d_counts=t["counts"], stream=st, radius=3, smooth=True)

    def wrap(ctx, t, st):
        out, cnt = ctx.joint_bilateral_dev(t["depth"], t["guide"], t["tables"], counts=True, stream=st, radius=3, smooth=True)
        return {"out": out, "counts": cnt}

    def expect(inp):
        w = [want(inp["depth"][f], inp["guide"][f], tab, radius=3, smooth=True) for f in range(b)]
        return {"out": np.stack([x[0] for x in w]), "counts": np.array([x[1:] for x in w], np.int32)}

    outs = {"out": SO.Out((b, rows, cols), f32), "counts": SO.Out((b, 2), np.int32)}
    return SO.Case("joint_bilateral", (rows, cols, b), inputs, outs, call, expect, None, wrap)


@gpu
def test_queued_behind_other_work_on_a_stream():
    """The scheme of tests/test_gpu_stream_order.py: behind a delay on a non-default stream, producer copies, the call and the consumer
    copies with no host synchronisation between them; the clones hold the restatement's bits, so nothing blocked and nothing escaped
    to the null stream."""
    SO.run_ordered(stream_case())


@gpu
def test_wrapper_creates_its_outputs_on_the_stream_it_enqueues_on():
    case = stream_case()
    SO.cases()[case.name] = case                             # that test looks its case up by name
    try:
        SO.test_wrapper_creates_its_output_on_the_stream_it_enqueues_on(case.name)
    finally:
        del SO.cases()[case.name]


@gpu
def test_chain_completion_trust_mask_joint_bilateral_evaluation_on_one_stream():
    """complete_dev -> support_distance_dev (in place, zero beyond R = 3) -> joint_bilateral_dev -> evaluate_dev on one non-default stream
    with no host synchronisation in between, against the numpy composition: the oracle's completion, the support restatement's select,
    the joint restatements; the sums of the evaluation are those of the evaluation made alone on that composed plane."""
    import torch
    rows, cols, b = 48, 64, 3
    sparse = SO.sparse_frames(b, rows, cols, 31, gap=True)
    g = np.random.Generator(np.random.PCG64(33))
    guide = np.stack([J.guide_plane(rows, cols, 1, 40 + f) for f in range(b)])
    gt = np.where(g.random((b, rows, cols)) < 0.3, g.uniform(1.0, 80.0, (b, rows, cols)), 0.0).astype(f32)
    params = api.make_params(spec_fill_iters=SO.SPEC)
    tab = J.as_record(*J.tables(6, 3.0, 40.0))
    s = torch.cuda.Stream()
    with api.Context(0, rows, cols, b) as c:
        d_sparse, d_guide, d_gt, d_tab = dev(sparse), dev(guide), dev(gt), tabdev(tab)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            dense = c.complete_dev(d_sparse, None, params, stream=s.cuda_stream)
            trusted, bey = c.support_distance_dev(d_sparse, dense, d_out=dense, beyond=True, stream=s.cuda_stream, max_radius=3)
            filled, cnt = c.joint_bilateral_dev(trusted, d_guide, d_tab, counts=True, stream=s.cuda_stream)
            sums = c.evaluate_dev(d_gt, filled, stream=s.cuda_stream)
        s.synchronize()
        got = {"filled": host(filled), "counts": host(cnt), "beyond": host(bey), "sums": host(sums)}
        composed = np.empty_like(sparse)
        for f in range(b):
            y, info = SO.O().img_completion(sparse[f], return_info=True)
            assert info["rc"] == 0 and info["fill_iters"] < SO.SPEC
            d2, n = S.edt_dist2(sparse[f], max_radius=3)
            cut = S.select(d2, y)
            w = want(cut, guide[f], tab)
            composed[f] = w[0]
            differ(got["filled"][f], w[0], f"frame {f}: filled")
            assert got["beyond"][f] == n and 0 < n < rows * cols and tuple(got["counts"][f]) == w[1:] and w[1] + w[2] == n and w[1] > 0
            assert got["sums"][f, 0] == int(((gt[f] > 0) & (composed[f] > 0)).sum())
        alone = host(c.evaluate_dev(d_gt, dev(composed)))
    assert got["sums"].tobytes() == alone.tobytes()


# ------------------------------------------------------------------------------------------------------------- refusals
@gpu
def test_refusals(ctx):
    import torch
    lib = L.lib()
    r, c, b = 8, 16, 3
    n = r * c * b
    buf = torch.full((32 * n,), 0x5A, dtype=torch.uint8, device="cuda")
    z = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    gd = torch.full((3 * n,), 9, dtype=torch.uint8, device="cuda")
    out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((2 * b,), 0x25, dtype=torch.int32, device="cuda")
    tab = tabdev(api.make_joint_tables())
    good = api.make_joint_params()
    P = lambda t, off=0: t.data_ptr() + off

    def call(zz=P(z), gg=P(gd), ch=1, tt=P(tab), oo=P(out), nn=P(cnt), rows=r, cols=c, batch=b, h=ctx._h, p=good):
        return lib.dcmt_joint_bilateral_dev(h, zz, gg, ch, tt, oo, rows, cols, batch, None if p is None else ctypes.byref(p), nn, None)

    def params(**kw):
        p = api.make_joint_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    bad = [call(zz=None), call(gg=None), call(tt=None), call(oo=None), call(p=None), call(h=None),
           call(ch=0), call(ch=2), call(ch=4), call(ch=-1),
           call(zz=P(z, 2)), call(oo=P(out, 2)), call(nn=P(cnt, 2)), call(tt=P(buf, 1)),
           call(rows=MAX_ROWS + 1), call(cols=MAX_COLS + 1), call(batch=MAX_BATCH + 1), call(rows=0), call(cols=0), call(batch=0),
           call(oo=P(z)), call(zz=P(buf), oo=P(buf, 4)), call(zz=P(buf), oo=P(buf, 4 * n - 4)), call(zz=P(buf, 64), oo=P(buf)),
           call(gg=P(z)), call(gg=P(out, 4 * n - 1)), call(gg=P(out), ch=3), call(tt=P(z)), call(tt=P(out, 4 * n - 2)), call(tt=P(gd)), call(tt=P(gd, 3 * n - 2), ch=3),
           call(nn=P(z)), call(nn=P(out, 4 * n - 4)), call(nn=P(gd)), call(nn=P(tab, 1788)), call(oo=P(tab)), call(zz=P(tab)),
           call(p=params(radius=0)), call(p=params(radius=-1)), call(p=params(radius=10)), call(p=params(flags=0)), call(p=params(flags=4)), call(p=params(flags=7)),
           call(p=params(min_weight=0)),
           call(p=params(valid_thresh=0.06)), call(p=params(valid_thresh=float("nan"))), call(p=params(valid_thresh=float("inf"))), call(p=params(valid_thresh=-1.0)),
           call(p=params(max_depth=0.05)), call(p=params(max_depth=16385.0)), call(p=params(max_depth=float("inf"))), call(p=params(max_depth=float("nan")))]
    assert bad == [L.E_INVALID] * len(bad), bad
    torch.cuda.synchronize()
    assert (host(out) == -7.0).all() and (host(cnt) == 0x25).all() and (host(buf) == 0x5A).all() and (host(z) == 7.0).all() and (host(gd) == 9).all()   # nothing written
    assert host(tab).tobytes() == api.make_joint_tables().tobytes()
    # what is allowed: without counts, three channels, a guide at an odd byte, touching buffers, the extreme parameters
    assert call() == L.OK and call(nn=None) == L.OK and call(ch=3) == L.OK and call(gg=P(gd, 1)) == L.OK
    assert call(zz=P(buf), gg=P(buf, 4 * n), ch=3, tt=P(buf, 7 * n), oo=P(buf, 12 * n), nn=P(buf, 16 * n)) == L.OK
    assert call(p=params(radius=1, flags=3, min_weight=2 ** 32 - 1, valid_thresh=0.0625, max_depth=16384.0)) == L.OK and call(p=params(radius=9, flags=2)) == L.OK
    torch.cuda.synchronize()
    assert (host(out) == 7.0).all() and not host(cnt).any() and (host(z) == 7.0).all()                 # every pixel valid, a constant plane
    # the host form
    hz, hg, ho = np.full((r, c), 7.0, f32), np.full((r, c), 9, u8), np.full((r, c), -7.0, f32)
    ht = api.make_joint_tables()
    one = lambda *a: lib.dcmt_joint_bilateral(ctx._h, *a)
    gp = ctypes.byref(good)
    Z, G, T, O = hz.ctypes.data, hg.ctypes.data, ht.ctypes.data, ho.ctypes.data
    assert one(Z, c * 4, G, c, 1, T, O, c * 4, r, c, gp, None) == L.OK and (ho == 7.0).all()
    ho[:] = -7.0
    bad = [one(None, c * 4, G, c, 1, T, O, c * 4, r, c, gp, None), one(Z, c * 4, None, c, 1, T, O, c * 4, r, c, gp, None), one(Z, c * 4, G, c, 1, None, O, c * 4, r, c, gp, None),
           one(Z, c * 4, G, c, 1, T, None, c * 4, r, c, gp, None), one(Z, c * 4, G, c, 1, T, O, c * 4, r, c, None, None), one(Z, c * 4, G, c, 2, T, O, c * 4, r, c, gp, None),
           one(Z, c * 4 - 4, G, c, 1, T, O, c * 4, r, c, gp, None), one(Z, c * 4, G, c - 1, 1, T, O, c * 4, r, c, gp, None), one(Z, c * 4, G, 3 * c - 1, 3, T, O, c * 4, r, c, gp, None),
           one(Z, c * 4, G, c, 1, T, O, c * 4 - 4, r, c, gp, None), one(Z, c * 4, G, c, 1, T, O, c * 4, MAX_ROWS + 1, c, gp, None),
           one(Z, c * 4, G, c, 1, T, O, c * 4, r, c, ctypes.byref(params(radius=10)), None), one(Z, c * 4, G, c, 1, T, O, c * 4, r, c, ctypes.byref(params(flags=0)), None)]
    assert bad == [L.E_INVALID] * len(bad) and (ho == -7.0).all(), bad
    d0, g0 = dev(np.zeros((1, r, c), f32)), dev(np.zeros((1, r, c), u8))
    with pytest.raises(ValueError):
        ctx.joint_bilateral_dev(d0, g0, tab, radius=0)
    with pytest.raises(ValueError):
        ctx.joint_bilateral_dev(d0, g0, tab, fill=False)
    with pytest.raises(api.DcmtError) as e:
        ctx.joint_bilateral_dev(d0, g0, tab, d_out=d0)
    assert e.value.status == L.E_INVALID
