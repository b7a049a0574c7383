"""dcmt_depth_normals_dev and its table twin on the device against the two restatements of tests/normals_restatement.py, bit for bit
(records and planes compared as uint32): every listed shape, two shapes with valid pixels and holes on both sides of every seam of
the kernel's strips (64 columns) and bands (8 rows at these sizes; 16 in the batch of full frames, 32 in the largest batch), one
KITTI-sized frame; planes with 40 % holes and the specials, a dense smooth plane, the tie planes; default, zero and large
min_plane_dist; normals only, filter only, both, with and without counts; in place against out of place, batches against each frame
alone, frames that must not leak into their neighbours, pointers offset by one element inside guard bands; the table twin and its bad
records; the host form with pitched rows, the wrappers' own outputs, the refusals; the call queued behind other work on a stream; the
chain completion -> normals and filter in place -> cloud on one stream; and a batch whose records pass 2^32 bytes.
The vectorised restatement is computed once per input and shared; the literal one runs on every pixel of the planes up to
LITERAL_PIXELS (tests/test_normals.py compares the two on the rest)."""
import ctypes

import numpy as np
import pytest

import normals_restatement as N
import test_gpu_stream_order as SO
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api
from test_cloud import want_cloud, words

gpu = pytest.mark.gpu
f32, f64, u32 = np.float32, np.float64, np.uint32
MAX_ROWS, MAX_COLS, MAX_BATCH = 352, 1216, 5
LITERAL_PIXELS = 12000
SMALL = [(1, 1), (1, 2), (2, 1), (1, 65), (17, 1), (5, 3)]
SEAMS = [(70, 131), (33, 257)]
DMINS = (0.4, 0.0, 30.0)


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


def differ(got, wanted, what):
    assert got.shape == wanted.shape and got.dtype == wanted.dtype, (what, got.shape, got.dtype, wanted.shape, wanted.dtype)
    neq = np.ascontiguousarray(got).view(u32) != np.ascontiguousarray(wanted).view(u32)
    if neq.any():
        first = tuple(np.argwhere(neq)[0])
        raise AssertionError(f"{what}: {int(neq.sum())} elements differ, first at {first}: {got[first]!r} vs {wanted[first]!r}")


_want = {}


def want(z, **kw):
    """The restatements of one frame, computed once per input and shared (never modified): (normals, out, removed, none)."""
    key = (z.shape, z.tobytes(), tuple(sorted(kw.items())))
    if key not in _want:
        res = N.vectorised(z, **kw)
        if z.size <= LITERAL_PIXELS:
            lit = N.literal(z, **kw)
            assert lit[0].tobytes() == res[0].tobytes() and lit[1].tobytes() == res[1].tobytes() and lit[2:] == res[2:]
        for a in res[:2]:
            a.setflags(write=False)
        _want[key] = res
    return _want[key]


def cloud_of(kw):
    """(the dcmt_cloud_params of a call, the restatement's keywords) from one dict of intrinsics and parameters."""
    return api.make_cloud_params(**{k: kw[k] for k in ("fx", "fy", "cx", "cy") if k in kw}), {k: v for k, v in kw.items() if k not in ("fx", "fy", "cx", "cy")}


def run_all(ctx, zs, what, **kw):
    """The batch through every combination of outputs and both routes, every frame against the restatements."""
    import torch
    zs = np.ascontiguousarray(zs, f32)
    b = len(zs)
    w = [want(z, **kw) for z in zs]
    wn, wo = np.stack([x[0] for x in w]), np.stack([x[1] for x in w])
    wc = np.array([x[2:] for x in w], np.int32)
    cp, pk = cloud_of(kw)
    d = dev(zs)
    n, o, c = ctx.depth_normals_dev(d, cp, d_out=torch.full_like(d, -3.0), counts=True, **pk)                 # both, counts
    differ(host(n), wn, f"{what}: records"); differ(host(o), wo, f"{what}: plane")
    assert host(c).tolist() == wc.tolist(), (what, host(c).tolist(), wc.tolist())
    differ(host(ctx.depth_normals_dev(d, cp, **pk)), wn, f"{what}: records only")                              # normals only, no counts
    o, c = ctx.depth_normals_dev(d, cp, normals=False, counts=True, **pk)                                      # filter only, counts
    differ(host(o), wo, f"{what}: plane only"); assert host(c).tolist() == wc.tolist(), what
    differ(host(ctx.depth_normals_dev(d, cp, normals=False, **pk)), wo, f"{what}: plane only, no counts")
    d1 = d.clone()                                                                                             # in place, filter only
    o, c = ctx.depth_normals_dev(d1, cp, normals=False, d_out=d1, counts=True, **pk)
    assert o.data_ptr() == d1.data_ptr()
    differ(host(d1), wo, f"{what}: in place"); assert host(c).tolist() == wc.tolist(), what
    d2 = d.clone()                                                                                             # in place with the records
    n, o = ctx.depth_normals_dev(d2, cp, d_out=d2, **pk)
    differ(host(n), wn, f"{what}: records beside an in-place filter"); differ(host(d2), wo, f"{what}: in place beside records")
    differ(host(d), zs, f"{what}: the input")
    return wn, wo, wc


def planes_of(rows, cols, seed):
    lin, peak = N.tie_planes(rows, cols)
    return [("holes", N.holey_plane(rows, cols, seed)), ("smooth", N.smooth_plane(rows, cols, seed + 1)), ("lin", lin), ("peak", peak)]


# ------------------------------------------------------------------------------------------------------------- shapes
@gpu
@pytest.mark.parametrize("rows,cols", SMALL)
def test_small_shapes(ctx, rows, cols):
    for name, z in planes_of(rows, cols, rows * 100 + cols):
        for dmin in DMINS:
            run_all(ctx, z[None], f"{name} {rows}x{cols} {dmin}", min_plane_dist=dmin, **N.KITTI)
    run_all(ctx, N.smooth_plane(rows, cols, 2)[None], f"{rows}x{cols}, the library's intrinsics")


@gpu
@pytest.mark.parametrize("rows,cols", SEAMS)
def test_shapes_with_strip_and_band_seams(ctx, rows, cols):
    removed = 0
    for name, z in planes_of(rows, cols, rows + cols):
        for dmin in DMINS:
            removed += int(run_all(ctx, z[None], f"{name} {rows}x{cols} {dmin}", min_plane_dist=dmin, **N.KITTI)[2][0, 0])
    assert removed > 0
    z = N.holey_plane(rows, cols, rows + cols)
    ok = (z >= f32(0.1)) & (z <= f32(100.0))                            # holes and valid pixels on both sides of every seam
    for yy in range(8, rows, 8):
        assert all((~ok[yy + k]).any() and ok[yy + k].any() for k in (-1, 0))
    for xx in range(64, cols, 64):
        assert all((~ok[:, xx + k]).any() and ok[:, xx + k].any() for k in (-1, 0))
    assert np.isnan(z).any() and np.isinf(z).any() and (z.view(u32) == 0x80000000).any()


@gpu
def test_one_kitti_frame(ctx):
    z = N.holey_plane(352, 1216, 3)
    wn, wo, wc = run_all(ctx, z[None], "352x1216", min_plane_dist=2.0, **N.KITTI)
    assert wc[0, 0] > 1000 and wc[0, 1] > 1000
    run_all(ctx, N.smooth_plane(352, 1216, 4)[None], "352x1216 smooth", **N.KITTI)


# ------------------------------------------------------------------------------------------------------------- batches
@gpu
def test_a_batch_of_five_against_each_frame_alone(ctx):
    rows, cols = 33, 130
    zs = np.stack([N.holey_plane(rows, cols, 10 + f) for f in range(5)])
    wn, wo, wc = run_all(ctx, zs, "batch 5", min_plane_dist=3.0, **N.KITTI)
    cp = api.make_cloud_params(**N.KITTI)
    for f in range(5):
        n, o, c = ctx.depth_normals_dev(dev(zs[f]), cp, normals=True, d_out=dev(np.zeros((rows, cols), f32)), counts=True, min_plane_dist=3.0)
        differ(host(n), wn[f], f"frame {f} alone: records"); differ(host(o), wo[f], f"frame {f} alone: plane")
        assert host(c).tolist() == [wc[f].tolist()]
    assert len({wo[f].tobytes() for f in range(5)}) == 5 and (wc[:, 0] > 0).all()


@gpu
def test_five_full_frames(ctx):
    """At this size the plan takes bands of 16 rows."""
    zs = np.stack([N.holey_plane(352, 1216, 40 + f) if f % 2 else N.smooth_plane(352, 1216, 40 + f) for f in range(5)])
    run_all(ctx, zs, "5 x 352x1216", min_plane_dist=1.0, **N.KITTI)


@gpu
def test_nothing_crosses_a_frame_or_wraps_a_row(ctx):
    """A frame between two very different neighbours does not change; a frame of holes between two dense ones stays untouched; and a
    bright last column does not reach the first column of the next row."""
    rows, cols = 20, 70
    mid = N.holey_plane(rows, cols, 5)
    holes = np.resize(np.array(N.SPECIALS + (0.0,), f32), (rows, cols)).copy()
    edge = np.full((rows, cols), 30.0, f32)
    edge[:, -1] = 2.0
    a = np.stack([np.full((rows, cols), 1.0, f32), mid, np.full((rows, cols), 90.0, f32), holes, edge])
    b = np.stack([N.smooth_plane(rows, cols, 9), mid, N.holey_plane(rows, cols, 6), holes, edge])
    ra, rb = run_all(ctx, a, "neighbours a", min_plane_dist=3.0, **N.KITTI), run_all(ctx, b, "neighbours b", min_plane_dist=3.0, **N.KITTI)
    assert ra[0][1].tobytes() == rb[0][1].tobytes() and ra[1][1].tobytes() == rb[1][1].tobytes() and ra[2][1].tolist() == rb[2][1].tolist()
    assert ra[1][3].tobytes() == holes.tobytes() and not ra[0][3].any() and ra[2][3].tolist() == [0, 0]
    assert ra[2][0].tolist() == [rows * cols, 0] and ra[2][2].tolist() == [0, 0]           # a frontal wall at 1 m goes whole at 3 m, at 90 m it stays
    assert (ra[0][4][:, 0, :2] == 0).all() and (ra[0][4][:, 0, 2] == -1).all()            # column 0 sees a frontal wall


# ------------------------------------------------------------------------------------------------------------- alignment
@gpu
def test_pointers_offset_by_one_element(ctx):
    import torch
    rows, cols, b = 33, 130, 3
    n = b * rows * cols
    zs = np.stack([N.holey_plane(rows, cols, 20 + f) for f in range(b)])
    w = [want(z, min_plane_dist=3.0, **N.KITTI) for z in zs]
    wn, wo, wc = np.stack([x[0] for x in w]), np.stack([x[1] for x in w]), [list(x[2:]) for x in w]
    cp = api.make_cloud_params(**N.KITTI)
    for oz, oo, on, oc in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 4, 0), (0, 0, 0, 1), (1, 1, 4, 1), (3, 2, 8, 3), (2, 3, 0, 1)):
        bz, bo = (torch.full((n + 8,), 37.0, dtype=torch.float32, device="cuda") for _ in range(2))
        bn = torch.full((4 * n + 16,), 37.0, dtype=torch.float32, device="cuda")
        bc = torch.full((2 * b + 8,), 0x25, dtype=torch.int32, device="cuda")
        vz, vo = bz[oz:oz + n].view(b, rows, cols), bo[oo:oo + n].view(b, rows, cols)
        vn, vc = bn[on:on + 4 * n].view(b, rows, cols, 4), bc[oc:oc + 2 * b].view(b, 2)
        vz.copy_(dev(zs))
        ctx.depth_normals_dev(vz, cp, d_normals=vn, d_out=vo, d_counts=vc, min_plane_dist=3.0)
        what = f"offsets {(oz, oo, on, oc)}"
        differ(host(vn), wn, what + ": records"); differ(host(vo), wo, what + ": plane")
        assert host(vc).tolist() == wc, what
        ho, hn, hc = host(bo), host(bn), host(bc)                      # nothing outside the outputs
        assert (ho[:oo] == 37.0).all() and (ho[oo + n:] == 37.0).all() and (hn[:on] == 37.0).all() and (hn[on + 4 * n:] == 37.0).all()
        assert (hc[:oc] == 0x25).all() and (hc[oc + 2 * b:] == 0x25).all()
        ctx.depth_normals_dev(vz, cp, normals=False, d_out=vz, d_counts=vc)           # in place inside its guard bands (the default removes less)
        hz = host(bz)
        differ(hz[oz:oz + n].reshape(b, rows, cols), np.stack([want(z, **N.KITTI)[1] for z in zs]), what + ": in place")
        assert (hz[:oz] == 37.0).all() and (hz[oz + n:] == 37.0).all()


# ------------------------------------------------------------------------------------------------------------- the table twin
def table(records):
    t = np.zeros(len(records), api.CLOUD_CALIB_DTYPE)
    for i, r in enumerate(records):
        t[i] = r
    return t


@gpu
def test_table_twin_equals_the_uniform_call_per_record(ctx):
    rows, cols, b = 33, 130, 5
    zs = np.stack([N.holey_plane(rows, cols, 60 + f) for f in range(b)])
    recs = [(721.5, 721.5, 608.0, 176.0), (959.791, 956.9251, 696.0217, 224.1806), (-500.0, 300.0, -20.5, 1000.25), (2.0 ** -10, 2.0 ** 20, 2.0 ** 20, -2.0 ** 20),
            (1234.5, 0.75, 0.0, 1e-300)]
    t = api.make_normals_calib(*(np.array([r[k] for r in recs]) for k in range(4)))
    assert t.tobytes() == table(recs).tobytes()
    d, dt = dev(zs), api.calib_to_device(t)
    n, o, c = ctx.depth_normals_calib_dev(d, dt, d_out=dev(np.zeros_like(zs)), counts=True, min_plane_dist=3.0)
    n, o, c = host(n), host(o), host(c)
    for f, r in enumerate(recs):
        kw = dict(zip(("fx", "fy", "cx", "cy"), r), min_plane_dist=3.0)
        w = want(zs[f], **kw)
        differ(n[f], w[0], f"table, frame {f}: records"); differ(o[f], w[1], f"table, frame {f}: plane")
        assert tuple(c[f]) == w[2:], (f, tuple(c[f]), w[2:])
        un, uo, uc = ctx.depth_normals_dev(dev(zs[f]), cloud_of(kw)[0], d_out=dev(np.zeros_like(zs[f])), counts=True, min_plane_dist=3.0)
        assert host(un).tobytes() == n[f].tobytes() and host(uo).tobytes() == o[f].tobytes() and host(uc).tolist() == [c[f].tolist()]
    assert len({n[f].tobytes() for f in range(b)}) == b
    d1 = d.clone()                                                      # the twin in place, filter only and with the records
    ctx.depth_normals_calib_dev(d1, dt, normals=False, d_out=d1, min_plane_dist=3.0)
    differ(host(d1), o, "table, in place")
    d2 = d.clone()
    n2, _ = ctx.depth_normals_calib_dev(d2, dt, d_out=d2, min_plane_dist=3.0)
    differ(host(n2), n, "table, records beside an in-place filter"); differ(host(d2), o, "table, in place beside records")
    differ(host(ctx.depth_normals_calib_dev(d, dt, min_plane_dist=3.0)), n, "table, records only")


@gpu
@pytest.mark.parametrize("bad", [(np.nan, 721.5, 608.0, 176.0), (0.0, 721.5, 608.0, 176.0), (721.5, -0.0, 608.0, 176.0), (721.5, 2.0 ** 21, 608.0, 176.0),
                                 (2.0 ** -11, 721.5, 608.0, 176.0), (721.5, 721.5, 2.0 ** 20 + 1, 176.0), (721.5, 721.5, 608.0, -np.inf),
                                 (721.5, 721.5, 608.0, np.nan)])
def test_a_bad_record_empties_its_frame_only(ctx, bad):
    rows, cols, b = 33, 130, 3
    zs = np.stack([N.holey_plane(rows, cols, 70 + f) for f in range(b)])
    good = (721.5, 721.5, 608.0, 176.0)
    valid = int(((zs[1].view(u32) >= f32(0.1).view(u32)) & (zs[1].view(u32) <= f32(100.0).view(u32))).sum())
    dt = api.calib_to_device(table([good, bad, good]))
    for in_place in (False, True):
        d = dev(zs)
        n, o, c = ctx.depth_normals_calib_dev(d, dt, d_out=d if in_place else dev(np.full_like(zs, -3.0)), counts=True, min_plane_dist=3.0)
        n, o, c = host(n), host(o), host(c)
        for f in (0, 2):
            w = want(zs[f], min_plane_dist=3.0, **N.KITTI)
            differ(n[f], w[0], f"frame {f}: records"); differ(o[f], w[1], f"frame {f}: plane")
            assert tuple(c[f]) == w[2:] and w[2] > 0
        assert not n[1].view(u32).any() and o[1].tobytes() == zs[1].tobytes() and c[1].tolist() == [0, valid]


# ------------------------------------------------------------------------------------------------------------- host form, wrappers
@gpu
def test_host_entry_point_and_module_level_calls(ctx):
    rows, cols = 33, 130
    z = N.holey_plane(rows, cols, 30)
    cp = api.make_cloud_params(**N.KITTI)
    w = want(z, min_plane_dist=3.0, **N.KITTI)
    n, o, removed, none = ctx.depth_normals(z, cp, min_plane_dist=3.0)
    differ(n, w[0], "host form: records"); differ(o, w[1], "host form: plane")
    assert (removed, none) == w[2:] and removed > 0
    wide = np.full((rows, 150), 3.0, f32)
    wide[:, :cols] = z
    n, o, _, _ = ctx.depth_normals(wide[:, :cols], cp, min_plane_dist=3.0)
    differ(n, w[0], "pitched input: records"); differ(o, w[1], "pitched input: plane")
    assert ctx.depth_normals(z, cp, normals=False, min_plane_dist=3.0)[0] is None and ctx.depth_normals(z, cp, filtered=False)[1] is None
    dflt = want(z)
    differ(api.depth_normals(z), dflt[0], "depth_normals, every default")
    differ(api.filter_flying_pixels(z), dflt[1], "filter_flying_pixels, every default")
    differ(api.filter_flying_pixels(z, cp, min_plane_dist=3.0), w[1], "filter_flying_pixels")
    dense = np.where(np.isfinite(z) & (z > 0), z, f32(7.0)).astype(f32)
    cloud, nrm = api.reproject_pc_normals(dense)
    assert len(cloud) == rows * cols and nrm.shape == (rows * cols, 4)
    differ(nrm, want(dense)[0].reshape(-1, 4), "reproject_pc_normals")
    cloud, nrm = api.reproject_pc_normals(z)
    with np.errstate(invalid="ignore"):
        sel = z > 0
    assert len(cloud) == int(sel.sum()) and nrm.tobytes() == dflt[0][sel].tobytes()
    # the wrapper's own outputs, a [rows][cols] tensor
    o = ctx.depth_normals_dev(dev(z), normals=False)
    assert tuple(o.shape) == (rows, cols)
    differ(host(o), dflt[1], "allocated plane")
    n, c = ctx.depth_normals_dev(dev(z), counts=True)
    assert tuple(n.shape) == (rows, cols, 4) and tuple(c.shape) == (1, 2) and str(c.dtype) == "torch.int32"
    differ(host(n), dflt[0], "allocated records"); assert host(c).tolist() == [list(dflt[2:])]
    # the C entry point itself: pitched outputs, with and without the counts and either output
    p = api.make_normals_params(min_plane_dist=3.0)
    for cnt in ((ctypes.c_uint32 * 2)(77, 77), None):
        po, pn = np.full((rows, 200), -3.0, f32), np.full((rows, 4 * cols + 12), -3.0, f32)
        st = L.lib().dcmt_depth_normals(ctx._h, z.ctypes.data, cols * 4, rows, cols, ctypes.byref(cp), ctypes.byref(p), pn.ctypes.data, pn.strides[0],
                                        po.ctypes.data, 800, cnt)
        assert st == L.OK and (cnt is None or tuple(cnt) == w[2:])
        differ(np.ascontiguousarray(po[:, :cols]), w[1], "host, pitched plane")
        differ(np.ascontiguousarray(pn[:, :4 * cols]).reshape(rows, cols, 4), w[0], "host, pitched records")
        assert (po[:, cols:] == -3.0).all() and (pn[:, 4 * cols:] == -3.0).all()


# ------------------------------------------------------------------------------------------------------------- stream order, the chain
def stream_case(in_place, rows=40, cols=133, b=3):
    kw = dict(min_plane_dist=3.0)

    def inputs(which):
        return {"depth": np.stack([N.holey_plane(rows, cols, 700 + 10 * which + f, specials=False) for f in range(b)])}     # (no NaN: SO compares values)

    def call(ctx, t, st):
        ctx.depth_normals_dev(t["depth"], d_normals=t["normals"], d_out=t["depth" if in_place else "out"], d_counts=t["counts"], stream=st, **kw)

    def wrap(ctx, t, st):
        n, o, c = ctx.depth_normals_dev(t["depth"], counts=True, filtered=True, stream=st, **kw)
        return {"normals": n, "out": o, "counts": c}

    def expect(inp):
        w = [want(inp["depth"][f], **kw) for f in range(b)]
        return {"normals": np.stack([x[0] for x in w]), ("depth" if in_place else "out"): np.stack([x[1] for x in w]),
                "counts": np.array([x[2:] for x in w], np.int32)}

    outs = {"normals": SO.Out((b, rows, cols, 4), f32), ("depth" if in_place else "out"): SO.Out((b, rows, cols), f32), "counts": SO.Out((b, 2), np.int32)}
    return SO.Case(f"depth_normals {'in place' if in_place else 'out of place'}", (rows, cols, b), inputs, outs, call, expect, None, None if in_place else wrap)


@gpu
@pytest.mark.parametrize("in_place", [False, True])
def test_queued_behind_other_work_on_a_stream(in_place):
    """The scheme of tests/test_gpu_stream_order.py: behind a delay on a non-default stream, producer copies, the call and the consumer
    copies with no host synchronisation between them; the clones hold the restatement's bits, so nothing blocked and nothing escaped
    to the null stream."""
    SO.run_ordered(stream_case(in_place))


@gpu
def test_wrapper_creates_its_outputs_on_the_stream_it_enqueues_on():
    case = stream_case(False)
    SO.cases()[case.name] = case                             # that test looks its case up by name
    try:
        SO.test_wrapper_creates_its_output_on_the_stream_it_enqueues_on(case.name)
    finally:
        del SO.cases()[case.name]


@gpu
def test_chain_completion_normals_cloud_on_one_stream():
    """complete_dev -> depth_normals_dev (the filter in place, the records out) -> depth_to_cloud_dev on one non-default stream with no
    host synchronisation in between, against the numpy composition: the oracle's completion, the restatement, test_cloud.py's cloud;
    the records of the pixels that stay are the normals of the cloud's points, in its order."""
    import torch
    rows, cols, b = 48, 64, 3
    sparse = SO.sparse_frames(b, rows, cols, 31, gap=True)
    params = api.make_params(spec_fill_iters=SO.SPEC)
    kw = dict(min_plane_dist=1.0)
    s = torch.cuda.Stream()
    with api.Context(0, rows, cols, b) as c:
        d_sparse = dev(sparse)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            dense = c.complete_dev(d_sparse, None, params, stream=s.cuda_stream)
            nrm, kept, cnt = c.depth_normals_dev(dense, d_out=dense, counts=True, stream=s.cuda_stream, **kw)
            pts, off = c.depth_to_cloud_dev(kept, stream=s.cuda_stream)
        s.synchronize()
        nrm, kept, cnt, pts, off = host(nrm), host(kept), host(cnt), host(pts), host(off)
    composed = np.empty_like(sparse)
    for f in range(b):
        y, info = SO.O().img_completion(sparse[f], return_info=True)
        assert info["rc"] == 0 and info["fill_iters"] < SO.SPEC
        w = want(np.ascontiguousarray(y, f32), **kw)
        composed[f] = w[1]
        differ(nrm[f], w[0], f"frame {f}: records"); differ(kept[f], w[1], f"frame {f}: plane")
        assert tuple(cnt[f]) == w[2:]
    assert cnt[:, 0].sum() > 0
    wp, wo = want_cloud(composed)
    assert off.tolist() == wo.tolist() and np.array_equal(words(pts[:wo[-1]]), words(wp))
    assert len(nrm[composed > 0]) == wo[-1]


# ------------------------------------------------------------------------------------------------------------- past 2^32 bytes
@gpu
def test_records_past_2_to_the_32_bytes():
    """Frame offsets are 64-bit: 640 frames of 352 x 1216, 6.9 GB of records over 1.1 GB of depth, compared on the first frame, the last
    and the two frames whose records straddle byte 2^32 of d_normals; the counts of every frame against the plane on the device.  At
    this size the plan takes bands of 32 rows."""
    import torch
    rows, cols, b = 352, 1216, 640
    assert 16 * b * rows * cols > 2 ** 32
    g = torch.Generator(device="cuda").manual_seed(5)
    d = 1.0 / (torch.rand((b, rows, cols), device="cuda", generator=g) * 0.004 + 0.02 + torch.arange(rows, device="cuda")[None, :, None] * 0.0004)
    d[torch.rand((b, rows, cols), device="cuda", generator=g) < 0.3] = 0
    straddle = 2 ** 32 // (rows * cols * 16)
    assert straddle * rows * cols * 16 < 2 ** 32 < (straddle + 1) * rows * cols * 16
    picked = [0, straddle, straddle + 1, b - 1]
    cp = api.make_cloud_params(**N.KITTI)
    with api.Context(0, rows, cols, b) as ctx:
        n, o, c = ctx.depth_normals_dev(d, cp, d_out=torch.empty_like(d), counts=True, min_plane_dist=1.0)
        c = host(c)
        for f in picked:
            w = N.vectorised(host(d[f]), min_plane_dist=1.0, **N.KITTI)
            differ(host(n[f]), w[0], f"640 frames: frame {f}, records"); differ(host(o[f]), w[1], f"640 frames: frame {f}, plane")
            assert tuple(c[f]) == w[2:] and w[2] > 0
        assert np.array_equal(host(((o == 0) & (d != 0)).flatten(1).sum(1)), c[:, 0])
        d1 = d.clone()
        ctx.depth_normals_dev(d1, cp, normals=False, d_out=d1, min_plane_dist=1.0)
        assert torch.equal(d1.view(torch.int32), o.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------- refusals
@gpu
def test_refusals(ctx):
    import torch
    lib = L.lib()
    r, c, b = 8, 16, 3
    n = r * c * b
    buf = torch.full((64 * n,), 0x5A, dtype=torch.uint8, device="cuda")
    z = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    nr = torch.full((4 * n,), -7.0, dtype=torch.float32, device="cuda")
    out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((2 * b,), 0x25, dtype=torch.int32, device="cuda")
    tab = api.calib_to_device(api.make_normals_calib([721.5] * b, 721.5, 608.0, 176.0))
    good, cloud = api.make_normals_params(), api.make_cloud_params(**N.KITTI)
    P = lambda t, off=0: t.data_ptr() + off

    def call(zz=P(z), kk=cloud, qq=P(nr), oo=P(out), nn=P(cnt), rows=r, cols=c, batch=b, h=ctx._h, p=good, twin=False):
        fn = lib.dcmt_depth_normals_calib_dev if twin else lib.dcmt_depth_normals_dev
        geo = kk if twin or kk is None else ctypes.byref(kk)
        return fn(h, zz, rows, cols, batch, geo, None if p is None else ctypes.byref(p), qq, oo, nn, None)

    def params(**kw):
        p = api.make_normals_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def intr(**kw):
        k = api.make_cloud_params(**N.KITTI)
        for name, v in kw.items():
            setattr(k, name, v)
        return k

    nan, inf = float("nan"), float("inf")
    bad = [call(zz=None), call(kk=None), call(qq=None, oo=None), call(p=None), call(h=None), call(kk=None, twin=True),
           call(zz=P(z, 2)), call(oo=P(out, 2)), call(nn=P(cnt, 2)), call(qq=P(nr, 4)), call(qq=P(nr, 8)), call(kk=P(tab, 4), twin=True),
           call(rows=MAX_ROWS + 1), call(cols=MAX_COLS + 1), call(batch=MAX_BATCH + 1), call(rows=0), call(cols=0), call(batch=0),
           call(zz=P(buf), oo=P(buf, 4)), call(zz=P(buf), oo=P(buf, 4 * n - 4)), call(zz=P(buf, 64), oo=P(buf)),
           call(qq=P(z)), call(zz=P(buf, 16 * n - 16), qq=P(buf)), call(oo=P(buf, 16 * n - 16), qq=P(buf)), call(qq=P(buf, 16), oo=P(buf)),
           call(nn=P(z)), call(nn=P(out, 4 * n - 4)), call(nn=P(nr, 16 * n - 4)),
           call(kk=P(buf), qq=P(buf, 32 * b - 16), twin=True), call(kk=P(buf, 8), oo=P(buf), twin=True), call(kk=P(cnt), twin=True),
           call(p=params(min_plane_dist=-0.5)), call(p=params(min_plane_dist=1024.5)), call(p=params(min_plane_dist=nan)), call(p=params(min_plane_dist=inf)),
           call(p=params(valid_thresh=0.06)), call(p=params(valid_thresh=nan)), call(p=params(valid_thresh=inf)), call(p=params(valid_thresh=-1.0)),
           call(p=params(max_depth=0.05)), call(p=params(max_depth=16385.0)), call(p=params(max_depth=inf)), call(p=params(max_depth=nan)),
           call(kk=intr(fx=0.0)), call(kk=intr(fy=-0.0)), call(kk=intr(fx=nan)), call(kk=intr(fy=inf)), call(kk=intr(fx=2.0 ** -11)), call(kk=intr(fy=-2.0 ** 21)),
           call(kk=intr(cx=nan)), call(kk=intr(cy=-inf)), call(kk=intr(cx=2.0 ** 20 + 1)), call(kk=intr(cy=-2.0 ** 20 - 1))]
    assert bad == [L.E_INVALID] * len(bad), bad
    torch.cuda.synchronize()
    assert (host(out) == -7.0).all() and (host(nr) == -7.0).all() and (host(cnt) == 0x25).all() and (host(buf) == 0x5A).all() and (host(z) == 7.0).all()
    # what is allowed: either output alone, no counts, in place, touching buffers, the extreme parameters and intrinsics, the twin
    assert call() == L.OK and call(nn=None) == L.OK and call(qq=None) == L.OK and call(oo=None) == L.OK and call(kk=P(tab), twin=True) == L.OK
    assert call(zz=P(buf), qq=P(buf, 4 * n), oo=P(buf, 20 * n), nn=P(buf, 24 * n)) == L.OK
    assert call(p=params(min_plane_dist=0.0, valid_thresh=0.0625, max_depth=16384.0)) == L.OK and call(p=params(min_plane_dist=1024.0)) == L.OK
    assert call(kk=intr(fx=2.0 ** -10, fy=-2.0 ** 20, cx=2.0 ** 20, cy=-2.0 ** 20)) == L.OK and call(kk=intr(cx=0.0, cy=-0.0)) == L.OK
    z2 = z.clone()
    assert call(zz=P(z2), oo=P(z2)) == L.OK
    torch.cuda.synchronize()
    hn = host(nr).reshape(-1, 4)
    assert (host(out) == 7.0).all() and (host(z2) == 7.0).all() and host(cnt).tolist() == [0, 0] * b          # a frontal wall at 7 m: 2^20 * 0 = 0
    assert (hn[:, 2] == -1).all() and not hn[:, :2].any() and np.allclose(hn[:, 3], 7.0, rtol=4e-7)
    # the host form
    hz, ho, hq = np.full((r, c), 7.0, f32), np.full((r, c), -7.0, f32), np.full((r, c, 4), -7.0, f32)
    one = lambda *a: lib.dcmt_depth_normals(ctx._h, *a)
    gp, kp = ctypes.byref(good), ctypes.byref(cloud)
    Z, O, Q = hz.ctypes.data, ho.ctypes.data, hq.ctypes.data
    assert one(Z, c * 4, r, c, kp, gp, Q, c * 16, O, c * 4, None) == L.OK and (ho == 7.0).all() and (hq[..., 2] == -1).all()
    ho[:], hq[:] = -7.0, -7.0
    bad = [one(None, c * 4, r, c, kp, gp, Q, c * 16, O, c * 4, None), one(Z, c * 4, r, c, None, gp, Q, c * 16, O, c * 4, None), one(Z, c * 4, r, c, kp, None, Q, c * 16, O, c * 4, None),
           one(Z, c * 4, r, c, kp, gp, None, 0, None, 0, None), one(Z, c * 4 - 4, r, c, kp, gp, Q, c * 16, O, c * 4, None), one(Z, c * 4, r, c, kp, gp, Q, c * 16 - 4, O, c * 4, None),
           one(Z, c * 4, r, c, kp, gp, Q, c * 16, O, c * 4 - 4, None), one(Z, c * 4, MAX_ROWS + 1, c, kp, gp, Q, c * 16, O, c * 4, None),
           one(Z, c * 4, r, c, kp, ctypes.byref(params(min_plane_dist=-1.0)), Q, c * 16, O, c * 4, None), one(Z, c * 4, r, c, ctypes.byref(intr(fx=0.0)), gp, Q, c * 16, O, c * 4, None)]
    assert bad == [L.E_INVALID] * len(bad) and (ho == -7.0).all() and (hq == -7.0).all(), bad
    d0 = dev(np.zeros((1, r, c), f32))
    with pytest.raises(ValueError):
        ctx.depth_normals_dev(d0, min_plane_dist=-1.0)
    with pytest.raises(ValueError):
        ctx.depth_normals_dev(d0, intr(fx=0.0))
    with pytest.raises(ValueError):
        ctx.depth_normals(np.zeros((r, c), f32), intr(cy=3e6))
    with pytest.raises(api.DcmtError) as e:
        ctx.depth_normals_dev(d0, d_counts=d0.view(torch.int32).view(-1)[:2].view(1, 2))                   # the counts inside the depth plane
    assert e.value.status == L.E_INVALID
