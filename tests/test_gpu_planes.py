"""The per-superpixel plane fit on the device: dcmt_superpixel_planes_dev, its host form and fit_superpixel_planes, bit for bit against
the restatements of tests/planes_restatement.py, for the output plane and for d_fits (test_planes.py holds the two restatements
against each other).  The literal restatement is the reference wherever a frame has at most 10000 pixels; above that (one frame of
352 x 1216, the dense one-label frame) it is the vectorised one, which test_planes.py shows to be the same bits.

Shapes.  k_planes_sum takes tiles of 64 x 64 pixels, a wave 64 columns, k_planes_paint four pixels a lane: 1 x 1, 1 x 70 and 3 x 33
(the scalar paint), 17 x 65 (one column past a wave), 40 x 130 with blocks of 8 (three tiles, labels that straddle them), 33 x 257
with one label over the whole frame (five tiles into one record), 24 x 96 with every pixel its own label (n_labels = 2304: beyond the
512 slots of the tile's LDS table, the global route), one frame of 352 x 1216 with blocks of 18."""
import ctypes

import numpy as np
import pytest

import connectivity_restatement as CR
import planes_restatement as R
import test_gpu_stream_order as SO
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

gpu = pytest.mark.gpu
f32, i32, u8 = np.float32, np.int32, np.uint8
MAX_ROWS, MAX_COLS, MAX_BATCH = 352, 1216, 8
LITERAL_PIXELS = 10000


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, MAX_ROWS, MAX_COLS, MAX_BATCH)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


_want = {}


def want(depth, labels, n, **kw):
    """The restatement of one frame, computed once per input and shared (never modified)."""
    key = (depth.shape, depth.tobytes(), labels.tobytes(), n, tuple(sorted(kw.items())))
    if key not in _want:
        f = R.literal_planes if depth.size <= LITERAL_PIXELS else R.closed_planes
        _want[key] = f(depth, labels, n, **kw)
        for a in _want[key]:
            a.setflags(write=False)
    return _want[key]


def fits_of(d_fits):
    return host(d_fits).view(api.PLANE_FIT_DTYPE)[..., 0]


def differ(got, wanted, what):
    assert got.shape == wanted.shape and got.dtype == wanted.dtype, (what, got.shape, got.dtype, wanted.shape, wanted.dtype)
    if got.dtype == f32:
        neq = got.view(np.uint32) != wanted.view(np.uint32)
    else:
        neq = np.array([a.tobytes() != b.tobytes() for a, b in zip(got.reshape(-1), wanted.reshape(-1))]).reshape(got.shape)
    assert not neq.any(), f"{what}: {int(neq.sum())} elements differ, first at {tuple(np.argwhere(neq)[0])}: {got[tuple(np.argwhere(neq)[0])]} vs {wanted[tuple(np.argwhere(neq)[0])]}"


def check(ctx, depth, labels, n, what, **kw):
    """One device call on the batch (depth, labels) with d_fits against the restatement of every frame; returns (out, fits)."""
    depth, labels = np.ascontiguousarray(depth, f32), np.ascontiguousarray(labels, i32)
    d_out, d_fits = ctx.superpixel_planes_dev(dev(depth), dev(labels), n, dev(np.full(depth.shape, -7.0, f32)), True, **kw)
    out, fits = host(d_out), fits_of(d_fits)
    assert fits.shape == (len(depth), n)
    for f in range(len(depth)):
        o, ft = want(depth[f], labels[f], n, **kw)
        differ(out[f], o, f"{what} frame {f}: output")
        differ(fits[f], ft, f"{what} frame {f}: fits")
    return out, fits


def dirty(ctx, b):
    """Leaves both scratch planes of the context dirty up to their last record: a call of the largest n_labels a batch of b frames
    may name, with no d_fits, on full frames whose labels run through all of them.  The first plane then holds non-zero sums and
    the 0xFFFFFFFF minima of cleared records, the second plane fits.  (No public call can fill the planes with one byte value.)"""
    import torch
    n = api.superpixel_planes_max_labels(MAX_ROWS, MAX_COLS, MAX_BATCH, b)
    lab = (torch.arange(b * MAX_ROWS * MAX_COLS, dtype=torch.int64, device="cuda") % n).to(torch.int32).reshape(b, MAX_ROWS, MAX_COLS)
    z = torch.full((b, MAX_ROWS, MAX_COLS), 7.0, dtype=torch.float32, device="cuda")
    ctx.superpixel_planes_dev(z, lab, n, refit_tol=0.5)


# ------------------------------------------------------------------------------------------------------------- against the restatement
SHAPES = [(1, 1, "one"), (1, 70, "blocks4"), (3, 33, "blocks4"), (17, 65, "voronoi"), (40, 130, "blocks8"), (33, 257, "one"), (24, 96, "pixels")]


def labels_for(rows, cols, kind):
    if kind == "one":
        return np.zeros((rows, cols), i32), 1
    if kind == "pixels":
        return R.pixel_labels(rows, cols)
    if kind == "voronoi":
        return R.voronoi(rows, cols), 12
    return R.block_labels(rows, cols, int(kind[6:]))


@gpu
@pytest.mark.parametrize("rows,cols,kind", SHAPES)
def test_shapes(ctx, rows, cols, kind):
    lab, n = labels_for(rows, cols, kind)
    depth = np.stack([R.sparse_depth(rows, cols, d, 10 + i) for i, d in enumerate((0.05, 0.3, 1.0))])
    labels = np.stack([lab] * 3)
    _, fits = check(ctx, depth, labels, n, f"{rows}x{cols} {kind}")
    check(ctx, depth, labels, n, f"{rows}x{cols} {kind}, refit", refit_tol=0.05, keep_returns=False)
    if kind == "pixels":
        assert n == 2304 and (fits["kind"] != R.PLANE).all() and (fits[2]["kind"] == R.CONSTANT).sum() > 2000
    if rows * cols > 500 and kind != "pixels":
        assert (fits["kind"] == R.PLANE).any()


@gpu
def test_one_kitti_frame_with_blocks_of_18(ctx):
    lab, n = R.block_labels(352, 1216, 18)
    z, _, _, _ = R.facet_scene(352, 1216, 40, 0.05, 3)
    z.reshape(-1)[::1001] = np.resize(np.array(R.SPECIALS, f32), len(z.reshape(-1)[::1001]))
    _, fits = check(ctx, z[None], lab[None], n, "352x1216 blocks of 18")
    _, fits2 = check(ctx, z[None], lab[None], n, "352x1216 blocks of 18, refit", refit_tol=0.02)
    assert n == 20 * 68 and (fits["kind"] == R.PLANE).mean() > 0.9 and (fits2["used"] < fits["used"]).any()


@gpu
def test_a_dense_frame_of_one_label(ctx):
    """Every pixel of 352 x 1216 a return of one label: 428032 atomics into one record, and centred terms beyond 2^64 (n Suw is about
    2^67), the 128-bit part of the solve."""
    g = np.random.Generator(np.random.PCG64(5))
    V, U = np.mgrid[0:352, 0:1216]
    z = (1.0 / (0.011 + 5.0 * U / 1216 + 4.0 * V / 352 + g.uniform(0, 0.5, U.shape))).astype(f32)
    lab = np.zeros((1, 352, 1216), i32)
    _, fits = check(ctx, z[None], lab, 1, "dense one label", keep_returns=False)
    assert fits[0, 0]["kind"] == R.PLANE and fits[0, 0]["seen"] == 352 * 1216
    check(ctx, z[None], lab, 1, "dense one label, refit", keep_returns=False, refit_tol=0.3)


@gpu
@pytest.mark.parametrize("rows,cols", [(17, 65), (24, 70)])
def test_adversarial_label_planes(ctx, rows, cols):
    cases = R.plane_cases(rows, cols)
    assert {c[0].split()[0] for c in cases} == set(R.PLANES)
    planes = np.stack([p for _, p in cases])
    assert (planes[5] < 0).any() and (planes[5] >= 6).any()     # labels outside the range
    depth = np.stack([R.sparse_depth(rows, cols, 0.4, 20 + i) for i in range(len(planes))])
    out, _ = check(ctx, depth, planes, 6, f"adversarial {rows}x{cols}, 6 labels")
    outside = (planes < 0) | (planes >= 6)
    assert not out[outside].view(np.uint32).any() and (depth[outside] > 0.1).any()
    check(ctx, depth, planes, max(rows, 6), f"adversarial {rows}x{cols}, {max(rows, 6)} labels", refit_tol=0.5, min_extent=1)


GRID = [(mp, me, tol, keep) for mp in (3, 8) for me in (1, 2, 5) for tol in (0.0, 0.05, 0.5) for keep in (True, False)]


@gpu
def test_parameter_grid(ctx):
    rows, cols = 24, 96
    lab, n = R.block_labels(rows, cols, 8)
    z, flab, fn, _, _ = R.outlier_scene(rows, cols, 6, 0.25, 2, facet=1, share=0.2, factor=2.0)
    depth = np.stack([R.sparse_depth(rows, cols, 0.15, 31), z])
    seen = set()
    for mp, me, tol, keep in GRID:
        kw = dict(min_points=mp, min_extent=me, refit_tol=tol, keep_returns=keep)
        out, fits = check(ctx, depth, np.stack([lab, lab]), n, f"grid {kw}", **kw)
        seen.add((out.tobytes(), fits.tobytes()))
    assert len(seen) >= 12                                      # the parameters matter on these frames
    check(ctx, z[None], flab[None], fn, "outlier scene", refit_tol=0.25)
    check(ctx, depth, np.stack([lab, lab]), n, "other bounds", valid_thresh=0.5, max_depth=20.0)


@gpu
@pytest.mark.parametrize("b", [1, 3, 8])
def test_batches_on_dirty_scratch(ctx, b):
    """Frame f of a batch equals the frame alone, whatever the scratch planes held: every call here runs behind one that dirtied both
    planes (dirty)."""
    rows, cols = 40, 130
    lab, n = R.block_labels(rows, cols, 8)
    depth = np.stack([R.sparse_depth(rows, cols, 0.1 + 0.05 * f, 40 + f) for f in range(b)])
    labels = np.stack([np.roll(lab, f, axis=1) for f in range(b)])
    for kw in ({}, dict(refit_tol=0.1)):
        dirty(ctx, b)
        out, fits = check(ctx, depth, labels, n, f"batch of {b} {kw}", **kw)
        for f in {0, b - 1}:
            dirty(ctx, 1)
            o1, f1 = check(ctx, depth[f][None], labels[f][None], n, f"frame {f} alone {kw}", **kw)
            differ(o1[0], out[f], f"frame {f} alone against its place in the batch")
            differ(f1[0], fits[f], f"frame {f} alone against its place in the batch: fits")
        # without d_fits (the fits on the second scratch plane): the same output
        dirty(ctx, b)
        differ(host(ctx.superpixel_planes_dev(dev(depth), dev(labels), n, **kw)), out, f"without d_fits {kw}")


@gpu
def test_in_place(ctx):
    rows, cols = 40, 130
    lab, n = R.block_labels(rows, cols, 8)
    depth = np.stack([R.sparse_depth(rows, cols, 0.2, 50 + f) for f in range(3)])
    labels = np.stack([lab] * 3)
    for kw in ({}, dict(refit_tol=0.1, keep_returns=False)):
        out, fits = check(ctx, depth, labels, n, f"out of place {kw}", **kw)
        d = dev(depth)
        same, d_fits = ctx.superpixel_planes_dev(d, dev(labels), n, d, True, **kw)
        assert same.data_ptr() == d.data_ptr()
        differ(host(d), out, f"in place {kw}")
        differ(fits_of(d_fits), fits, f"in place {kw}: fits")
    d = dev(R.sparse_depth(3, 33, 0.3, 1))                      # the scalar paint, a 2-D tensor
    l2, n2 = R.block_labels(3, 33, 4)
    ctx.superpixel_planes_dev(d, dev(l2), n2, d)
    differ(host(d), want(R.sparse_depth(3, 33, 0.3, 1), l2, n2)[0], "in place, 3x33")


@gpu
def test_host_entry_point_and_module_level_call(ctx):
    rows, cols = 40, 130
    lab, n = R.block_labels(rows, cols, 8)
    z = R.sparse_depth(rows, cols, 0.2, 60)
    o, ft = want(z, lab, n, refit_tol=0.1)
    out, fits = ctx.superpixel_planes(z, lab, n, refit_tol=0.1)
    differ(out, o, "host output")
    differ(fits, ft, "host fits")
    wide_z, wide_l = np.full((rows, 140), 3.0, f32), np.full((rows, 150), 1, i32)
    wide_z[:, :cols], wide_l[:, :cols] = z, lab
    out, fits = ctx.superpixel_planes(wide_z[:, :cols], wide_l[:, :cols], n, refit_tol=0.1)
    differ(out, o, "pitched inputs")
    out, fits = api.fit_superpixel_planes(z, lab, n, refit_tol=0.1)
    differ(out, o, "fit_superpixel_planes")
    differ(fits, ft, "fit_superpixel_planes: fits")
    pl, pn = R.pixel_labels(24, 96)                              # 2304 labels on a small frame: the default context is large enough
    zz = R.sparse_depth(24, 96, 0.5, 61)
    differ(api.fit_superpixel_planes(zz, pl, pn)[0], want(zz, pl, pn)[0], "fit_superpixel_planes, 2304 labels")
    # the C entry point itself: in place on a pitched plane, no fits
    p = api.make_planes_params()
    pitched = np.full((rows, 200), -3.0, f32)
    pitched[:, :cols] = z
    st = L.lib().dcmt_superpixel_planes(ctx._h, pitched.ctypes.data, 800, lab.ctypes.data, cols * 4, rows, cols, n, ctypes.byref(p), pitched.ctypes.data, 800, None)
    assert st == L.OK
    differ(np.ascontiguousarray(pitched[:, :cols]), want(z, lab, n)[0], "host, in place, pitched")
    assert (pitched[:, cols:] == -3.0).all()


# ------------------------------------------------------------------------------------------------------------- stream order, the chain
def stream_case(rows=40, cols=56, b=3, n_labels=9):
    def inputs(which):
        g = np.random.Generator(np.random.PCG64(71 + which))
        return {"labels": SO.salt_and_pepper(g, (b, rows, cols)), "sparse": np.stack([R.sparse_depth(rows, cols, 0.2, 700 + 10 * which + f) for f in range(b)])}

    def call(ctx, t, st):
        ctx.superpixel_planes_dev(t["sparse"], t["labels"], n_labels, t["planes"], t["fits"], stream=st, refit_tol=0.2)

    def wrap(ctx, t, st):
        planes, fits = ctx.superpixel_planes_dev(t["sparse"], t["labels"], n_labels, None, True, stream=st, refit_tol=0.2)
        return {"planes": planes, "fits": fits}

    def expect(inp):
        w = [want(inp["sparse"][f], inp["labels"][f], n_labels, refit_tol=0.2) for f in range(b)]
        return {"planes": np.stack([x[0] for x in w]), "fits": np.stack([x[1] for x in w]).view(u8).reshape(b, n_labels, 48)}

    outs = {"planes": SO.Out((b, rows, cols), f32), "fits": SO.Out((b, n_labels, 48), u8)}
    return SO.Case("superpixel_planes", (rows, cols, b), inputs, outs, call, expect, None, wrap)


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
def test_chain_slic_connectivity_planes_completion_on_one_stream():
    """slic_labels_dev -> slic_connectivity_dev -> superpixel_planes_dev -> complete_dev on one non-default stream with no host
    synchronisation in between, against the same chain on the CPU: the oracle's SLIC, the sequential connectivity restatement, the
    plane restatement, the oracle's labelled completion."""
    import torch
    rows, cols, b, step, nc = 70, 130, 2, 16, 40
    lab_img = np.stack([synth.synth_lab(rows, cols, 40 + f) for f in range(b)])
    sparse = SO.sparse_frames(b, rows, cols, 900)
    params = api.make_params(spec_fill_iters=SO.SPEC)
    s = torch.cuda.Stream()
    with api.Context(0, rows, cols, b) as c:
        d_img, d_sparse = dev(lab_img), dev(sparse)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            labels, n = c.slic_labels_dev(d_img, step, nc, stream=s.cuda_stream)
            conn, max_labels, _ = c.slic_connectivity_dev(labels, n, stream=s.cuda_stream)
            planes, fits = c.superpixel_planes_dev(d_sparse, conn, max_labels, None, True, stream=s.cuda_stream)
            dense = c.complete_dev(planes, None, params, d_labels=conn, n_labels=max_labels, stream=s.cuda_stream)
        s.synchronize()
        got = {"conn": host(conn), "planes": host(planes), "fits": fits_of(fits), "dense": host(dense)}
    assert max_labels <= api.superpixel_planes_max_labels(rows, cols, b, b)
    for f in range(b):
        raw, n_cpu = SO.O().slic(lab_img[f], step, nc)
        assert n_cpu == n
        conn_cpu, count = CR.sequential(raw, n)
        differ(got["conn"][f], conn_cpu, f"frame {f}: connected labels")
        o, ft = want(sparse[f], conn_cpu, max_labels)
        differ(got["planes"][f], o, f"frame {f}: planes")
        differ(got["fits"][f], ft, f"frame {f}: fits")
        y, info = SO.O().interpolate_with_superpixels(o, conn_cpu, max_labels, return_info=True)
        assert info["rc"] == 0 and info["fill_iters"] < SO.SPEC
        differ(got["dense"][f], y, f"frame {f}: dense")
        filled = (o > 0).mean()
        assert filled > (sparse[f] > 0).mean() and (ft["kind"][:count] != R.NONE).any()
    print(f"[planes] chain {rows}x{cols}: {n} centres, max_labels {max_labels}; valid {float((sparse > 0).mean()):.3f} -> planes {float((got['planes'] > 0).mean()):.3f} -> dense {float((got['dense'] > 0).mean()):.3f}")


# ------------------------------------------------------------------------------------------------------------- refusals
@gpu
def test_refusals(ctx):
    import torch
    lib = L.lib()
    r, c, b, nl = 8, 16, 3, 4
    n = r * c * b
    buf = torch.full((16 * n,), 0x5A, dtype=torch.uint8, device="cuda")
    z = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    lab = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    fits = torch.full((b * nl * 48,), 0xA5, dtype=torch.uint8, device="cuda")
    good = api.make_planes_params()
    P = lambda t, off=0: t.data_ptr() + off

    def call(zz=P(z), ll=P(lab), oo=P(out), ff=P(fits), n_labels=nl, rows=r, cols=c, batch=b, h=ctx._h, p=good):
        return lib.dcmt_superpixel_planes_dev(h, zz, ll, rows, cols, batch, n_labels, None if p is None else ctypes.byref(p), oo, ff, None)

    def params(**kw):
        p = api.make_planes_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    most = MAX_ROWS * MAX_COLS * MAX_BATCH // (24 * b)
    bad = [call(zz=None), call(ll=None), call(oo=None), call(p=None), call(h=None),
           call(zz=P(z, 2)), call(ll=P(lab, 2)), call(oo=P(out, 2)), call(ff=P(fits, 4)),
           call(n_labels=0), call(n_labels=-3), call(n_labels=most + 1), call(n_labels=most + 1, ff=None),
           call(rows=MAX_ROWS + 1), call(cols=MAX_COLS + 1), call(batch=MAX_BATCH + 1), call(rows=0), call(cols=0), call(batch=0),
           call(zz=P(buf), oo=P(buf, 4)), call(zz=P(buf), oo=P(buf, 4 * n - 4)), call(zz=P(buf, 64), oo=P(buf)),
           call(zz=P(buf), ll=P(buf)), call(zz=P(buf), ll=P(buf, 4 * n - 4)), call(ll=P(buf), oo=P(buf, 4 * n - 4)), call(ll=P(buf, 8), oo=P(buf)),
           call(ff=P(z)), call(ff=P(lab, 4 * n - 8)), call(ff=P(out, 8)), call(zz=P(buf, 48 * b * nl - 8), ff=P(buf)),
           call(p=params(valid_thresh=0.06)), call(p=params(valid_thresh=float("nan"))), call(p=params(valid_thresh=float("inf"))), call(p=params(valid_thresh=-1.0)),
           call(p=params(max_depth=0.05)), call(p=params(max_depth=16385.0)), call(p=params(max_depth=float("inf"))), call(p=params(max_depth=float("nan"))),
           call(p=params(min_points=2)), call(p=params(min_points=-1)), call(p=params(min_extent=0)), call(p=params(refit_tol=1.0)),
           call(p=params(refit_tol=-0.5)), call(p=params(refit_tol=float("nan"))), call(p=params(keep_returns=2)), call(p=params(keep_returns=-1))]
    assert bad == [L.E_INVALID] * len(bad), bad
    torch.cuda.synchronize()
    assert (host(out) == -7.0).all() and (host(fits) == 0xA5).all() and (host(buf) == 0x5A).all() and (host(z) == 7.0).all()      # nothing written
    # what is allowed: touching buffers, in place, no fits, the bound itself, the extreme parameters
    assert call(ff=None) == L.OK and call(oo=P(z)) == L.OK
    assert call(zz=P(buf), oo=P(buf, 4 * n), ff=None) == L.OK and call(zz=P(buf), ll=P(buf, 4 * n), oo=P(buf, 8 * n), ff=P(buf, 12 * n)) == L.OK
    assert call(n_labels=most, ff=None) == L.OK
    assert call(ff=None, p=params(valid_thresh=0.0625, max_depth=16384.0, min_points=2 ** 31 - 1, min_extent=2 ** 31 - 1, refit_tol=0.999)) == L.OK
    assert call() == L.OK
    torch.cuda.synchronize()
    f = host(fits).view(api.PLANE_FIT_DTYPE).reshape(b, nl)
    assert (host(out) == 7.0).all() and (f["kind"][:, 0] == R.PLANE).all() and (f["kind"][:, 1:] == R.NONE).all() and (f["seen"][:, 0] == r * c).all()
    # the host form
    hz, hl, ho = np.full((r, c), 7.0, f32), np.zeros((r, c), i32), np.full((r, c), -7.0, f32)
    hf = np.zeros(nl, api.PLANE_FIT_DTYPE)
    one = lambda *a: lib.dcmt_superpixel_planes(ctx._h, *a)
    gp = ctypes.byref(good)
    assert one(hz.ctypes.data, c * 4, hl.ctypes.data, c * 4, r, c, nl, gp, ho.ctypes.data, c * 4, hf.ctypes.data) == L.OK and (ho == 7.0).all() and hf[0]["kind"] == R.PLANE
    ho[:] = -7.0
    bad = [one(None, c * 4, hl.ctypes.data, c * 4, r, c, nl, gp, ho.ctypes.data, c * 4, None), one(hz.ctypes.data, c * 4, None, c * 4, r, c, nl, gp, ho.ctypes.data, c * 4, None),
           one(hz.ctypes.data, c * 4, hl.ctypes.data, c * 4, r, c, nl, gp, None, c * 4, None), one(hz.ctypes.data, c * 4, hl.ctypes.data, c * 4, r, c, nl, None, ho.ctypes.data, c * 4, None),
           one(hz.ctypes.data, c * 4 - 4, hl.ctypes.data, c * 4, r, c, nl, gp, ho.ctypes.data, c * 4, None), one(hz.ctypes.data, c * 4, hl.ctypes.data, c * 4 - 4, r, c, nl, gp, ho.ctypes.data, c * 4, None),
           one(hz.ctypes.data, c * 4, hl.ctypes.data, c * 4, r, c, nl, gp, ho.ctypes.data, c * 4 - 4, None), one(hz.ctypes.data, c * 4, hl.ctypes.data, c * 4, r, c, 0, gp, ho.ctypes.data, c * 4, None),
           one(hz.ctypes.data, c * 4, hl.ctypes.data, c * 4, r, c, 1 << 30, gp, ho.ctypes.data, c * 4, None), one(hz.ctypes.data, c * 4, hl.ctypes.data, c * 4, MAX_ROWS + 1, c, nl, gp, ho.ctypes.data, c * 4, None),
           one(hz.ctypes.data, c * 4, hl.ctypes.data, c * 4, r, c, nl, ctypes.byref(params(min_points=1)), ho.ctypes.data, c * 4, None)]
    assert bad == [L.E_INVALID] * len(bad) and (ho == -7.0).all(), bad
    with pytest.raises(api.DcmtError) as e:
        ctx.superpixel_planes_dev(dev(np.zeros((1, r, c), f32)), dev(np.zeros((1, r, c), i32)), 0)
    assert e.value.status == L.E_INVALID
    with pytest.raises(ValueError):
        ctx.superpixel_planes_dev(dev(np.zeros((1, r, c), f32)), dev(np.zeros((1, r, c), i32)), 1, min_points=2)
    # a frame of more than 2^21 pixels, on a context that allows it
    with api.Context(0, 1025, 2048, 1) as big:
        zz, ll = torch.zeros((1025, 2048), dtype=torch.float32, device="cuda"), torch.zeros((1025, 2048), dtype=torch.int32, device="cuda")
        assert lib.dcmt_superpixel_planes_dev(big._h, zz.data_ptr(), ll.data_ptr(), 1025, 2048, 1, 1, gp, zz.data_ptr(), None, None) == L.E_INVALID
        assert lib.dcmt_superpixel_planes_dev(big._h, zz.data_ptr(), ll.data_ptr(), 1024, 2048, 1, 1, gp, zz.data_ptr(), None, None) == L.OK
        torch.cuda.synchronize()
