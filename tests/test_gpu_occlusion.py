"""The occlusion filter of projected LiDAR returns on the device: dcmt_sparse_occlusion_dev, its payload form, its host form and
filter_occluded_returns, bit for bit against the restatements of tests/occlusion_restatement.py (test_occlusion.py holds the two
restatements against each other).  The literal restatement is the reference at the default parameters wherever a frame has at most
10000 pixels; elsewhere it is the vectorised one, which test_occlusion.py shows to be the same bits.

Shapes.  k_occl takes tiles of 64 x 64 pixels with a halo of (rx, ry), a wave 64 columns, the mask of the in-place route 32 pixels a
word: 1 x 1, 1 x 65 (a second tile of one column, a third mask word of one bit), 17 x 1, 5 x 3 (smaller than the window), 33 x 130 and
65 x 129 (partial tiles in both directions), one frame of 352 x 1216, batches of 1, 3 and 5 frames of 33 x 130."""
import ctypes

import numpy as np
import pytest

import nearest_restatement as NR
import occlusion_restatement as R
import test_gpu_stream_order as SO
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

gpu = pytest.mark.gpu
f32, u16, u32, i16 = np.float32, np.uint16, np.uint32, np.int16
MAX_ROWS, MAX_COLS, MAX_BATCH = 352, 1216, 5
LITERAL_PIXELS = 10000
RADII = [(0, 0), (3, 6), (8, 16), (8, 0), (0, 16)]
TOLS = [0, 655, 1 << 20]
SHAPES = [(1, 1), (1, 65), (17, 1), (5, 3), (33, 130), (65, 129)]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, MAX_ROWS, MAX_COLS, MAX_BATCH)
    yield c
    c.close()


def dev(a):
    import torch
    a = np.array(a, order="C")                                  # (a copy: the shared inputs are read-only)
    return torch.from_numpy(a.view(i16) if a.dtype == u16 else a).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(u16) if a.dtype == i16 else a


_want = {}


def want(plane, **kw):
    """The restatement of one frame, computed once per input and shared (never modified): (out, removed)."""
    key = (plane.shape, plane.dtype.str, plane.tobytes(), tuple(sorted(kw.items())))
    if key not in _want:
        f = R.literal_occlusion if plane.size <= LITERAL_PIXELS and not kw else R.shifted_occlusion
        out, n = f(plane, **kw)
        out.setflags(write=False)
        _want[key] = (out, n)
    return _want[key]


def differ(got, wanted, what):
    assert got.shape == wanted.shape and got.dtype == wanted.dtype, (what, got.shape, got.dtype, wanted.shape, wanted.dtype)
    w = {2: u16, 4: u32}[got.dtype.itemsize]
    neq = np.ascontiguousarray(got).view(w) != np.ascontiguousarray(wanted).view(w)
    assert not neq.any(), f"{what}: {int(neq.sum())} elements differ, first at {tuple(np.argwhere(neq)[0])}: {got[tuple(np.argwhere(neq)[0])]} vs {wanted[tuple(np.argwhere(neq)[0])]}"


def check(ctx, planes, what, **kw):
    """The batch `planes` (f32 or the payload) out of place and in place, both with d_removed, against the restatement of every frame;
    the two routes byte for byte.  Returns (out, removed)."""
    planes = np.ascontiguousarray(planes)
    payload = planes.dtype == u16
    fill = np.full(planes.shape, 0xA5A5 if payload else -7.0, planes.dtype)
    d_out, d_rem = ctx.sparse_occlusion_dev(dev(planes), dev(fill), removed=True, u16=payload, **kw)
    d_in = dev(planes)
    same, d_rem2 = ctx.sparse_occlusion_dev(d_in, d_in, removed=True, u16=payload, **kw)
    assert same.data_ptr() == d_in.data_ptr()
    out, rem, out2, rem2 = host(d_out), host(d_rem), host(d_in), host(d_rem2)
    for f in range(len(planes)):
        o, n = want(planes[f], **kw)
        differ(out[f], o, f"{what} frame {f}: out of place")
        differ(out2[f], o, f"{what} frame {f}: in place")
        assert rem[f] == n and rem2[f] == n, f"{what} frame {f}: removed {rem[f]} / {rem2[f]} against {n}"
    assert out.tobytes() == out2.tobytes()
    return out, rem


# ------------------------------------------------------------------------------------------------------------- against the restatement
@gpu
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_shapes(ctx, rows, cols):
    z = np.stack([R.sparse_plane(rows, cols, d, 10 + i) for i, d in enumerate((0.1, 0.6))])
    v = np.stack([R.payload_plane(rows, cols, d, 10 + i) for i, d in enumerate((0.1, 0.6))])
    total = 0
    for rx, ry in RADII:
        for tol in TOLS:
            kw = {} if (rx, ry, tol) == (3, 6, 655) else dict(rx=rx, ry=ry, tol_code=tol)
            _, rem = check(ctx, z, f"{rows}x{cols} {kw}", **kw)
            _, rem16 = check(ctx, v, f"{rows}x{cols} payload {kw}", **kw)
            if (rx, ry) == (0, 0) or tol == 1 << 20:
                assert not rem.any() and not rem16.any()
            total += int(rem.sum()) + int(rem16.sum())
    assert total > 0 or rows * cols < 50
    check(ctx, v, f"{rows}x{cols} payload, another scale", scale=0.01)
    check(ctx, z, f"{rows}x{cols} other bounds", valid_thresh=0.5, max_depth=20.0, tol_code=50, rx=2, ry=1)


@gpu
def test_one_kitti_frame(ctx):
    scene, see_through = R.lidar_scene()
    z = R.sparse_plane(352, 1216, 0.05, 3)
    out, rem = check(ctx, np.stack([scene, z]), "352x1216")
    assert not out[0][see_through].any() and rem[0] >= see_through.sum() > 300 and rem[1] > 100
    check(ctx, R.payload_plane(352, 1216, 0.05, 4)[None], "352x1216 payload")
    check(ctx, z[None], "352x1216 at the largest radii", rx=8, ry=16, tol_code=100)


def dirty(ctx, how):
    """Leaves both scratch planes of the context dirty: the labels of a speckle filter or of the SLIC connectivity over full frames."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    if how == "speckles":
        ctx.filter_speckles_dev(torch.randint(-16, 2000, (MAX_BATCH, MAX_ROWS, MAX_COLS), dtype=torch.int16, device="cuda", generator=g))
    else:
        ctx.slic_connectivity_dev(torch.randint(0, 1300, (MAX_BATCH, MAX_ROWS, MAX_COLS), dtype=torch.int32, device="cuda", generator=g), 1300)


@gpu
@pytest.mark.parametrize("b,how", [(1, "speckles"), (3, "connectivity"), (5, "speckles")])
def test_batches_on_dirty_scratch(ctx, b, how):
    """Frame f of a batch equals the frame alone, whatever the scratch planes held, and d_removed is zeroed for a frame with nothing
    removed (the middle frame holds no returns)."""
    import torch
    rows, cols = 33, 130
    z = np.stack([R.sparse_plane(rows, cols, 0.2 + 0.1 * f, 40 + f) for f in range(b)])
    if b > 1:
        z[b // 2] = 0
    for planes in (z, np.stack([R.payload_plane(rows, cols, 0.3, 50 + f) for f in range(b)])):
        payload = planes.dtype == u16
        dirty(ctx, how)
        out, rem = check(ctx, planes, f"batch of {b}")
        d_in = dev(planes)
        d_rem = torch.full((b,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        dirty(ctx, how)
        ctx.sparse_occlusion_dev(d_in, d_in, d_removed=d_rem, u16=payload)
        assert host(d_rem).tolist() == rem.tolist() and host(d_in).tobytes() == out.tobytes()
        if b > 1 and not payload:
            assert rem[b // 2] == 0 and rem[0] > 0
        for f in {0, b - 1}:
            dirty(ctx, how)
            o1, r1 = check(ctx, planes[f][None], f"frame {f} alone")
            differ(o1[0], out[f], f"frame {f} alone against its place in the batch")
            assert r1[0] == rem[f]


# ------------------------------------------------------------------------------------------------------------- planted cases
@gpu
@pytest.mark.parametrize("rx,ry", [(3, 6), (8, 16), (1, 2)])
def test_occluders_across_tile_seams(ctx, rx, ry):
    """A return beside a seam of the 64 x 64 tiles (columns 63 | 64, rows 63 | 64) and an occluder exactly rx / ry away on the other side
    of it removes the return; at rx + 1 / ry + 1 it stays."""
    rows, cols = 100, 140
    frames, expect = [], []
    for (y, x), sy, sx in (((64, 64), -1, -1), ((63, 63), 1, 1), ((64, 63), -1, 1), ((63, 64), 1, -1)):
        for dy, dx, hit in ((ry, rx, True), (ry + 1, rx, False), (ry, rx + 1, False), (ry, 0, True), (0, rx, True), (ry + 1, 0, False), (0, rx + 1, False)):
            z = np.zeros((rows, cols), f32)
            z[y, x], z[y + sy * dy, x + sx * dx] = 50.0, 2.0
            frames.append(z)
            expect.append(hit)
    for i in range(0, len(frames), MAX_BATCH):
        out, rem = check(ctx, np.stack(frames[i:i + MAX_BATCH]), f"seams {rx} {ry}", rx=rx, ry=ry)
        assert rem.tolist() == [int(h) for h in expect[i:i + MAX_BATCH]]


@gpu
def test_nothing_crosses_a_frame_or_wraps_a_row(ctx):
    """A near return in the last row of frame f does not touch the first row of frame f + 1, nor the last column of a row the first
    column of the next."""
    rows, cols = 33, 130
    z = np.zeros((3, rows, cols), f32)
    z[0, rows - 1, :] = 2.0                                       # the whole last row of frame 0 is near
    z[1, 0, :] = 50.0                                             # ... the whole first row of frame 1 far
    z[1, rows - 1, 7], z[2, 0, 7] = 2.0, 50.0
    z[2, 10, cols - 1], z[2, 11, 0], z[2, 30, 0], z[2, 29, cols - 1] = 2.0, 50.0, 2.0, 50.0     # (19 rows apart: beyond any ry)
    for kw in ({}, dict(rx=8, ry=16), dict(rx=8, ry=0), dict(rx=0, ry=16)):
        out, rem = check(ctx, z, f"frame boundaries {kw}", **kw)
        assert not rem.any() and out.tobytes() == z.tobytes()
    v = np.where(z > 0, np.rint(z * 256), 0).astype(u16)
    assert not check(ctx, v, "frame boundaries, payload", rx=8, ry=16)[1].any()


@gpu
def test_a_removed_return_still_hides_others(ctx):
    """A hides B and B, though removed, still hides C, which A does not reach: what an in-place call that read its own output would get
    wrong.  Horizontally across the tile seam at column 64, vertically across the one at row 64; and whole rows of returns at three depths, six columns apart."""
    z = np.zeros((2, 80, 140), f32)
    z[0, 5, 60], z[0, 5, 63], z[0, 5, 66] = 2.0, 10.0, 50.0
    z[0, 58, 9], z[0, 64, 9], z[0, 70, 9] = 2.0, 10.0, 50.0
    z[1, ::7, :] = 50.0
    z[1, ::7, ::6] = 10.0
    z[1, ::7, ::12] = 2.0
    out, rem = check(ctx, z, "chains")
    assert rem[0] == 4 and out[0, 5, 63] == 0 and out[0, 5, 66] == 0 and out[0, 64, 9] == 0 and out[0, 70, 9] == 0 and out[0, 5, 60] == 2.0
    assert (out[1][z[1] == 50.0] == 0).all() and (out[1][z[1] == 10.0] == 10.0).all() and (out[1][z[1] == 2.0] == 2.0).all()
    assert R.shifted_occlusion(z[0], rx=2, ry=5)[1] == 0          # A does not reach C: only B, removed, hides it


# ------------------------------------------------------------------------------------------------------------- alignment, forms
@gpu
def test_pointers_offset_by_one_element(ctx):
    import torch
    rows, cols, b = 33, 130, 3
    n = b * rows * cols
    for planes, tdt, fill in ((np.stack([R.sparse_plane(rows, cols, 0.3, 60 + f) for f in range(b)]), torch.float32, -7.0),
                              (np.stack([R.payload_plane(rows, cols, 0.3, 60 + f) for f in range(b)]), torch.int16, 0x2525)):
        payload = planes.dtype == u16
        for off_in, off_out in ((1, 0), (0, 1), (1, 1), (3, 2)):
            src = torch.full((n + 8,), fill, dtype=tdt, device="cuda")
            dst = torch.full((n + 8,), fill, dtype=tdt, device="cuda")
            vin, vout = src[off_in:off_in + n].view(b, rows, cols), dst[off_out:off_out + n].view(b, rows, cols)
            vin.copy_(dev(planes))
            assert vin.data_ptr() % 16 == (off_in * planes.itemsize) % 16
            _, rem = ctx.sparse_occlusion_dev(vin, vout, removed=True, u16=payload)
            got = host(vout)
            for f in range(b):
                differ(got[f], want(planes[f])[0], f"offsets {off_in} {off_out} frame {f}")
                assert host(rem)[f] == want(planes[f])[1]
            h = host(dst)
            assert (h[:off_out] == h.dtype.type(fill)).all() and (h[off_out + n:] == h.dtype.type(fill)).all()       # nothing outside the output
            ctx.sparse_occlusion_dev(vin, vin, u16=payload)                                                       # in place at that offset
            assert host(vin).tobytes() == got.tobytes()
            h = host(src)
            assert (h[:off_in] == h.dtype.type(fill)).all() and (h[off_in + n:] == h.dtype.type(fill)).all()


@gpu
def test_payload_form_equals_the_f32_form_on_the_ingested_depths(ctx):
    v = np.stack([R.payload_plane(65, 129, 0.4, 70 + f) for f in range(2)])
    for kw in ({}, dict(scale=0.01, rx=5, ry=3, tol_code=200)):
        pkw = {k: x for k, x in kw.items() if k != "scale"}
        z = R.metres(v, kw.get("scale", 1.0 / 256.0))
        out16, rem16 = ctx.sparse_occlusion_dev(dev(v), removed=True, u16=True, **kw)
        out32, rem32 = ctx.sparse_occlusion_dev(dev(z), removed=True, **pkw)
        out16, out32 = host(out16), host(out32)
        assert host(rem16).tolist() == host(rem32).tolist() and host(rem16).sum() > 0
        assert np.array_equal(out16 != v, out32.view(u32) != z.view(u32)) and not out16[out16 != v].any()


@gpu
def test_host_entry_point_and_module_level_call(ctx):
    rows, cols = 33, 130
    z = R.sparse_plane(rows, cols, 0.3, 80)
    o, n = want(z)
    out, removed = ctx.sparse_occlusion(z)
    differ(out, o, "host output")
    assert removed == n > 0
    wide = np.full((rows, 150), 3.0, f32)
    wide[:, :cols] = z
    out, removed = ctx.sparse_occlusion(wide[:, :cols])
    differ(out, o, "pitched input")
    assert removed == n
    differ(api.filter_occluded_returns(z), o, "filter_occluded_returns")
    differ(api.filter_occluded_returns(z, rx=8, ry=16, inv_depth_tol=0.002), want(z, rx=8, ry=16, tol_code=131)[0], "filter_occluded_returns, parameters")
    # the C entry point itself: in place on a pitched plane, with and without the count
    p = api.make_occlusion_params()
    for cnt in (ctypes.c_uint32(77), None):
        pitched = np.full((rows, 200), -3.0, f32)
        pitched[:, :cols] = z
        st = L.lib().dcmt_sparse_occlusion(ctx._h, pitched.ctypes.data, 800, pitched.ctypes.data, 800, rows, cols, ctypes.byref(p), ctypes.byref(cnt) if cnt else None)
        assert st == L.OK and (cnt is None or cnt.value == n)
        differ(np.ascontiguousarray(pitched[:, :cols]), o, "host, in place, pitched")
        assert (pitched[:, cols:] == -3.0).all()


# ------------------------------------------------------------------------------------------------------------- stream order, the chain
def stream_case(in_place, rows=40, cols=133, b=3):
    def inputs(which):
        return {"sparse": np.stack([R.sparse_plane(rows, cols, 0.3, 700 + 10 * which + f, specials=False) for f in range(b)])}      # (no NaN: SO compares values)

    def call(ctx, t, st):
        ctx.sparse_occlusion_dev(t["sparse"], t["sparse"] if in_place else t["out"], d_removed=t["removed"], stream=st)

    def wrap(ctx, t, st):
        out, removed = ctx.sparse_occlusion_dev(t["sparse"], None, removed=True, stream=st)
        return {"out": out, "removed": removed}

    def expect(inp):
        w = [want(inp["sparse"][f]) for f in range(b)]
        return {"sparse" if in_place else "out": np.stack([x[0] for x in w]), "removed": np.array([x[1] for x in w], np.int32)}

    outs = {"sparse" if in_place else "out": SO.Out((b, rows, cols), f32), "removed": SO.Out((b,), np.int32)}
    return SO.Case("sparse_occlusion in place" if in_place else "sparse_occlusion", (rows, cols, b), inputs, outs, call, expect, None, None if in_place else wrap)


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
def test_chain_projection_occlusion_completion_on_one_stream():
    """project_points_dev(nearest=True) -> sparse_occlusion_dev (in place) -> complete_dev on one non-default stream with no host
    synchronisation in between, against the same chain on the CPU: the nearest-wins restatement, the occlusion restatement, the oracle's
    completion."""
    import torch
    rows, cols = 24, 40
    inp = NR.project_inputs(rows, cols)
    pts, offsets, (T, P) = inp["points"], inp["offsets"], inp["records"][0]
    b = len(offsets) - 1
    params = api.make_params(spec_fill_iters=SO.SPEC)
    s = torch.cuda.Stream()
    with api.Context(0, rows, cols, b) as c:
        d_pts, d_off = dev(pts), dev(offsets)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            sparse = c.project_points_dev(d_pts, d_off, T, P, rows, cols, stream=s.cuda_stream, nearest=True)
            kept = sparse.clone()
            filtered, removed = c.sparse_occlusion_dev(sparse, sparse, removed=True, stream=s.cuda_stream, rx=1, ry=1, inv_depth_tol=0.05)
            dense = c.complete_dev(filtered, None, params, stream=s.cuda_stream)
        s.synchronize()
        got = {"projected": host(kept), "filtered": host(filtered), "removed": host(removed), "dense": host(dense)}
    projected = NR.project_batch(pts, offsets, T, P, rows, cols)
    for f in range(b):
        differ(got["projected"][f], projected[f], f"frame {f}: projected")
        o, n = want(projected[f], rx=1, ry=1, tol_code=3277)
        differ(got["filtered"][f], o, f"frame {f}: filtered")
        assert got["removed"][f] == n
        y, info = SO.O().img_completion(o, return_info=True)
        assert info["rc"] == 0 and info["fill_iters"] < SO.SPEC
        differ(got["dense"][f], y, f"frame {f}: dense")
    assert got["removed"].sum() > 0
    print(f"[occlusion] chain {rows}x{cols}: removed {got['removed'].tolist()} of {[int((projected[f] > 0).sum()) for f in range(b)]} returns")


# ------------------------------------------------------------------------------------------------------------- refusals
@gpu
def test_refusals(ctx):
    import torch
    lib = L.lib()
    r, c, b = 8, 16, 3
    n = r * c * b
    buf = torch.full((16 * n,), 0x5A, dtype=torch.uint8, device="cuda")
    z = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    rem = torch.full((b,), 0x25, dtype=torch.int32, device="cuda")
    good = api.make_occlusion_params()
    P = lambda t, off=0: t.data_ptr() + off

    def call(zz=P(z), oo=P(out), rr=P(rem), rows=r, cols=c, batch=b, h=ctx._h, p=good):
        return lib.dcmt_sparse_occlusion_dev(h, zz, oo, rows, cols, batch, None if p is None else ctypes.byref(p), rr, None)

    def call16(zz=P(buf), oo=P(buf, 4 * n), rr=P(rem), scale=1.0 / 256.0, p=good):
        return lib.dcmt_sparse_occlusion_u16_dev(ctx._h, zz, scale, oo, r, c, b, ctypes.byref(p), rr, None)

    def params(**kw):
        p = api.make_occlusion_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    bad = [call(zz=None), call(oo=None), call(p=None), call(h=None),
           call(zz=P(z, 2)), call(oo=P(out, 2)), call(rr=P(rem, 2)), call16(zz=P(buf, 1)), call16(oo=P(buf, 4 * n + 1)), call16(rr=P(rem, 2)),
           call(rows=MAX_ROWS + 1), call(cols=MAX_COLS + 1), call(batch=MAX_BATCH + 1), call(rows=0), call(cols=0), call(batch=0),
           call(zz=P(buf), oo=P(buf, 4)), call(zz=P(buf), oo=P(buf, 4 * n - 4)), call(zz=P(buf, 64), oo=P(buf)),
           call16(zz=P(buf), oo=P(buf, 2)), call16(zz=P(buf), oo=P(buf, 2 * n - 2)),
           call(rr=P(z)), call(rr=P(out, 4 * n - 4)), call(zz=P(buf), oo=P(buf), rr=P(buf, 8)), call16(rr=P(buf, 4 * n + 8)),
           call(p=params(rx=-1)), call(p=params(rx=9)), call(p=params(ry=-1)), call(p=params(ry=17)), call(p=params(tol_code=-1)), call(p=params(tol_code=(1 << 20) + 1)),
           call(p=params(valid_thresh=0.06)), call(p=params(valid_thresh=float("nan"))), call(p=params(valid_thresh=float("inf"))), call(p=params(valid_thresh=-1.0)),
           call(p=params(max_depth=0.05)), call(p=params(max_depth=16385.0)), call(p=params(max_depth=float("inf"))), call(p=params(max_depth=float("nan"))),
           call16(scale=0.0), call16(scale=-1.0), call16(scale=float("nan")), call16(scale=float("inf")), call16(p=params(rx=9))]
    assert bad == [L.E_INVALID] * len(bad), bad
    torch.cuda.synchronize()
    assert (host(out) == -7.0).all() and (host(rem) == 0x25).all() and (host(buf) == 0x5A).all() and (host(z) == 7.0).all()      # nothing written
    # what is allowed: touching buffers, in place, no counts, the extreme parameters
    assert call(rr=None) == L.OK and call(oo=P(z), rr=None) == L.OK and call(zz=P(buf), oo=P(buf, 4 * n), rr=P(buf, 8 * n)) == L.OK
    assert call(p=params(rx=0, ry=0, tol_code=0, valid_thresh=0.0625, max_depth=16384.0)) == L.OK and call(p=params(rx=8, ry=16, tol_code=1 << 20)) == L.OK
    assert call16(zz=P(buf, 2), oo=P(buf, 4 * n + 2)) == L.OK and call16(zz=P(buf), oo=P(buf), scale=1e-3) == L.OK
    torch.cuda.synchronize()
    assert (host(out) == 7.0).all() and (host(z) == 7.0).all() and (host(rem) == 0).all()
    # the host form
    hz, ho = np.full((r, c), 7.0, f32), np.full((r, c), -7.0, f32)
    one = lambda *a: lib.dcmt_sparse_occlusion(ctx._h, *a)
    gp = ctypes.byref(good)
    assert one(hz.ctypes.data, c * 4, ho.ctypes.data, c * 4, r, c, gp, None) == L.OK and (ho == 7.0).all()
    ho[:] = -7.0
    bad = [one(None, c * 4, ho.ctypes.data, c * 4, r, c, gp, None), one(hz.ctypes.data, c * 4, None, c * 4, r, c, gp, None),
           one(hz.ctypes.data, c * 4, ho.ctypes.data, c * 4, r, c, None, None), one(hz.ctypes.data, c * 4 - 4, ho.ctypes.data, c * 4, r, c, gp, None),
           one(hz.ctypes.data, c * 4, ho.ctypes.data, c * 4 - 4, r, c, gp, None), one(hz.ctypes.data, c * 4, ho.ctypes.data, c * 4, MAX_ROWS + 1, c, gp, None),
           one(hz.ctypes.data, c * 4, ho.ctypes.data, c * 4, r, c, ctypes.byref(params(ry=17)), None)]
    assert bad == [L.E_INVALID] * len(bad) and (ho == -7.0).all(), bad
    with pytest.raises(ValueError):
        ctx.sparse_occlusion_dev(dev(np.zeros((1, r, c), f32)), rx=9)
    with pytest.raises(api.DcmtError) as e:
        ctx.sparse_occlusion_dev(dev(np.zeros((1, r, c), u16)), u16=True, scale=0.0)
    assert e.value.status == L.E_INVALID
