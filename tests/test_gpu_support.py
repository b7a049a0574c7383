"""The distance to the nearest LiDAR return and the trust mask on the device: dcmt_support_distance_dev, its payload form, its host
form and the module-level calls, bit for bit against the restatements of tests/support_restatement.py (test_support.py holds the two
against each other).  Every frame of at most 10000 pixels is compared with BOTH restatements, the larger ones with scipy's transform.

Shapes.  k_support_cols takes strips of 64 columns in chunks of 8 rows, k_support_rows segments of 256 columns with a halo of R
columns, bands of 4 rows, 4 bands to a workgroup: 1 x 1, 1 x 65 (a second strip of one column), 17 x 1 (a second group of one band
of one row), 5 x 3 (smaller than any window), 33 x 130 and 65 x 129 (partial strips, chunks, bands and groups), 3 x 600 at R = 255 (both halos clip, three column tiles seam), 300 x 70 at R = 255 (the column cap, a sweep
longer than R), 4097 x 3 (past the rows whose ballots LDS holds: the route that reads the plane twice) beside 4096 x 3."""
import ctypes

import numpy as np
import pytest

import support_restatement as R
import test_gpu_stream_order as SO
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

gpu = pytest.mark.gpu
f32, u16, u32, i16 = np.float32, np.uint16, np.uint32, np.int16
MAX_ROWS, MAX_COLS, MAX_BATCH = 352, 1216, 5
LITERAL_PIXELS = 10000
RADII = [1, 9, 64, 255]
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
    """The restatement of one frame, computed once per input and shared (never modified): (dist2, beyond)."""
    key = (plane.shape, plane.dtype.str, plane.tobytes(), tuple(sorted(kw.items())))
    if key not in _want:
        d2, n = R.edt_dist2(plane, **kw)
        if plane.size <= LITERAL_PIXELS:
            lit = R.literal_dist2(plane, **kw)
            assert lit[0].tobytes() == d2.tobytes() and lit[1] == n
        d2.setflags(write=False)
        _want[key] = (d2, n)
    return _want[key]


def differ(got, wanted, what):
    assert got.shape == wanted.shape and got.dtype == wanted.dtype, (what, got.shape, got.dtype, wanted.shape, wanted.dtype)
    w = {2: u16, 4: u32}[got.dtype.itemsize]
    neq = np.ascontiguousarray(got).view(w) != np.ascontiguousarray(wanted).view(w)
    assert not neq.any(), f"{what}: {int(neq.sum())} elements differ, first at {tuple(np.argwhere(neq)[0])}: {got[tuple(np.argwhere(neq)[0])]} vs {wanted[tuple(np.argwhere(neq)[0])]}"


_dense = {}


def dense_for(shape):
    if shape not in _dense:
        b, rows, cols = shape
        pairs = [R.dense_planes(rows, cols, 900 + f) for f in range(b)]
        _dense[shape] = tuple(np.stack([p[k] for p in pairs]) for k in range(2))
        for a in _dense[shape]:
            a.setflags(write=False)
    return _dense[shape]


def check(ctx, planes, what, **kw):
    """The batch `planes` (f32 or the payload) through every combination of outputs against the restatement of every frame: dist2
    alone; out alone; both; with and without a fallback; with and without d_beyond; in place, whose bytes are the out-of-place call's.
    Returns (dist2, beyond)."""
    import torch
    planes = np.ascontiguousarray(planes)
    b = len(planes)
    payload = planes.dtype == u16
    skw = dict(kw, u16=payload)
    pkw = {k: v for k, v in kw.items() if k != "scale" or payload}
    dense, fallback = dense_for(planes.shape)
    w = [want(planes[f], **pkw) for f in range(b)]
    d2w, nw = np.stack([x[0] for x in w]), [x[1] for x in w]
    out_zero = np.stack([R.select(d2w[f], dense[f]) for f in range(b)])
    out_fb = np.stack([R.select(d2w[f], dense[f], fallback[f]) for f in range(b)])
    d_sparse, d_dense, d_fb = dev(planes), dev(dense), dev(fallback)
    junk16 = lambda: torch.full(planes.shape, 0x2525, dtype=torch.int16, device="cuda")
    junk32 = lambda: torch.full(planes.shape, -7.0, dtype=torch.float32, device="cuda")
    junkb = lambda: torch.full((b,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")

    def same(got, wanted, label):
        got = host(got)
        for f in range(b):
            differ(got[f], wanted[f], f"{what} frame {f}: {label}")

    # dist2 alone, without and with the count
    same(ctx.support_distance_dev(d_sparse, d_dist2=junk16(), **skw), d2w, "dist2 alone")
    d2, bey = ctx.support_distance_dev(d_sparse, d_dist2=junk16(), d_beyond=junkb(), **skw)
    same(d2, d2w, "dist2 with beyond")
    assert host(bey).tolist() == nw, f"{what}: beyond {host(bey).tolist()} against {nw}"
    # out alone, no fallback, without and with the count
    same(ctx.support_distance_dev(d_sparse, d_dense, d_out=junk32(), **skw), out_zero, "out alone")
    out, bey = ctx.support_distance_dev(d_sparse, d_dense, d_out=junk32(), d_beyond=junkb(), **skw)
    same(out, out_zero, "out with beyond")
    assert host(bey).tolist() == nw
    # out with a fallback; both outputs, without and with a fallback and the count
    same(ctx.support_distance_dev(d_sparse, d_dense, d_fb, d_out=junk32(), **skw), out_fb, "out with a fallback")
    out, d2 = ctx.support_distance_dev(d_sparse, d_dense, d_out=junk32(), d_dist2=junk16(), **skw)
    same(out, out_zero, "both: out")
    same(d2, d2w, "both: dist2")
    out, d2, bey = ctx.support_distance_dev(d_sparse, d_dense, d_fb, d_out=junk32(), d_dist2=junk16(), d_beyond=junkb(), **skw)
    same(out, out_fb, "all: out")
    same(d2, d2w, "all: dist2")
    assert host(bey).tolist() == nw
    assert host(d_dense).tobytes() == dense.tobytes() and host(d_fb).tobytes() == fallback.tobytes() and host(d_sparse).tobytes() == planes.tobytes()
    # in place: the bytes of the out-of-place call
    for fb, wanted in ((None, out_zero), (d_fb, out_fb)):
        d_in = dev(dense)
        got, d2, bey = ctx.support_distance_dev(d_sparse, d_in, fb, d_out=d_in, d_dist2=junk16(), d_beyond=junkb(), **skw)
        assert got.data_ptr() == d_in.data_ptr()
        same(d_in, wanted, "in place")
        same(d2, d2w, "in place: dist2")
        assert host(bey).tolist() == nw and host(d_in).tobytes() == wanted.tobytes()
        d_in = dev(dense)
        ctx.support_distance_dev(d_sparse, d_in, fb, d_out=d_in, **skw)
        assert host(d_in).tobytes() == wanted.tobytes()
    return d2w, nw


# ------------------------------------------------------------------------------------------------------------- against the restatements
@gpu
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_shapes(ctx, rows, cols):
    z = np.stack([R.sparse_plane(rows, cols, d, 10 + i) for i, d in enumerate((0.01, 0.2))] + [synth.synth_frame(rows, cols, 3), np.full((rows, cols), 5.0, f32)])
    v = np.stack([R.payload_plane(rows, cols, d, 10 + i) for i, d in enumerate((0.01, 0.2))])
    for radius in RADII:
        kw = {} if radius == 9 else dict(max_radius=radius)
        check(ctx, z, f"{rows}x{cols} {kw}", **kw)
        check(ctx, v, f"{rows}x{cols} payload {kw}", **kw)
    check(ctx, v, f"{rows}x{cols} payload, another scale", scale=0.01, max_radius=64)
    check(ctx, z, f"{rows}x{cols} other bounds", valid_thresh=0.5, max_depth=20.0, max_radius=64)


@gpu
def test_clipped_halos_and_seams_at_the_largest_radius(ctx):
    """3 x 600 at R = 255: a halo of 255 columns clips at both ends of the row and the three column tiles seam at 256 and 512; returns
    at the ends, beside the seams and none between: distances up to 255 along the row."""
    z = np.zeros((4, 3, 600), f32)
    z[0, 1, 0], z[0, 1, 599] = 5.0, 6.0
    z[1, 0, 255], z[1, 2, 512] = 5.0, 6.0
    z[2, 2, 300] = 7.0
    z[3, 0, 0], z[3, 0, 256], z[3, 2, 511] = 5.0, 6.0, 7.0
    for radius in (254, 64):
        check(ctx, z, f"3x600 R {radius}", max_radius=radius)
    d2, n = check(ctx, z, "3x600 R 255", max_radius=255)
    assert d2[2, 2, 45] == 65025 and d2[2, 2, 44] == R.BEYOND and d2[2, 2, 555] == 65025 and d2[2, 2, 556] == R.BEYOND
    assert d2[0, 1, 255] == 65025 and d2[0, 1, 256] == R.BEYOND and d2[0, 1, 344] == 65025 and d2[0, 0, 255] == R.BEYOND
    check(ctx, np.where(z > 0, 1280, 0).astype(u16), "3x600 payload", max_radius=255)


@gpu
def test_the_column_cap_and_a_sweep_longer_than_the_radius(ctx):
    """300 x 70 at R = 255: columns whose nearest return is more than R rows away (the cap, and 255 against 256), a down sweep and an
    up sweep that both run past R without a return; 70 columns are two strips."""
    z = np.zeros((3, 300, 70), f32)
    z[0, 0, 0] = 5.0
    z[1, 299, 69] = 5.0
    z[2, 150, 63], z[2, 0, 64] = 5.0, 6.0
    d2, n = check(ctx, z, "300x70 R 255", max_radius=255)
    assert d2[0, 255, 0] == 65025 and d2[0, 256, 0] == R.BEYOND and d2[0, 255, 1] == R.BEYOND and d2[0, 254, 1] == 254 * 254 + 1
    assert d2[1, 44, 69] == 65025 and d2[1, 43, 69] == R.BEYOND and d2[1, 299, 0] == 69 * 69
    check(ctx, z, "300x70 R 254", max_radius=254)
    check(ctx, z, "300x70 R 9")
    lone = np.zeros((1, 300, 3), f32)                             # the issue's lone return
    lone[0, 0, 0] = 5.0
    d2, n = check(ctx, lone, "300x3 R 255", max_radius=255)
    assert d2[0, 255, 0] == 65025 and d2[0, 256, 0] == R.BEYOND


@gpu
def test_frames_taller_than_the_ballots_lds_holds():
    """4096 rows keep their ballots in LDS, 4097 rows read the sparse plane twice: the same bytes, against the restatement."""
    for rows in (4096, 4097):
        with api.Context(0, rows, 3, 2) as c:
            z = np.zeros((2, rows, 3), f32)
            g = np.random.Generator(np.random.PCG64(rows))
            z[0][g.random((rows, 3)) < 0.004] = 5.0
            z[0, :300], z[0, rows - 1, 2] = 0.0, 7.0
            z[1, 2000, 1] = 5.0
            for radius in (9, 255):
                check(c, z, f"{rows}x3 R {radius}", max_radius=radius)
            check(c, np.where(z > 0, 1280, 0).astype(u16), f"{rows}x3 payload", max_radius=255)


@gpu
def test_one_kitti_frame(ctx):
    z = synth.synth_frame(352, 1216, 0)
    d2, n = check(ctx, np.stack([z, R.sparse_plane(352, 1216, 0.002, 3)]), "352x1216")
    assert n[0] == 138604 and (d2[0][:102] == R.BEYOND).all()     # what test_support.py records of this frame
    check(ctx, z[None], "352x1216 R 32", max_radius=32)
    check(ctx, R.sparse_plane(352, 1216, 0.0005, 4)[None], "352x1216 R 255", max_radius=255)
    check(ctx, R.payload_plane(352, 1216, 0.002, 4)[None], "352x1216 payload")


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
    """Frame f of a batch equals the frame alone, whatever the scratch planes held; the middle frame holds no returns: all of it is
    beyond, and d_beyond of the others is not disturbed by it."""
    import torch
    rows, cols = 33, 130
    z = np.stack([R.sparse_plane(rows, cols, 0.01 + 0.02 * f, 40 + f) for f in range(b)])
    if b > 1:
        z[b // 2] = 0
    for planes in (z, np.stack([R.payload_plane(rows, cols, 0.02, 50 + f) for f in range(b)])):
        payload = planes.dtype == u16
        dirty(ctx, how)
        d2, n = check(ctx, planes, f"batch of {b}")
        dirty(ctx, how)
        got, bey = ctx.support_distance_dev(dev(planes), d_beyond=torch.full((b,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), u16=payload)
        assert host(bey).tolist() == n and host(got).tobytes() == d2.tobytes()
        if b > 1 and not payload:
            assert n[b // 2] == rows * cols and 0 < n[0] < rows * cols
        for f in {0, b - 1}:
            dirty(ctx, how)
            d1, n1 = check(ctx, planes[f][None], f"frame {f} alone")
            differ(d1[0], d2[f], f"frame {f} alone against its place in the batch")
            assert n1[0] == n[f]


@gpu
def test_nothing_crosses_a_frame_or_wraps_a_row(ctx):
    """Returns on the last row and the last column of frame f and on the first of frame f + 1 reach neither the other frame nor, along
    a row, the other end of the next row."""
    rows, cols = 33, 130
    z = np.zeros((3, rows, cols), f32)
    z[0, rows - 1, :] = 2.0                                       # the whole last row of frame 0
    z[1, 0, 7] = 5.0                                              # one return on the first row of frame 1
    z[1, rows - 1, cols - 1] = 5.0                                # the last pixel of frame 1
    z[2, 0, 0] = 5.0                                              # the first pixel of frame 2
    z[2, 10, cols - 1] = 5.0                                      # the end of row 10: row 11 starts 1 element later
    for radius in (1, 9, 64, 255):
        d2, n = check(ctx, z, f"frame boundaries R {radius}", max_radius=radius)
        assert d2[1, 0, 60] == (53 * 53 if radius >= 53 else R.BEYOND)           # not the row of returns one row "above" it in memory
        assert d2[0, 0, 7] == (32 * 32 if radius >= 32 else R.BEYOND)            # not frame 1's return one row "below" frame 0's last
        assert d2[2, 11, 0] == (11 * 11 if radius >= 11 else R.BEYOND)           # not the end of row 10, one element back
        assert d2[1, rows - 1, cols - 2] == 1 and d2[2, 0, 1] == 1
    v = np.where(z > 0, 1280, 0).astype(u16)
    check(ctx, v, "frame boundaries, payload", max_radius=255)


# ------------------------------------------------------------------------------------------------------------- alignment, forms
@gpu
def test_pointers_offset_by_one_element(ctx):
    import torch
    rows, cols, b = 33, 130, 3
    n = b * rows * cols
    dense, fallback = dense_for((b, rows, cols))
    for planes, tdt in ((np.stack([R.sparse_plane(rows, cols, 0.02, 60 + f) for f in range(b)]), torch.float32),
                        (np.stack([R.payload_plane(rows, cols, 0.02, 60 + f) for f in range(b)]), torch.int16)):
        payload = planes.dtype == u16
        w = [want(planes[f]) for f in range(b)]
        d2w = np.stack([x[0] for x in w])
        outw = np.stack([R.select(d2w[f], dense[f], fallback[f]) for f in range(b)])
        for offs in ((1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 1, 1, 1, 1), (3, 2, 1, 3, 5)):
            bufs = [torch.full((n + 8,), 0x25, dtype=dt, device="cuda") for dt in (tdt, torch.float32, torch.float32, torch.float32, torch.int16)]
            vs, vd, vf, vo, vq = (t[o:o + n].view(b, rows, cols) for t, o in zip(bufs, offs))
            vs.copy_(dev(planes)); vd.copy_(dev(dense)); vf.copy_(dev(fallback))
            assert vq.data_ptr() % 16 == (bufs[4].data_ptr() + 2 * offs[4]) % 16
            out, d2, bey = ctx.support_distance_dev(vs, vd, vf, d_out=vo, d_dist2=vq, beyond=True, u16=payload)
            for f in range(b):
                differ(host(vo)[f], outw[f], f"offsets {offs} frame {f}: out")
                differ(host(vq)[f], d2w[f], f"offsets {offs} frame {f}: dist2")
            assert host(bey).tolist() == [x[1] for x in w]
            for t, o in ((bufs[3], offs[3]), (bufs[4], offs[4])):         # nothing outside the outputs
                h = t.cpu().numpy()
                assert (h[:o] == h.dtype.type(0x25)).all() and (h[o + n:] == h.dtype.type(0x25)).all()
            ctx.support_distance_dev(vs, vd, vf, d_out=vd, u16=payload)                                          # in place at that offset
            assert host(vd).tobytes() == outw.tobytes()
            h = bufs[1].cpu().numpy()
            assert (h[:offs[1]] == f32(0x25)).all() and (h[offs[1] + n:] == f32(0x25)).all()


@gpu
def test_payload_form_equals_the_f32_form_on_the_ingested_depths(ctx):
    v = np.stack([R.payload_plane(65, 129, 0.02, 70 + f) for f in range(2)])
    dense, fallback = dense_for(v.shape)
    for kw in ({}, dict(scale=0.01, max_radius=20, valid_thresh=0.3, max_depth=50.0)):
        pkw = {k: x for k, x in kw.items() if k != "scale"}
        z = (v.astype(f32) * f32(kw.get("scale", 1.0 / 256.0))).astype(f32)
        a = ctx.support_distance_dev(dev(v), dev(dense), dev(fallback), dist2=True, beyond=True, u16=True, **kw)
        c = ctx.support_distance_dev(dev(z), dev(dense), dev(fallback), dist2=True, beyond=True, **pkw)
        for x, y in zip(a, c):
            assert host(x).tobytes() == host(y).tobytes()
        assert 0 < host(a[2]).sum() < v.size


@gpu
def test_host_entry_point_and_module_level_calls(ctx):
    rows, cols = 33, 130
    z = R.sparse_plane(rows, cols, 0.02, 80)
    dense, fallback = (a[0] for a in dense_for((1, rows, cols)))
    d2w, nw = want(z)
    d2, n = ctx.support_distance(z)
    differ(d2, d2w, "host dist2")
    assert n == nw and 0 < n < z.size
    out, d2, n = ctx.support_distance(z, dense, fallback)
    differ(out, R.select(d2w, dense, fallback), "host out with a fallback")
    differ(d2, d2w, "host dist2 beside out")
    assert n == nw
    out, d2, n = ctx.support_distance(z, dense, max_radius=3)
    differ(out, R.select(want(z, max_radius=3)[0], dense), "host out, R 3")
    wide = np.full((rows, 150), 3.0, f32)
    wide[:, :cols] = z
    differ(ctx.support_distance(wide[:, :cols])[0], d2w, "pitched input")
    differ(api.distance_to_returns(z), d2w, "distance_to_returns")
    differ(api.distance_to_returns(z, max_radius=64), want(z, max_radius=64)[0], "distance_to_returns, R 64")
    differ(api.trust_mask(z, dense), R.select(d2w, dense), "trust_mask")
    differ(api.trust_mask(z, dense, fallback, max_radius=2), R.select(want(z, max_radius=2)[0], dense, fallback), "trust_mask with a fallback")
    # the C entry point itself: in place on a pitched plane, a pitched dist2, with and without the count
    p = api.make_support_params()
    for cnt in (ctypes.c_uint32(77), None):
        pitched = np.full((rows, 200), -3.0, f32)
        pitched[:, :cols] = dense
        q = np.full((rows, 140), 0x2525, u16)
        st = L.lib().dcmt_support_distance(ctx._h, z.ctypes.data, cols * 4, pitched.ctypes.data, 800, fallback.ctypes.data, cols * 4, pitched.ctypes.data, 800,
                                           q.ctypes.data, 280, rows, cols, ctypes.byref(p), ctypes.byref(cnt) if cnt else None)
        assert st == L.OK and (cnt is None or cnt.value == nw)
        differ(np.ascontiguousarray(pitched[:, :cols]), R.select(d2w, dense, fallback), "host, in place, pitched")
        differ(np.ascontiguousarray(q[:, :cols]), d2w, "host, pitched dist2")
        assert (pitched[:, cols:] == -3.0).all() and (q[:, cols:] == 0x2525).all()


# ------------------------------------------------------------------------------------------------------------- stream order, the chain
def stream_case(in_place, rows=40, cols=133, b=3):
    def inputs(which):
        g = np.random.Generator(np.random.PCG64(800 + which))
        return {"sparse": np.stack([R.sparse_plane(rows, cols, 0.01, 700 + 10 * which + f, specials=False) for f in range(b)]),
                "dense": g.uniform(1.0, 90.0, (b, rows, cols)).astype(f32),                     # (no NaN: SO compares values)
                "fallback": g.uniform(1.0, 90.0, (b, rows, cols)).astype(f32)}

    def call(ctx, t, st):
        ctx.support_distance_dev(t["sparse"], t["dense"], t["fallback"], d_out=t["dense"] if in_place else t["out"], d_dist2=t["dist2"], d_beyond=t["beyond"],
                                 stream=st)

    def wrap(ctx, t, st):
        import torch
        out, d2, bey = ctx.support_distance_dev(t["sparse"], t["dense"], t["fallback"], dist2=True, beyond=True, stream=st)
        return {"out": out, "dist2": d2.view(torch.int16), "beyond": bey}

    def expect(inp):
        w = [want(inp["sparse"][f]) for f in range(b)]
        return {"dense" if in_place else "out": np.stack([R.select(w[f][0], inp["dense"][f], inp["fallback"][f]) for f in range(b)]),
                "dist2": np.stack([x[0] for x in w]).view(i16), "beyond": np.array([x[1] for x in w], np.int32)}

    outs = {"dense" if in_place else "out": SO.Out((b, rows, cols), f32), "dist2": SO.Out((b, rows, cols), i16), "beyond": SO.Out((b,), np.int32)}
    return SO.Case("support_distance in place" if in_place else "support_distance", (rows, cols, b), inputs, outs, call, expect, None, None if in_place else wrap)


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
def test_chain_completion_trust_mask_evaluation_on_one_stream():
    """complete_dev -> support_distance_dev(d_fallback = another plane, in place) -> evaluate_dev on one non-default stream with no host
    synchronisation in between, against the numpy composition: the oracle's completion, the restatement's distances, the select on the
    bits; the sums of the evaluation are those of the evaluation made alone on that composed plane, and their counts numpy's."""
    import torch
    rows, cols, b = 48, 64, 3
    sparse = SO.sparse_frames(b, rows, cols, 31, gap=True)
    g = np.random.Generator(np.random.PCG64(32))
    other = g.uniform(1.0, 80.0, (b, rows, cols)).astype(f32)
    gt = np.where(g.random((b, rows, cols)) < 0.3, g.uniform(1.0, 80.0, (b, rows, cols)), 0.0).astype(f32)
    params = api.make_params(spec_fill_iters=SO.SPEC)
    s = torch.cuda.Stream()
    with api.Context(0, rows, cols, b) as c:
        d_sparse, d_other, d_gt = dev(sparse), dev(other), dev(gt)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            dense = c.complete_dev(d_sparse, None, params, stream=s.cuda_stream)
            kept = dense.clone()
            trusted, bey = c.support_distance_dev(d_sparse, dense, d_other, d_out=dense, beyond=True, stream=s.cuda_stream, max_radius=3)
            sums = c.evaluate_dev(d_gt, trusted, stream=s.cuda_stream)
        s.synchronize()
        got = {"dense": host(kept), "trusted": host(trusted), "beyond": host(bey), "sums": host(sums)}
        composed = np.empty_like(sparse)
        for f in range(b):
            y, info = SO.O().img_completion(sparse[f], return_info=True)
            assert info["rc"] == 0 and info["fill_iters"] < SO.SPEC
            differ(got["dense"][f], y, f"frame {f}: dense")
            d2, n = want(sparse[f], max_radius=3)
            composed[f] = R.select(d2, y, other[f])
            differ(got["trusted"][f], composed[f], f"frame {f}: trusted")
            assert got["beyond"][f] == n and 0 < n < rows * cols
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
    dense = torch.full((n,), 3.0, dtype=torch.float32, device="cuda")
    fb = torch.full((n,), 4.0, dtype=torch.float32, device="cuda")
    out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    d2 = torch.full((n,), 0x2525, dtype=torch.int16, device="cuda")
    bey = torch.full((b,), 0x25, dtype=torch.int32, device="cuda")
    good = api.make_support_params()
    P = lambda t, off=0: t.data_ptr() + off

    def call(zz=P(z), dd=P(dense), ff=P(fb), oo=P(out), qq=P(d2), bb=P(bey), rows=r, cols=c, batch=b, h=ctx._h, p=good):
        return lib.dcmt_support_distance_dev(h, zz, dd, ff, oo, qq, rows, cols, batch, None if p is None else ctypes.byref(p), bb, None)

    def call16(zz=P(buf), dd=P(dense), ff=P(fb), oo=P(out), qq=P(d2), bb=P(bey), scale=1.0 / 256.0, p=good):
        return lib.dcmt_support_distance_u16_dev(ctx._h, zz, scale, dd, ff, oo, qq, r, c, b, ctypes.byref(p), bb, None)

    def params(**kw):
        p = api.make_support_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    bad = [call(zz=None), call(p=None), call(h=None), call(oo=None, qq=None, ff=None), call(dd=None), call(dd=None, ff=None), call(oo=None), call16(oo=None),
           call(zz=P(z, 2)), call(dd=P(dense, 2)), call(ff=P(fb, 2)), call(oo=P(out, 2)), call(qq=P(d2, 1)), call(bb=P(bey, 2)), call16(zz=P(buf, 1)), call16(qq=P(d2, 1)),
           call(rows=MAX_ROWS + 1), call(cols=MAX_COLS + 1), call(batch=MAX_BATCH + 1), call(rows=0), call(cols=0), call(batch=0),
           call(dd=P(buf), oo=P(buf, 4)), call(dd=P(buf), oo=P(buf, 4 * n - 4)), call(dd=P(buf, 64), oo=P(buf)),
           call(zz=P(dense)), call(zz=P(fb)), call(zz=P(out)), call(ff=P(dense)), call(ff=P(out)), call(ff=P(dense), oo=P(dense)), call(zz=P(dense), oo=P(dense)),
           call(qq=P(z)), call(qq=P(dense)), call(qq=P(fb, 2 * n)), call(qq=P(out, 4 * n - 2)), call(bb=P(z)), call(bb=P(dense, 8)), call(bb=P(fb)), call(bb=P(out, 4 * n - 4)),
           call(bb=P(d2, 2 * n - 4)), call16(zz=P(dense)), call16(zz=P(buf), qq=P(buf, 2 * n - 2)), call16(zz=P(buf), bb=P(buf, 2 * n - 4)),
           call(p=params(max_radius=0)), call(p=params(max_radius=-1)), call(p=params(max_radius=256)),
           call(p=params(valid_thresh=0.06)), call(p=params(valid_thresh=float("nan"))), call(p=params(valid_thresh=float("inf"))), call(p=params(valid_thresh=-1.0)),
           call(p=params(max_depth=0.05)), call(p=params(max_depth=16385.0)), call(p=params(max_depth=float("inf"))), call(p=params(max_depth=float("nan"))),
           call16(scale=0.0), call16(scale=-1.0), call16(scale=float("nan")), call16(scale=float("inf")), call16(p=params(max_radius=256))]
    assert bad == [L.E_INVALID] * len(bad), bad
    torch.cuda.synchronize()
    assert (host(out) == -7.0).all() and (host(bey) == 0x25).all() and (host(buf) == 0x5A).all() and (host(z) == 7.0).all()      # nothing written
    assert (host(dense) == 3.0).all() and (host(fb) == 4.0).all() and (d2.cpu().numpy() == 0x2525).all()
    # what is allowed: every output alone, in place, touching buffers, the extreme parameters, the payload at an odd element
    assert call() == L.OK and call(bb=None) == L.OK and call(qq=None, bb=None) == L.OK and call(oo=None, ff=None, dd=None) == L.OK and call(oo=None, ff=None) == L.OK
    assert call(ff=None) == L.OK and call(zz=P(buf), dd=P(buf, 4 * n), ff=P(buf, 8 * n), oo=P(buf, 12 * n), qq=P(buf, 16 * n), bb=P(buf, 18 * n)) == L.OK
    assert call(p=params(max_radius=1, valid_thresh=0.0625, max_depth=16384.0)) == L.OK and call(p=params(max_radius=255)) == L.OK
    assert call16(zz=P(buf, 2)) == L.OK and call16(scale=1e-3, oo=None, ff=None, dd=None) == L.OK
    torch.cuda.synchronize()
    assert (host(out) == 3.0).all() and (d2.cpu().numpy() == 0).all() and (host(bey) == 0).all() and (host(z) == 7.0).all()       # every pixel a return
    d_in = dense.clone()
    assert call(dd=P(d_in), oo=P(d_in)) == L.OK
    torch.cuda.synchronize()
    assert (host(d_in) == 3.0).all()
    # the host form
    hz, hd, ho, hq = np.full((r, c), 7.0, f32), np.full((r, c), 3.0, f32), np.full((r, c), -7.0, f32), np.full((r, c), 0x2525, u16)
    one = lambda *a: lib.dcmt_support_distance(ctx._h, *a)
    gp = ctypes.byref(good)
    Z, D, O, Q = hz.ctypes.data, hd.ctypes.data, ho.ctypes.data, hq.ctypes.data
    assert one(Z, c * 4, D, c * 4, None, 0, O, c * 4, Q, c * 2, r, c, gp, None) == L.OK and (ho == 3.0).all() and not hq.any()
    ho[:], hq[:] = -7.0, 0x2525
    bad = [one(None, c * 4, D, c * 4, None, 0, O, c * 4, Q, c * 2, r, c, gp, None), one(Z, c * 4, D, c * 4, None, 0, O, c * 4, Q, c * 2, r, c, None, None),
           one(Z, c * 4, D, c * 4, None, 0, None, 0, None, 0, r, c, gp, None), one(Z, c * 4, None, 0, None, 0, O, c * 4, Q, c * 2, r, c, gp, None),
           one(Z, c * 4, D, c * 4, D, c * 4, None, 0, Q, c * 2, r, c, gp, None), one(Z, c * 4 - 4, D, c * 4, None, 0, O, c * 4, Q, c * 2, r, c, gp, None),
           one(Z, c * 4, D, c * 4 - 4, None, 0, O, c * 4, Q, c * 2, r, c, gp, None), one(Z, c * 4, D, c * 4, None, 0, O, c * 4 - 4, Q, c * 2, r, c, gp, None),
           one(Z, c * 4, D, c * 4, None, 0, O, c * 4, Q, c * 2 - 2, r, c, gp, None), one(Z, c * 4, D, c * 4, None, 0, O, c * 4, Q, c * 2, MAX_ROWS + 1, c, gp, None),
           one(Z, c * 4, D, c * 4, None, 0, O, c * 4, Q, c * 2, r, c, ctypes.byref(params(max_radius=256)), None)]
    assert bad == [L.E_INVALID] * len(bad) and (ho == -7.0).all() and (hq == 0x2525).all(), bad
    with pytest.raises(ValueError):
        ctx.support_distance_dev(dev(np.zeros((1, r, c), f32)), max_radius=0)
    with pytest.raises(ValueError):
        ctx.support_distance_dev(dev(np.zeros((1, r, c), f32)), d_fallback=dev(np.zeros((1, r, c), f32)))
    with pytest.raises(api.DcmtError) as e:
        ctx.support_distance_dev(dev(np.zeros((1, r, c), u16)), u16=True, scale=0.0)
    assert e.value.status == L.E_INVALID
