"""get_initial_error on the device: dcmt_photo_error_dev / dcmt_photo_error_calib_dev / dcmt_photo_error and their Python surface, bit for
bit against tests/photo_error_restatement.py (its vectorised form, which tests/test_photo_error.py holds against the statement-by-
statement one without a GPU).

A case is one call on THREE frames, one per depth plane -- frame 0 random depths with 30 % zeros, frame 1 a constant plane, frame 2 the
adversarial plane -- so that every shape, window and image kind meets every plane, as a batch of 3 and, frame by frame, as batches
of 1.  Shapes: the smallest at which the kernels can go wrong (one pixel, one row, one column, fewer columns than a lane's four, no
multiple of four or sixteen, exactly and just beyond multiples of the tile, the reference's frame), the smallest that take bands of 8
and of 4 rows and a band cut down by the LDS budget, and the shape the plan sends down the fallback route
(tests/plan_photo_error_test.cpp pins the plan of each).  Up to 65 x 257 every window meets every image kind; on the larger shapes
the image kind rotates with the window, so that a case's reference stays a matter of seconds.  References are computed once per
(shape, window, image) and shared."""
import ctypes
import functools

import numpy as np
import pytest

import photo_error_restatement as R
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

gpu = pytest.mark.gpu
f32 = np.float32

SMALL = [(1, 1), (1, 9), (9, 1), (3, 5), (5, 7), (37, 131), (64, 256), (65, 257)]
FALLBACK = (3, 16400)
# (rows, cols, window): the reference's frame and the fallback shape at every window; bands of 8 rows (vec and not), of 4, an LDS-bound band
LARGE = [(352, 1216, w) for w in (1, 2, 3, 4)] + [FALLBACK + (w,) for w in (1, 2, 3, 4)] + \
        [(4096, 16, 1), (4100, 20, 3), (2100, 16, 2), (5, 3000, 4), (5, 3000, 2)]
CASES = [(r, c, w, img) for (r, c) in SMALL for w in (1, 2, 3, 4) for img in R.IMAGES] + \
        [(r, c, w, list(R.IMAGES)[(w + r) % 3]) for (r, c, w) in LARGE]


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                # (a copy: the shared frames are read-only)


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def frames(rows, cols, image):
    """The three frames of a shape: (depth [3][rows][cols], left, right).  The images differ from frame to frame (a roll)."""
    depth = np.stack([R.random_depth(rows, cols, 40 + rows), R.constant_depth(rows, cols, 9.5), R.adversarial_depth(rows, cols, 41 + cols)[0]])
    left, right = R.IMAGES[image](rows, cols)
    lefts = np.stack([np.roll(left, f, axis=1) for f in range(3)])
    rights = np.stack([np.roll(right, 2 * f, axis=0) for f in range(3)])
    for a in (depth, lefts, rights):
        a.setflags(write=False)
    return depth, lefts, rights


@functools.lru_cache(maxsize=None)
def reference(rows, cols, window, image, baseline=R.BASELINE, focal=R.FOCAL):
    """(err [3][rows][cols], stats int64 [3][4]) of frames(): computed once, shared, read-only."""
    depth, lefts, rights = frames(rows, cols, image)
    err, stats = R.batch(R.vectorised, depth, lefts, rights, window=window, baseline=baseline, focal=focal)
    stats = stats.astype(np.int64)
    err.setflags(write=False)
    stats.setflags(write=False)
    return err, stats


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    neq = got != want
    if neq.any():
        first = tuple(np.argwhere(neq)[0])
        raise AssertionError(f"{what}: {int(neq.sum())} of {want.size} differ; first at {first}: {got[first]!r} vs {want[first]!r}")


@gpu
@pytest.mark.parametrize("rows,cols,window,image", CASES)
def test_map_and_stats_are_the_restatement_bit_for_bit(rows, cols, window, image):
    import torch
    depth, lefts, rights = frames(rows, cols, image)
    want_err, want_stats = reference(rows, cols, window, image)
    d, l, r = dev(depth), dev(lefts), dev(rights)
    what = f"{rows}x{cols} window {window} {image}"
    with api.Context(0, rows, cols, 3) as ctx:
        err, stats = ctx.photo_error_dev(d, l, r, window=window)
        same(host(err), want_err, what + ": map")
        same(host(stats), want_stats, what + ": stats")
        # the same bits again, and with either output left out
        err2, stats2 = ctx.photo_error_dev(d, l, r, window=window)
        only_err = ctx.photo_error_dev(d, l, r, stats=False, window=window)
        only_stats = ctx.photo_error_dev(d, l, r, err=False, window=window)
        same(host(err2), want_err, what + ": map, second run")
        same(host(stats2), want_stats, what + ": stats, second run")
        same(host(only_err), want_err, what + ": map only")
        same(host(only_stats), want_stats, what + ": stats only")
        # batch independence: frame f of the batch equals f alone
        for f in range(3):
            e1, s1 = ctx.photo_error_dev(d[f:f + 1], l[f:f + 1], r[f:f + 1], window=window)
            same(host(e1)[0], want_err[f], what + f": frame {f} alone, map")
            same(host(s1)[0], want_stats[f], what + f": frame {f} alone, stats")
        # pointers that take no wide access (the inputs one byte / one float into their buffers): the same bits
        pad = lambda t: torch.cat([t.flatten()[:1], t.flatten()])[1:].view(t.shape)
        e3, s3 = ctx.photo_error_dev(pad(d), pad(l), pad(r), window=window)
        same(host(e3), want_err, what + ": unaligned inputs, map")
        same(host(s3), want_stats, what + ": unaligned inputs, stats")
        if cols < 37:
            # the reference's constants put few targets inside so narrow a frame: the same with disparities below a pixel
            kw = dict(baseline=0.5, focal=1.0)
            near_err, near_stats = reference(rows, cols, window, image, **kw)
            e4, s4 = ctx.photo_error_dev(d, l, r, window=window, **kw)
            same(host(e4), near_err, what + ": small disparities, map")
            same(host(s4), near_stats, what + ": small disparities, stats")
            assert cols < 3 or near_stats[1, 0] == rows * (cols - 2)          # the constant plane: every column from 2 on
    # what the planes are there for
    if image == "extremes":
        valid_with_taps = want_err > 0
        assert (want_err[valid_with_taps] == 255).all() and (want_stats[:, 3] == 255 * want_stats[:, 2]).all()
    if cols >= 37:
        assert want_stats[0, 0] > 0 and want_stats[1, 0] > 0 and want_stats[2, 0] > 0


@gpu
def test_the_adversarial_plane_holds_its_cases_on_the_device():
    """The pixels of the adversarial frame, one by one, at the reference's constants: t on -0.5, 0.5, beyond the left end, -inf and the
    odd values give 0; t on 1 and on cols - 1 are valid (all 0 against all 255: the byte is 255)."""
    rows, cols = 37, 131
    depth, placed = R.adversarial_depth(rows, cols, 41 + cols)
    assert set(placed) == set(R.T_TARGETS) | set(R.SPECIAL_VALUES)
    left, right = R.extremes_pair(rows, cols)
    with api.Context(0, rows, cols, 1) as ctx:
        err, stats = ctx.photo_error_dev(dev(depth[None]), dev(left[None]), dev(right[None]))
        err, stats = host(err)[0], host(stats)[0]
    want_err, want_stats = R.vectorised(depth, left, right)
    same(err, want_err, "adversarial: map")
    same(stats, want_stats.astype(np.int64), "adversarial: stats")
    for k in ("t=1", "t=cols-1"):
        assert err[placed[k]] == 255, (k, placed[k])
    for k in ("t=-0.5", "t=0.5", "t<left", "t=-inf", "1e-38", "1e-30", "-1", "-0.0", "nan", "-inf"):
        assert err[placed[k]] == 0, (k, placed[k])


@gpu
def test_calib_equals_the_uniform_call_frame_by_frame_and_a_bad_record_zeroes_its_frame():
    rows, cols, window, image = 37, 131, 2, "random"
    depth, lefts, rights = frames(rows, cols, image)
    d, l, r = dev(depth), dev(lefts), dev(rights)
    base, foc = [0.54, 0.25, 1.5], [959.791, 400.0, 96.0]
    table = api.make_stereo_calib(base, foc)
    with api.Context(0, rows, cols, 3) as ctx:
        err, stats = ctx.photo_error_calib_dev(d, l, r, api.calib_to_device(table), window=window)
        err, stats = host(err), host(stats)
        for f in range(3):
            e1, s1 = ctx.photo_error_dev(d[f:f + 1], l[f:f + 1], r[f:f + 1], window=window, baseline=base[f], focal=foc[f])
            same(err[f], host(e1)[0], f"record {f}: map")
            same(stats[f], host(s1)[0], f"record {f}: stats")
            we, ws = R.vectorised(depth[f], lefts[f], rights[f], baseline=base[f], focal=foc[f], window=window)
            same(err[f], we, f"record {f}: map against the restatement")
            same(stats[f], ws.astype(np.int64), f"record {f}: stats against the restatement")
            assert stats[f, 0] > 0
        # records the uniform call refuses, on the device: a zero plane and zero counts for that frame, the others as before
        for bad_frame, entries in ((0, (np.nan, 400.0)), (1, (0.54, -959.791)), (2, (0.0, 96.0)), (0, (np.inf, 959.791)), (1, (0.25, 0.0)),
                                   (2, (1.5, np.nan)), (1, (-0.0, 400.0)), (2, (-np.inf, -1.0))):
            bad = table.copy()
            bad["baseline"][bad_frame], bad["focal"][bad_frame] = entries
            e = dev(np.full((3, rows, cols), 0xA5, np.uint8))
            s = dev(np.full((3, 4), -7, np.int64))
            ctx.photo_error_calib_dev(d, l, r, api.calib_to_device(bad), d_err=e, d_stats=s, window=window)
            e, s = host(e), host(s)
            for f in range(3):
                if f == bad_frame:
                    assert (e[f] == 0).all() and (s[f] == 0).all(), (bad_frame, entries)
                else:
                    same(e[f], err[f], f"bad record {bad_frame} {entries}: frame {f} map")
                    same(s[f], stats[f], f"bad record {bad_frame} {entries}: frame {f} stats")
            only_stats = host(ctx.photo_error_calib_dev(d, l, r, api.calib_to_device(bad), err=False, window=window))
            same(only_stats, s, f"bad record {bad_frame} {entries}: stats only")
    # the fallback route takes the same records
    rows, cols = FALLBACK
    depth, lefts, rights = frames(rows, cols, "ramp")
    d, l, r = dev(depth), dev(lefts), dev(rights)
    bad = table.copy()
    bad["focal"][1] = np.nan
    with api.Context(0, rows, cols, 3) as ctx:
        e, s = ctx.photo_error_calib_dev(d, l, r, api.calib_to_device(bad), window=3)
        e, s = host(e), host(s)
        assert (e[1] == 0).all() and (s[1] == 0).all()
        for f in (0, 2):
            we, ws = R.vectorised(depth[f], lefts[f], rights[f], baseline=base[f], focal=foc[f], window=3)
            same(e[f], we, f"fallback, record {f}: map")
            same(s[f], ws.astype(np.int64), f"fallback, record {f}: stats")


@gpu
def test_host_forms_agree_with_the_device_entry():
    rows, cols, window = 65, 257, 2
    depth, lefts, rights = frames(rows, cols, "random")
    want_err, want_stats = reference(rows, cols, window, "random")
    with api.Context(0, rows, cols, 1) as ctx:
        e, s = ctx.photo_error(depth[0], lefts[0], rights[0], window=window)
        same(e, want_err[0], "host entry: map")
        assert s.dtype == np.uint64
        same(s.astype(np.int64), want_stats[0], "host entry: stats")
        same(ctx.photo_error(depth[0], lefts[0], rights[0], stats=False), want_err[0], "host entry: map only")
        same(ctx.photo_error(depth[0], lefts[0], rights[0], err=False).astype(np.int64), want_stats[0], "host entry: stats only")
        # rows further apart than they need to be
        wide_d, wide_l = np.zeros((rows, cols + 7), f32), np.full((rows, cols + 5), 9, np.uint8)
        wide_d[:, :cols], wide_l[:, :cols] = depth[2], lefts[2]
        e, s = ctx.photo_error(wide_d[:, :cols], wide_l[:, :cols], rights[2])
        same(e, want_err[2], "host entry, padded rows: map")
        same(s.astype(np.int64), want_stats[2], "host entry, padded rows: stats")
    e, stats = api.get_initial_error(depth[0], lefts[0], rights[0])
    same(e, want_err[0], "get_initial_error, grey: map")
    assert list(stats) == list(api.PHOTO_STATS) and [stats[k] for k in api.PHOTO_STATS] == [int(v) for v in want_stats[0]]
    # BGR inputs go through bgr_to_gray, as the reference's cvtColor calls do
    rng = np.random.default_rng(3)
    bgr_l, bgr_r = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8), rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    grey_l, grey_r = api.bgr_to_gray(bgr_l), api.bgr_to_gray(bgr_r)
    e, stats = api.get_initial_error(depth[0], bgr_l, bgr_r, window=3)
    we, ws = R.vectorised(depth[0], grey_l, grey_r, window=3)
    same(e, we, "get_initial_error, BGR: map")
    assert [stats[k] for k in api.PHOTO_STATS] == [int(v) for v in ws]
    e2, stats2 = api.get_initial_error(depth[0], grey_l, grey_r, window=3)
    same(e2, e, "get_initial_error, grey of the BGR: map")
    assert stats2 == stats


@gpu
def test_every_refusal_returns_invalid_and_writes_nothing():
    import torch
    rows, cols, b = 8, 16, 2
    px = b * rows * cols
    lib = L.lib()
    # one buffer, so that overlapping arguments can be named: depth | left | right | err | stats | table, each region 16-byte aligned
    off = {"depth": 0, "left": 4 * px, "right": 5 * px, "err": 6 * px, "stats": 7 * px, "table": 7 * px + 64, "end": 7 * px + 128}
    buf = torch.full((off["end"],), 0xA5, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    assert base % 16 == 0
    A = {k: base + v for k, v in off.items()}
    p = api.make_photo_error_params()
    with api.Context(0, rows, cols, b) as ctx:
        def call(calib=False, ctx_h=ctx._h, depth=A["depth"], left=A["left"], right=A["right"], r=rows, c=cols, n=b, params=p, table=A["table"],
                 err=A["err"], stats=A["stats"]):
            prm = ctypes.byref(params) if params is not None else None
            if calib:
                return lib.dcmt_photo_error_calib_dev(ctx_h, depth, left, right, r, c, n, prm, table, err, stats, None)
            return lib.dcmt_photo_error_dev(ctx_h, depth, left, right, r, c, n, prm, err, stats, None)

        refused = []
        for calib in (False, True):
            refused += [call(calib, ctx_h=None), call(calib, depth=None), call(calib, left=None), call(calib, right=None), call(calib, params=None),
                        call(calib, err=None, stats=None)]
            refused += [call(calib, r=rows + 1), call(calib, c=cols + 1), call(calib, n=b + 1), call(calib, r=0), call(calib, c=0), call(calib, n=0),
                        call(calib, r=-1)]
            refused += [call(calib, params=api.make_photo_error_params(window=w)) for w in (0, 5, -1, 1 << 20)]
            refused += [call(calib, depth=A["depth"] + 2), call(calib, stats=A["stats"] + 4), call(calib, stats=A["stats"] + 1)]
            # an output over an input, over the other output
            refused += [call(calib, err=A["left"]), call(calib, err=A["right"]), call(calib, err=A["depth"] + 3 * px), call(calib, err=A["left"] - 1),
                        call(calib, err=A["depth"] - px + 1), call(calib, stats=A["depth"]), call(calib, stats=A["left"] + 8), call(calib, stats=A["right"] + px - 8),
                        call(calib, stats=A["err"] + px - 8), call(calib, err=A["stats"] - px + 1), call(calib, err=A["stats"], stats=A["stats"])]
        for v in (np.nan, np.inf, -np.inf, 0.0, -0.0, -0.54):
            refused += [call(params=api.make_photo_error_params(baseline=v)), call(params=api.make_photo_error_params(focal=v))]
        refused += [call(True, table=None), call(True, table=A["table"] + 4), call(True, err=A["table"]), call(True, err=A["table"] - px + 1),
                    call(True, stats=A["table"]), call(True, stats=A["table"] - 56), call(True, stats=A["table"] + 8)]
        assert len(refused) > 80 and all(st == L.E_INVALID for st in refused), refused
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all()), "a refused call wrote something"
        # ... and the same arguments without the fault are taken (the table: two good records)
        buf[off["table"]:off["table"] + 16] = dev(api.make_stereo_calib([0.54, 0.3], 959.791).view(np.uint8))
        assert call() == L.OK and call(True) == L.OK and call(err=None) == L.OK and call(True, stats=None) == L.OK
        torch.cuda.synchronize()
        assert not bool((buf[off["stats"]:off["stats"] + 64] == 0xA5).all())
        assert bool((buf[:off["err"]] == 0xA5).all()), "a call wrote to its inputs"


def photo_case(rows, cols, b, window):
    """The call on three frames for tests/test_gpu_stream_order.py's scheme: real and decoy inputs, outputs with a fill."""
    from test_gpu_stream_order import Case, Out

    def inputs(which):
        depth = np.stack([R.random_depth(rows, cols, 500 + 10 * which + f) for f in range(b)])
        pairs = [R.random_pair(rows, cols, 600 + 10 * which + f) for f in range(b)]
        return {"depth": depth, "left": np.stack([p[0] for p in pairs]), "right": np.stack([p[1] for p in pairs])}

    def call(ctx, t, st):
        ctx.photo_error_dev(t["depth"], t["left"], t["right"], d_err=t["err"], d_stats=t["stats"], stream=st, window=window)

    def expect(inp):
        err, stats = R.batch(R.vectorised, inp["depth"], inp["left"], inp["right"], window=window)
        return {"err": err, "stats": stats.astype(np.int64)}

    return Case(f"photo_error_dev {rows}x{cols}x{b} window {window}", (rows, cols, b), inputs,
                {"err": Out((b, rows, cols), np.uint8), "stats": Out((b, 4), np.int64)}, call, expect)


@gpu
@pytest.mark.parametrize("rows,cols,window", [(65, 257, 2), (64, 256, 3)])
def test_queued_on_a_stream_behind_pending_work_without_host_syncs(rows, cols, window):
    """In the manner of tests/test_gpu_stream_order.py (its run_ordered, untouched): behind a delay kernel on a non-default stream,
    producer copies, the call, consumer copies and the restoring of decoys and fills are enqueued without the host ever waiting; the
    clones must be the restatement's bits for the real inputs, and the marker behind the delay must still be pending when the call
    returns (the call blocked on nothing).  The clear of the statistics is the call's own: a clear that ran early would be overwritten
    by the fill of the warm-up's restore, one that ran late would wipe the sums."""
    from test_gpu_stream_order import run_ordered
    run_ordered(photo_case(rows, cols, 3, window))


@gpu
def test_chained_behind_the_refinement_and_the_blur_on_one_stream():
    """stereo_refine_dev -> gaussian5_dev -> photo_error_dev, main_sl.cpp's tail, on one stream with no host synchronisation in between,
    equals the same three steps run singly, each synchronised and on a context of its own."""
    import torch
    rows, cols, b = 64, 256, 3
    depth = np.stack([R.random_depth(rows, cols, 70 + f) for f in range(b)])
    depth[depth == 0] = 20.0                                # a dense plane, as the refinement takes it
    pairs = [R.ramp_pair(rows, cols) for _ in range(b)]
    left = np.stack([np.roll(p[0], f, axis=1) for f, p in enumerate(pairs)])
    right = np.stack([np.roll(p[1], 3 * f, axis=1) for f, p in enumerate(pairs)])
    d, l, r = dev(depth), dev(left), dev(right)
    singly = []
    for step in range(3):
        with api.Context(0, rows, cols, b) as ctx:
            if step == 0:
                singly.append(ctx.stereo_refine_dev(d, l, r))
            elif step == 1:
                singly.append(ctx.gaussian5_dev(singly[0]))
            else:
                singly += list(ctx.photo_error_dev(singly[1], l, r))
            torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with api.Context(0, rows, cols, b) as ctx:
        s.wait_stream(torch.cuda.current_stream())
        refined = ctx.stereo_refine_dev(d, l, r, stream=s.cuda_stream)
        blurred = ctx.gaussian5_dev(refined, stream=s.cuda_stream)
        path = ctx.last_path()
        err, stats = ctx.photo_error_dev(blurred, l, r, stream=s.cuda_stream)
        before = ctx.photo_error_dev(d, l, r, err=False, stream=s.cuda_stream)      # the before / after picture, the same stream
        assert ctx.last_path() == path                      # not a cascade call: nothing reported, nothing carried
        s.synchronize()
    same(host(refined).view(np.uint32), host(singly[0]).view(np.uint32), "chain: refined")
    same(host(blurred).view(np.uint32), host(singly[1]).view(np.uint32), "chain: blurred")
    same(host(err), host(singly[2]), "chain: map")
    same(host(stats), host(singly[3]), "chain: stats")
    we, ws = R.batch(R.vectorised, host(blurred), left, right)
    same(host(err), we, "chain: map against the restatement")
    same(host(stats), ws.astype(np.int64), "chain: stats against the restatement")
    same(host(before), R.batch(R.vectorised, depth, left, right)[1].astype(np.int64), "chain: stats of the unrefined plane")


@gpu
def test_past_2_to_the_32_bytes_and_at_65535_frames():
    """Frame offsets are 64-bit: a batch whose depth planes end beyond 2^32 bytes (2600 frames of 352 x 1216: 4.45 GB of depth, 1.1 G
    pixels, so the byte planes pass 2^30 as well), compared on its first frame, the frame that straddles byte 2^32 of the depth, its
    neighbours and the last one; and the largest batch a context admits, 65535 frames (a grid's y dimension), every frame compared."""
    import torch
    rows, cols, b = 352, 1216, 2600
    assert b * rows * cols * 4 > 2 ** 32 and b * rows * cols > 2 ** 30
    g = torch.Generator(device="cuda").manual_seed(5)
    d = torch.rand((b, rows, cols), device="cuda", generator=g) * 78.5 + 1.5
    d[torch.rand((b, rows, cols), device="cuda", generator=g) < 0.3] = 0
    l = torch.randint(0, 256, (b, rows, cols), dtype=torch.uint8, device="cuda", generator=g)
    r = torch.randint(0, 256, (b, rows, cols), dtype=torch.uint8, device="cuda", generator=g)
    straddle = 2 ** 32 // (rows * cols * 4)
    picked = [0, straddle - 1, straddle, straddle + 1, b - 1]
    with api.Context(0, rows, cols, b) as ctx:
        err, stats = ctx.photo_error_dev(d, l, r)
        only_stats = ctx.photo_error_dev(d, l, r, err=False)
        stats = host(stats)
        same(host(only_stats), stats, "2600 frames: stats only")
        for f in picked:
            we, ws = R.vectorised(host(d[f]), host(l[f]), host(r[f]))
            same(host(err[f]), we, f"2600 frames: frame {f}, map")
            same(stats[f], ws.astype(np.int64), f"2600 frames: frame {f}, stats")
        # every frame's counts are its own plane's: nonzero and the sum, recomputed from the map on the device
        same(host((err > 0).flatten(1).sum(1)), stats[:, 2], "2600 frames: nonzero per frame")
        same(host(err.flatten(1).sum(1, dtype=torch.int64)), stats[:, 3], "2600 frames: sum per frame")
    del d, l, r, err
    rows, cols, b = 2, 9, 65535
    depth = np.tile(R.constant_depth(rows, cols, 40.0)[None], (b, 1, 1))
    depth[:, 1, 8] = np.linspace(600.0, 90000.0, b, dtype=f32)                    # a disparity that differs from frame to frame
    rng = np.random.default_rng(8)
    left, right = rng.integers(0, 256, (b, rows, cols), dtype=np.uint8), rng.integers(0, 256, (b, rows, cols), dtype=np.uint8)
    kw = dict(baseline=0.5, focal=1.0, window=1)
    with api.Context(0, rows, cols, b) as ctx:
        err, stats = ctx.photo_error_dev(dev(depth), dev(left), dev(right), **kw)
        err, stats = host(err), host(stats)
    for f in list(range(0, b, 257)) + [b - 2, b - 1]:
        we, ws = R.vectorised(depth[f], left[f], right[f], **kw)
        same(err[f], we, f"65535 frames: frame {f}, map")
        same(stats[f], ws.astype(np.int64), f"65535 frames: frame {f}, stats")
    assert (stats[:, 0] > 0).all() and np.array_equal((err > 0).reshape(b, -1).sum(1), stats[:, 2]) and \
        np.array_equal(err.reshape(b, -1).astype(np.int64).sum(1), stats[:, 3])
