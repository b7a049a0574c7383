"""The stereo matcher on the device: dcmt_sgm_dev / dcmt_sgm and their Python surface, bit for bit against tests/sgm_restatement.py (its
vectorised form, which tests/test_sgm.py holds against the pixel-by-pixel one without a GPU).  Every output is an integer or an
IEEE quotient of integers: every comparison is exact.

Shapes: the smallest at which the kernels can go wrong -- one pixel, one row, fewer rows than the block, fewer columns than D (x - d
clamps almost everywhere), idle lanes (D = 16, 48), two disparities a lane (D = 128), one column past a multiple of 256, the full
KITTI width at D = 64 and 128, one whole 375 x 1242 pair, and the two sides of the row kernel's LDS limit at D = 16 and 128: 3 x 4096
(all 64 KB of LDS staged) and 3 x 4097 (the rows read from global memory; tests/plan_sgm_test.cpp pins the route of each).  References are computed once per
(pair, D, p1, p2) and shared.

What is compared bit for bit beyond those shapes:
    winners at every targeted disparity   pairs whose answer is 1, D - 2 and D - 1 at D = 16, 48 and 128, and 62, 63, 64, 65 at D = 128
                                          (a lane carries d and d + 64: 63 | 64 is the step between its two registers), exact and half
                                          a pixel off (many sub-pixel fractions), and a staircase of bands at 0, 1, 62 .. 65, D - 2,
                                          D - 1; the conditions on these inputs are asserted from the restatement alone
    the UNIQUENESS x DISP12 grid          at D = 16, 48 (idle lanes) and 128 (two disparities a lane), on such pairs, both outputs
    both volumes                          C and S read back from the caller's workspace, every element, on both row routes and on
                                          columns ten times the lookahead; nothing written behind the batch's frames; with two
                                          chunks the last chunk's volumes
    a seeded differential fuzz            12 x 8 cases over shapes, D, penalties, checks, batch, workspace and outputs
    a 65535-frame batch                   past 2^32 bytes in the workspace and in the depth plane, 2^31 in disp16: the case
                                          "sgm_dev A" of tests/large_batch_cases.py, run by tests/test_gpu_large_batch.py"""
import ctypes
import functools
import itertools
import time

import numpy as np
import pytest

import sgm_restatement as R
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

gpu = pytest.mark.gpu
f32 = np.float32

# (rows, cols, D)
SHAPES = [(1, 1, 64), (1, 70, 64), (3, 33, 64), (7, 40, 64), (16, 70, 16), (9, 65, 48), (11, 130, 128), (24, 257, 64), (12, 1242, 64), (12, 1242, 128),
          (375, 1242, 64), (3, 4096, 16), (3, 4096, 128), (3, 4097, 16), (3, 4097, 128)]
PENALTIES = [(0, 0), (200, 800), (10000, 10000), (0, 10000)]
UNIQUENESS = [0, 10, 100]
DISP12 = [-1, 0, 1]


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                # (a copy: the shared frames are read-only)


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def pair(kind, rows, cols, D, seed=0):
    if kind == "shifted":
        out = R.shifted_pair(rows, cols, 100 + seed + rows + cols)
    elif kind == "same":
        out = R.shifted_pair(rows, cols, 200 + seed, shift=0)      # d* = 0 on most pixels: disp16 == 0
    elif kind == "stripes":
        out = R.stripes_pair(rows, cols)
    elif kind == "comb":
        out = R.comb_pair(rows, cols, D)
    elif kind == "box":
        out = R.box_scene(rows, cols, D, seed)[:2]
    elif kind == "staircase":
        out = R.staircase_scene(rows, cols, D, 5 + seed)[:2]
    elif kind == "half":                                           # d* = 63 | 64 where a lane carries two disparities
        out = R.shifted_pair(rows, cols, 400 + seed + rows + cols, min(63, D - 2), half=True)
    elif kind == "top":                                            # d* = D - 1
        out = R.shifted_pair(rows, cols, 500 + seed + rows + cols, D - 1)
    else:
        out = R.random_pair(rows, cols, 300 + seed + rows + cols)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=8)
def volumes(kind, rows, cols, D, seed, p1, p2):
    return R.vectorised_volumes(*pair(kind, rows, cols, D, seed), D, p1, p2)


@functools.lru_cache(maxsize=None)
def reference(kind, rows, cols, D, seed=0, p1=200, p2=800, uniqueness=10, disp12_max_diff=1):
    """disp16 of one pair: computed once, shared, read-only."""
    d16 = R.vectorised_select(volumes(kind, rows, cols, D, seed, p1, p2)[1], uniqueness, disp12_max_diff)
    d16.setflags(write=False)
    return d16


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    if got.dtype == f32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    neq = got != want
    if neq.any():
        first = tuple(np.argwhere(neq)[0])
        raise AssertionError(f"{what}: {int(neq.sum())} of {want.size} differ; first at {first}: {got[first]!r} vs {want[first]!r}")


def stack(kinds, rows, cols, D):
    lefts, rights = zip(*(pair(k, rows, cols, D) for k in kinds))
    return np.stack(lefts), np.stack(rights)


@gpu
@pytest.mark.parametrize("rows,cols,D", SHAPES)
def test_shapes_are_the_restatement_bit_for_bit(rows, cols, D):
    kinds = ("shifted",) if rows * cols > 100000 else ("shifted", "random", "same")
    lefts, rights = stack(kinds, rows, cols, D)
    want = np.stack([reference(k, rows, cols, D) for k in kinds])
    what = f"{rows}x{cols} D {D}"
    with api.Context(0, rows, cols, len(kinds)) as ctx:
        d16, depth = ctx.sgm_dev(dev(lefts), dev(rights), depth=True, num_disparities=D)
        same(host(d16), want, what + ": disp16")
        same(host(depth), R.depth_of(want), what + ": depth")
    if cols > 2 * 8 and rows >= 7:
        assert (np.abs(want[0][:, 8:-4] - 48) <= 8).mean() > 0.8, what        # the reference itself: 3 px found


@gpu
@pytest.mark.parametrize("p1,p2", PENALTIES)
def test_parameter_grid(p1, p2):
    rows, cols, D = 24, 96, 32
    kinds = ("box", "random", "stripes", "comb")
    lefts, rights = stack(kinds, rows, cols, D)
    l, r = dev(lefts), dev(rights)
    if p2 == 10000:        # the comb: S beyond what int16 holds
        assert volumes("comb", rows, cols, D, 0, p1, p2)[1].max() > 50000
    with api.Context(0, rows, cols, len(kinds)) as ctx:
        for u, lr in itertools.product(UNIQUENESS, DISP12):
            want = np.stack([reference(k, rows, cols, D, 0, p1, p2, u, lr) for k in kinds])
            got = ctx.sgm_dev(l, r, num_disparities=D, p1=p1, p2=p2, uniqueness=u, disp12_max_diff=lr)
            same(host(got), want, f"p1 {p1} p2 {p2} uniqueness {u} disp12 {lr}")


@gpu
def test_outputs_alone_and_together_and_the_depth_formula():
    rows, cols, D = 16, 70, 16
    kinds = ("shifted", "same", "random")
    lefts, rights = stack(kinds, rows, cols, D)
    l, r = dev(lefts), dev(rights)
    want = np.stack([reference(k, rows, cols, D) for k in kinds])
    assert (want == 0).any() and (want > 0).any() and (want == R.INVALID).any()
    with api.Context(0, rows, cols, 3) as ctx:
        both = ctx.sgm_dev(l, r, depth=True, num_disparities=D)
        only_disp = ctx.sgm_dev(l, r, num_disparities=D)
        only_depth = ctx.sgm_dev(l, r, disp16=False, depth=True, num_disparities=D)
        assert isinstance(both, tuple) and only_disp.dtype == both[0].dtype and only_depth.dtype == both[1].dtype
        same(host(both[0]), want, "both: disp16")
        same(host(only_disp), want, "disp16 alone")
        same(host(both[1]), R.depth_of(want), "both: depth")
        same(host(only_depth), R.depth_of(want), "depth alone")
        z = host(both[1])
        assert (z[want <= 0] == 0).all() and (z[want > 0] > 0).all()
        # constants no depth plane could be made of are nobody's business without one, in Python as in C ...
        same(host(ctx.sgm_dev(l, r, num_disparities=D, baseline=np.nan, focal=0.0, max_depth=-1.0)), want, "disp16 alone, unusable constants")
        for bad in (dict(baseline=np.nan), dict(focal=0.0), dict(max_depth=-1.0)):      # ... and refused with one
            with pytest.raises(ValueError):
                ctx.sgm_dev(l, r, depth=True, num_disparities=D, **bad)
        # the clamp, other constants
        for kw in (dict(max_depth=30.0), dict(baseline=0.1, focal=100.0), dict(baseline=2.0, focal=2000.0, max_depth=1e4)):
            got = ctx.sgm_dev(l, r, disp16=False, depth=True, num_disparities=D, **kw)
            same(host(got), R.depth_of(want, **{**{k: R.DEFAULTS[k] for k in ("baseline", "focal", "max_depth")}, **kw}), f"depth {kw}")
        # a clamp that cuts through the data: 10 / disparity against 3 -- the 3 px of the shifted pair are clamped, larger disparities not
        kw = dict(baseline=0.1, focal=100.0, max_depth=3.0)
        expected = R.depth_of(want, **kw)
        assert (expected == 3.0).any() and ((expected > 0) & (expected < 3.0)).any()
        same(host(ctx.sgm_dev(l, r, disp16=False, depth=True, num_disparities=D, **kw)), expected, f"depth {kw}")


@gpu
def test_chunks_determinism_and_a_dirty_workspace():
    import torch
    rows, cols, D, b = 24, 96, 32, 5
    kinds = ("box", "random", "shifted", "same", "comb")
    lefts, rights = stack(kinds, rows, cols, D)
    l, r = dev(lefts), dev(rights)
    want = np.stack([reference(k, rows, cols, D) for k in kinds])
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    with api.Context(0, rows, cols, b) as ctx:
        for held in (1, 2, 5):
            work = torch.full((held * one + 8,), 0xFF, dtype=torch.uint8, device="cuda")      # dirty, and a few bytes over
            d16, depth = ctx.sgm_dev(l, r, depth=True, d_work=work, num_disparities=D)
            same(host(d16), want, f"workspace of {held}: disp16")
            same(host(depth), R.depth_of(want), f"workspace of {held}: depth")
            again = ctx.sgm_dev(l, r, d_work=work, num_disparities=D)              # the same call on the workspace it left
            same(host(again), want, f"workspace of {held}: second run")
        same(host(ctx.sgm_dev(l, r, num_disparities=D, frames_in_flight=3)), want, "frames_in_flight 3")
        for f in range(b):
            same(host(ctx.sgm_dev(l[f:f + 1], r[f:f + 1], num_disparities=D))[0], want[f], f"frame {f} alone")
        too_small = torch.empty(one - 16, dtype=torch.uint8, device="cuda")
        with pytest.raises(api.DcmtError):
            ctx.sgm_dev(l, r, d_work=too_small, num_disparities=D)


# ---- stream order: the scheme of tests/test_gpu_stream_order.py, on its own -------------------------------------------------------------
def _ticks_per_ms():
    """torch.cuda._sleep spins for a number of clock ticks: how many make a millisecond, measured with events."""
    import torch
    n, ms = 1_000_000, 0.0
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 5.0:
            break
        n *= 8
    assert ms >= 5.0, f"torch.cuda._sleep({n}) took {ms} ms: unusable as a delay"
    return n / ms


def _delayed(stream, ms, ticks):
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(int(ms * ticks))
        marker = torch.cuda.Event()
        marker.record(stream)
    return marker


def _stream_beside_the_null_stream(ticks):
    """A stream whose work runs while the null stream is held up: a launch that escaped to the null stream would otherwise be
    serialised behind the delay and look right."""
    import torch
    null = torch.cuda.default_stream()
    for c in (torch.cuda.Stream() for _ in range(8)):
        if c.cuda_stream == null.cuda_stream:
            continue
        marker = _delayed(null, 20.0, ticks)
        with torch.cuda.stream(c):
            torch.zeros(16, device="cuda")
        c.synchronize()
        ran = not marker.query()
        null.synchronize()
        if ran:
            return c
    raise AssertionError("none of eight streams ran while the null stream was busy: an escaped launch could not be seen here")


@gpu
def test_queued_on_a_stream_behind_pending_work_without_host_syncs():
    """Behind a delay kernel on a non-default stream: the copy of the real inputs over decoys, the call (two chunks), clones of the outputs
    and the restoring of the decoys are enqueued without the host ever waiting.  The clones must be the real inputs' bits -- a kernel
    that ran early, or on another stream, reads the decoys -- and the marker behind the delay must still be pending when the call
    returns: the call blocked on nothing."""
    import torch
    rows, cols, D, b = 24, 96, 32, 3
    real = stack(("box", "shifted", "random"), rows, cols, D)
    decoy = stack(("random", "same", "box"), rows, cols, D)[::-1]          # other images, left and right swapped
    want = np.stack([reference(k, rows, cols, D) for k in ("box", "shifted", "random")])
    ticks = _ticks_per_ms()
    s = _stream_beside_the_null_stream(ticks)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    with api.Context(0, rows, cols, b) as ctx:
        decoy_l, decoy_r = dev(decoy[0]), dev(decoy[1])
        l, r = decoy_l.clone(), decoy_r.clone()
        real_l, real_r = dev(real[0]), dev(real[1])
        d16 = torch.full((b, rows, cols), 0x5A5A, dtype=torch.int16, device="cuda")
        depth = torch.full((b, rows, cols), -7.0, dtype=torch.float32, device="cuda")
        work = torch.zeros(2 * one, dtype=torch.uint8, device="cuda")
        call = lambda: ctx.sgm_dev(l, r, d_disp16=d16, d_depth=depth, d_work=work, stream=s.cuda_stream, num_disparities=D)
        torch.cuda.synchronize()
        call()                                                  # warm-up on the decoys: code objects loaded
        s.synchronize()
        decoy_result = host(d16)
        assert not np.array_equal(decoy_result, want)
        t0 = time.perf_counter()
        call()
        t_call = time.perf_counter() - t0
        s.synchronize()
        d16.fill_(0x5A5A)
        depth.fill_(-7.0)
        torch.cuda.synchronize()
        d_ms = min(1000.0, max(100.0, 20.0 * t_call * 1e3))
        marker = _delayed(s, d_ms, ticks)
        with torch.cuda.stream(s):
            l.copy_(real_l)
            r.copy_(real_r)
            call()
            pending = not marker.query()
            got16, got_depth = d16.clone(), depth.clone()
            l.copy_(decoy_l)
            r.copy_(decoy_r)
        s.synchronize()
        assert pending, f"the marker behind a {d_ms:.0f} ms delay was complete when the call returned (t_call {t_call * 1e3:.3f} ms)"
        same(host(got16), want, "behind the delay: disp16")
        same(host(got_depth), R.depth_of(want), "behind the delay: depth")


@gpu
def test_every_refusal_returns_invalid_and_writes_nothing():
    import torch
    rows, cols, b, D = 8, 16, 2, 16
    px = b * rows * cols
    lib = L.lib()
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    # one buffer, so that overlapping arguments can be named: left | right | disp16 | depth | work, each region 16-byte aligned
    off = {"left": 0, "right": px, "disp": 2 * px, "depth": 4 * px, "work": 8 * px, "end": 8 * px + 2 * one}
    buf = torch.full((off["end"],), 0xA5, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    assert base % 16 == 0
    A = {k: base + v for k, v in off.items()}
    good = api.make_sgm_params(num_disparities=D)

    def prm(**kw):
        p = api.make_sgm_params(num_disparities=D)
        for k, v in kw.items():
            setattr(p, k, v)                                    # past make_sgm_params, which would raise
        return p

    with api.Context(0, rows, cols, b) as ctx:
        def call(ctx_h=ctx._h, left=A["left"], right=A["right"], disp=A["disp"], depth=A["depth"], r=rows, c=cols, n=b, params=good, work=A["work"],
                 work_bytes=2 * one):
            return lib.dcmt_sgm_dev(ctx_h, left, right, disp, depth, r, c, n, ctypes.byref(params) if params is not None else None, work, work_bytes, None)

        refused = [call(ctx_h=None), call(left=None), call(right=None), call(disp=None, depth=None), call(params=None), call(work=None)]
        refused += [call(params=prm(num_disparities=d)) for d in (0, 8, 24, 17, 144, 256, -16, 1 << 20)]
        refused += [call(params=prm(p1=-1)), call(params=prm(p1=801)), call(params=prm(p2=10001)), call(params=prm(p1=300, p2=200)),
                    call(params=prm(uniqueness=-1)), call(params=prm(uniqueness=101))]
        for v in (np.nan, np.inf, -np.inf, 0.0, -0.0, -0.54):
            refused += [call(params=prm(baseline=v)), call(params=prm(focal=v)), call(params=prm(max_depth=v))]
        refused += [call(disp=A["disp"] + 1), call(depth=A["depth"] + 2), call(depth=A["depth"] + 1), call(work=A["work"] + 8), call(work=A["work"] + 4),
                    call(work=A["work"] + 1)]
        refused += [call(work_bytes=one - 1), call(work_bytes=0), call(work_bytes=16)]
        refused += [call(r=rows + 1), call(c=cols + 1), call(n=b + 1), call(r=0), call(c=0), call(n=0), call(r=-1)]
        # overlaps: an output over an input, over the other output, over the workspace; the workspace over an input
        refused += [call(disp=A["left"]), call(disp=A["right"]), call(disp=A["right"] + px - 2), call(depth=A["left"]), call(depth=A["right"] + px - 4),
                    call(disp=A["depth"]), call(disp=A["depth"] - 2), call(depth=A["disp"]), call(depth=A["disp"] + 2 * px - 4),
                    call(disp=A["work"]), call(depth=A["work"] + 2 * one - 16), call(depth=A["work"] - 4 * px + 16), call(work=A["left"], work_bytes=one),
                    call(work=A["depth"] + 4 * px - 16), call(work=A["right"] - one + 16, work_bytes=one), call(disp=A["disp"], depth=A["disp"])]
        assert len(refused) > 60 and all(st == L.E_INVALID for st in refused), refused
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all()), "a refused call wrote something"
        # a baseline that is refused with a depth plane is nobody's business without one; the same arguments without a fault are taken
        assert call(depth=None, params=prm(baseline=np.nan, focal=0.0, max_depth=-1.0)) == L.OK
        assert call() == L.OK and call(disp=None) == L.OK and call(work_bytes=one) == L.OK and call(right=A["left"]) == L.OK
        torch.cuda.synchronize()
        assert not bool((buf[off["disp"]:off["work"]] == 0xA5).all())
        assert bool((buf[:off["disp"]] == 0xA5).all()), "a call wrote to its inputs"


@gpu
def test_host_forms_agree_with_the_device_entry():
    rows, cols, D = 24, 257, 64
    left, right = pair("shifted", rows, cols, D)
    want = reference("shifted", rows, cols, D)
    with api.Context(0, rows, cols, 1) as ctx:
        d16, depth = ctx.sgm(left, right, depth=True)
        same(d16, want, "host entry: disp16")
        same(depth, R.depth_of(want), "host entry: depth")
        same(ctx.sgm(left, right), want, "host entry: disp16 alone")
        same(ctx.sgm(left, right, disp16=False, depth=True, max_depth=20.0), R.depth_of(want, max_depth=20.0), "host entry: depth alone")
        wide = np.full((rows, cols + 5), 9, np.uint8)          # rows further apart than they need to be
        wide[:, :cols] = left
        same(ctx.sgm(wide[:, :cols], right), want, "host entry, padded rows")
        with pytest.raises(ValueError):
            ctx.sgm(left, right, num_disparities=20)
    same(api.stereo_sgm(left, right), want, "stereo_sgm")
    d16, depth = api.stereo_sgm(left, right, depth=True, uniqueness=0, disp12_max_diff=-1)
    want_loose = reference("shifted", rows, cols, D, 0, 200, 800, 0, -1)
    same(d16, want_loose, "stereo_sgm, no checks: disp16")
    same(depth, R.depth_of(want_loose), "stereo_sgm, no checks: depth")
    # BGR inputs go through bgr_to_gray
    rng = np.random.default_rng(3)
    bgr_l, bgr_r = rng.integers(0, 256, (12, 40, 3), dtype=np.uint8), rng.integers(0, 256, (12, 40, 3), dtype=np.uint8)
    same(api.stereo_sgm(bgr_l, bgr_r, num_disparities=16), R.vectorised(api.bgr_to_gray(bgr_l), api.bgr_to_gray(bgr_r), num_disparities=16)[0], "stereo_sgm, BGR")


@gpu
def test_chained_in_front_of_the_refinement_and_the_error_map_on_one_stream():
    """sgm_dev(depth) -> stereo_refine_dev -> photo_error_dev on one stream with no host synchronisation in between equals the
    restatements chained on the CPU: the matcher's depth plane is what the two take, zeros (invalid pixels) included."""
    import torch
    import photo_error_restatement as P
    from oracle import oracle as O
    rows, cols, D, b = 24, 96, 32, 2
    kw = dict(baseline=0.5, focal=64.0)                          # disparities of 3..12 px are depths of 2.7..10.7
    lefts, rights = stack(("box", "shifted"), rows, cols, D)
    want16 = np.stack([reference(k, rows, cols, D) for k in ("box", "shifted")])
    want_depth = R.depth_of(want16, max_depth=100.0, **kw)
    assert (want_depth == 0).any() and (want_depth > 0).mean() > 0.8
    want_refined = np.stack([O.stereo_refine(want_depth[f], lefts[f], rights[f], **kw) for f in range(b)])
    want_err, want_stats = P.batch(P.vectorised, want_refined, lefts, rights, **kw)
    s = torch.cuda.Stream()
    l, r = dev(lefts), dev(rights)
    with api.Context(0, rows, cols, b) as ctx:
        s.wait_stream(torch.cuda.current_stream())
        d16, depth = ctx.sgm_dev(l, r, depth=True, stream=s.cuda_stream, num_disparities=D, **kw)
        refined = ctx.stereo_refine_dev(depth, l, r, stream=s.cuda_stream, **kw)
        err, stats = ctx.photo_error_dev(refined, l, r, stream=s.cuda_stream, **kw)
        s.synchronize()
    same(host(d16), want16, "chain: disp16")
    same(host(depth), want_depth, "chain: depth")
    same(host(refined), want_refined.astype(f32), "chain: refined")
    same(host(err), want_err, "chain: error map")
    same(host(stats), want_stats.astype(np.int64), "chain: counts")


# ---- winners across the disparity range -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def targets(D):
    """The target pairs of one D (tests/sgm_restatement.py: TARGET_SHIFTS, exact and half) as a batch, and their references."""
    pairs = [R.target_pair(D, shift, half) for shift, half in R.target_pairs(D)]
    lefts, rights = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = np.stack([R.vectorised(l, r, num_disparities=D)[0] for l, r in pairs])
    for a in (lefts, rights, want):
        a.setflags(write=False)
    return lefts, rights, want


@functools.lru_cache(maxsize=None)
def staircases(D, n=3):
    scenes = [R.staircase_scene(R.STAIR_ROWS, R.staircase_cols(D), D, 5 + s) for s in range(n)]
    want = np.stack([R.vectorised(l, r, num_disparities=D)[0] for l, r, _ in scenes])
    return np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes]), want, scenes[0][2]


@gpu
@pytest.mark.parametrize("D", list(R.TARGET_SHIFTS))
def test_winners_at_every_targeted_disparity(D):
    """Pairs whose answer is the chosen disparity -- 1, D - 2, D - 1, and 62 .. 65 where a lane carries d and d + 64 -- exact and
    half a pixel off, and the staircase: the conditions on the inputs (from the reference alone), then disp16 and depth bit for
    bit.  What the verified pixels pass through: held() on both registers, the sub-pixel step whose neighbours sit in different
    registers, the left-right gather and the rival test in the second register, the d* = D - 1 and D - 2 edges of the sub-pixel rule."""
    lefts, rights, want = targets(D)
    R.assert_targets_found(D, dict(zip(R.target_pairs(D), want)))
    rows, cols = lefts.shape[1:]
    with api.Context(0, rows, cols, len(lefts)) as ctx:
        d16, depth = ctx.sgm_dev(dev(lefts), dev(rights), depth=True, num_disparities=D)
        for f, (shift, half) in enumerate(R.target_pairs(D)):
            same(host(d16[f]), want[f], f"D {D} shift {shift} half {half}: disp16")
        same(host(depth), R.depth_of(want), f"D {D} target pairs: depth")
    lefts, rights, want, truth = staircases(D)
    R.assert_staircase_found(D, want[0], truth)
    rows, cols = lefts.shape[1:]
    with api.Context(0, rows, cols, len(lefts)) as ctx:
        d16, depth = ctx.sgm_dev(dev(lefts), dev(rights), depth=True, num_disparities=D)
        same(host(d16), want, f"D {D} staircase: disp16")
        same(host(depth), R.depth_of(want), f"D {D} staircase: depth")


GRID_KINDS = ("staircase", "half", "top", "random", "comb")


@gpu
@pytest.mark.parametrize("p1,p2", [(200, 800), (0, 10000)])
@pytest.mark.parametrize("D", [16, 48, 128])
def test_parameter_grid_with_idle_lanes_and_two_disparities_a_lane(D, p1, p2):
    """UNIQUENESS x DISP12 where lanes idle (D = 16, 48) and where a lane carries two disparities (D = 128), on pairs whose
    winners lie across the range: without the two checks (uniqueness 0, disp12 -1) every pixel with x >= d* is valid, so the value
    computed for it is compared."""
    rows, cols = 12, R.staircase_cols(D)
    lefts, rights = stack(GRID_KINDS, rows, cols, D)
    l, r = dev(lefts), dev(rights)
    if p2 == 10000:        # the comb: S beyond what int16 holds
        assert volumes("comb", rows, cols, D, 0, p1, p2)[1].max() > 50000
    if D == 128:           # the reference alone: the random pair has verified winners in the second register and on both sides of the step
        loose = reference("random", rows, cols, D, 0, p1, p2, 0, -1)
        whole = loose[loose >= 0] >> 4
        assert (whole >= 64).sum() >= 100 and (whole == 63).any() and (whole == 64).any(), ((whole >= 64).sum(), (whole == 63).sum(), (whole == 64).sum())
    with api.Context(0, rows, cols, len(GRID_KINDS)) as ctx:
        for u, lr in itertools.product(UNIQUENESS, DISP12):
            want = np.stack([reference(k, rows, cols, D, 0, p1, p2, u, lr) for k in GRID_KINDS])
            got, depth = ctx.sgm_dev(l, r, depth=True, num_disparities=D, p1=p1, p2=p2, uniqueness=u, disp12_max_diff=lr)
            same(host(got), want, f"D {D} p1 {p1} p2 {p2} uniqueness {u} disp12 {lr}: disp16")
            same(host(depth), R.depth_of(want), f"D {D} p1 {p1} p2 {p2} uniqueness {u} disp12 {lr}: depth")


# ---- the volumes ---------------------------------------------------------------------------------------------------------------------------
# the two row routes at D = 16 and 128, and 40 rows: the column paths run ten times their lookahead
VOLUME_SHAPES = [(7, 40, 64), (9, 65, 48), (11, 130, 128), (3, 4096, 16), (3, 4097, 128), (40, 200, 128)]
VOLUME_RUNS = [(("staircase", "random", "stripes"), 200, 800), (("comb", "staircase"), 0, 10000)]


def workspace_volumes(work, slot, rows, cols, D):
    """(C, S) of the frame in slot `slot` of a workspace (a uint8 tensor), by the layout include/dcmt.h states: per frame in flight
    C, then S volume_elems behind it, each uint16 [rows][cols][D]."""
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    elems = rows * cols * D
    assert one == 2 * 2 * elems
    both = host(work[slot * one:(slot + 1) * one]).view(np.uint16)
    return both[:elems].reshape(rows, cols, D), both[elems:].reshape(rows, cols, D)


def same_volumes(work, slot, kind, rows, cols, D, p1, p2, what):
    C, S = workspace_volumes(work, slot, rows, cols, D)
    wantC, wantS = volumes(kind, rows, cols, D, 0, p1, p2)
    same(C, wantC.astype(np.uint16), f"{what}: C")
    same(S, wantS.astype(np.uint16), f"{what}: S")


@gpu
@pytest.mark.parametrize("rows,cols,D", VOLUME_SHAPES)
def test_both_volumes_are_the_restatement_element_for_element(rows, cols, D):
    """C and S as k_sgm_rows and k_sgm_cols leave them in the caller's workspace: every element, so also the disparities that
    neither win nor rival.  One chunk: the workspace holds the batch and a frame more, filled with 0xFF; behind the batch's frames
    it must still hold 0xFF."""
    import torch
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    for kinds, p1, p2 in VOLUME_RUNS:
        b = len(kinds)
        lefts, rights = stack(kinds, rows, cols, D)
        work = torch.full(((b + 1) * one,), 0xFF, dtype=torch.uint8, device="cuda")
        with api.Context(0, rows, cols, b) as ctx:
            d16 = ctx.sgm_dev(dev(lefts), dev(rights), d_work=work, num_disparities=D, p1=p1, p2=p2)
        for f, kind in enumerate(kinds):
            same_volumes(work, f, kind, rows, cols, D, p1, p2, f"{rows}x{cols} D {D} p2 {p2} {kind}")
        assert bool((work[b * one:] == 0xFF).all()), f"{rows}x{cols} D {D}: the workspace was written behind its {b} frames"
        same(host(d16), np.stack([reference(k, rows, cols, D, 0, p1, p2) for k in kinds]), f"{rows}x{cols} D {D} p2 {p2}: disp16")
        if "comb" in kinds and rows >= 7 and cols > D:
            assert volumes("comb", rows, cols, D, 0, p1, p2)[1].max() > 32767          # S that an int16 volume could not hold


@gpu
def test_volumes_of_the_last_chunk_stay_in_the_workspace():
    """Two chunks: three frames through a workspace of two.  Slot 0 ends with the volumes of frame 2 (the last chunk), slot 1 with
    those of frame 1 (the first chunk's second frame, which nothing has written over)."""
    import torch
    rows, cols, D = 11, 130, 128
    kinds = ("staircase", "random", "stripes")
    lefts, rights = stack(kinds, rows, cols, D)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    work = torch.full((3 * one,), 0xFF, dtype=torch.uint8, device="cuda")
    with api.Context(0, rows, cols, 3) as ctx:
        d16 = ctx.sgm_dev(dev(lefts), dev(rights), d_work=work[:2 * one], num_disparities=D)
    same_volumes(work, 0, kinds[2], rows, cols, D, 200, 800, "two chunks, slot 0: frame 2")
    same_volumes(work, 1, kinds[1], rows, cols, D, 200, 800, "two chunks, slot 1: frame 1")
    assert bool((work[2 * one:] == 0xFF).all())
    same(host(d16), np.stack([reference(k, rows, cols, D) for k in kinds]), "two chunks: disp16")


# ---- seeded differential fuzz ---------------------------------------------------------------------------------------------------------------
FUZZ_ELEMS = 1_500_000         # rows * cols * D * batch of one case: about 0.2 s of the vectorised restatement


def _fuzz_pair(g, rows, cols, D):
    kind = int(g.integers(0, 8))
    seed = int(g.integers(0, 1 << 30))
    if kind == 0:
        return R.random_pair(rows, cols, seed)
    if kind == 1:
        return R.shifted_pair(rows, cols, seed, int(g.integers(0, D)), half=bool(g.integers(0, 2)))
    if kind == 2:
        return R.stripes_pair(rows, cols, int(g.choice([0, 128, 255])))
    if kind == 3:
        return R.comb_pair(rows, cols, D)
    if kind == 4:
        return R.box_scene(rows, cols, D, seed)[:2]
    if kind == 5:                                                       # a staircase with a random set of band disparities
        return R.staircase_scene(rows, cols, D, seed, disparities=g.choice(D, int(g.integers(1, 7)), replace=False))
    if kind == 6:
        return R.staircase_scene(rows, cols, D, seed)[:2]
    left = R.random_pair(rows, cols, seed)[0]                            # the same image twice: d* = 0 wherever it is unique
    return left, left.copy()


@gpu
@pytest.mark.parametrize("seed", range(12))
def test_fuzz_against_the_restatement(seed):
    import torch
    g = np.random.Generator(np.random.PCG64(26000 + seed))
    for case in range(8):
        D = int(g.choice([16, 32, 48, 64, 80, 128]))
        batch = int(g.choice([1, 2, 7]))
        cols = int(g.integers(1, 301))
        rows = min(int(g.integers(1, 41)), max(1, FUZZ_ELEMS // (cols * D * batch)))
        p2 = int(g.integers(0, 10001)) if g.random() < 0.6 else int(g.choice([0, 800, 10000]))
        p1 = int(g.integers(0, p2 + 1))
        kw = dict(num_disparities=D, p1=p1, p2=p2, uniqueness=int(g.integers(0, 101)), disp12_max_diff=int(g.choice([-1, 0, 1, 2, 5])))
        held = int(g.integers(1, batch + 1))
        outputs = ("both", "disp16", "depth")[int(g.integers(0, 3))]
        pairs = [_fuzz_pair(g, rows, cols, D)[:2] for _ in range(batch)]
        what = f"seed {seed} case {case}: {batch} x {rows}x{cols} {kw} workspace of {held}, {outputs}"
        lefts, rights = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        want16, want_depth = R.batch(R.vectorised, lefts, rights, **kw)
        work = torch.full((held * api.sgm_workspace_bytes(rows, cols, D, 1),), 0xFF, dtype=torch.uint8, device="cuda")
        with api.Context(0, rows, cols, batch) as ctx:
            got = ctx.sgm_dev(dev(lefts), dev(rights), disp16=outputs != "depth", depth=outputs != "disp16", d_work=work, **kw)
        got16, got_depth = got if outputs == "both" else (got, None) if outputs == "disp16" else (None, got)
        if got16 is not None:
            same(host(got16), want16, what + ": disp16")
        if got_depth is not None:
            same(host(got_depth), want_depth, what + ": depth")
