"""The speckle filter on the device (dcmt_filter_speckles_dev) against the restatements of tests/speckle_restatement.py, bit for bit:
out, depth and removed, at the smallest shapes at which the kernels can still go wrong -- one pixel, one row, exactly one tile of
64 x 16 (no border launch), one more row and column of tiles, a frame of many tiles -- the non-transitive block at every position
relative to a tile corner, ramps and serpentines across 3 x 3 tiles with the threshold counted across tiles, the int16 extremes, in
place against out of place, batches, refusals, stream order behind pending work, and the sizes at which an offset passes 2^32."""
import ctypes
import functools
import itertools
import time

import numpy as np
import pytest

import sgm_restatement as G
import speckle_restatement as R
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api
from test_gpu_sgm import _delayed, _stream_beside_the_null_stream, _ticks_per_ms, dev, host, same

gpu = pytest.mark.gpu
f32 = np.float32

SHAPES = [(1, 1), (1, 70), (16, 64), (17, 65), (33, 129), (5, 4097), (375, 1242)]
PLANES = list(itertools.product((1, 3, 8), (0.3, 0.6, 0.9)))            # (k, live fraction)


def grid(rows, cols, full):
    sizes = sorted({0, 1, 5, 200, rows * cols})
    if full:
        return list(itertools.product(R.MAX_DIFFS, sizes))
    # every max_diff and every max_size once
    return [(0, 1), (15, 0), (16, 5), (32, 200), (65535, rows * cols)]


@functools.lru_cache(maxsize=None)
def planes(rows, cols, count=len(PLANES), new_val=-16):
    out = np.stack([R.random_plane(rows, cols, k, live, 1000 * rows + cols + i, new_val) for i, (k, live) in enumerate(PLANES[:count])])
    out.setflags(write=False)
    return out


def expect(v, depth=None, **kw):
    """(out, depth' or None, removed uint32 [batch]) of a batch, from the vectorised restatement."""
    return R.batch(R.vectorised, v, depth, **kw)


def run(ctx, v, depth=None, in_place=False, removed=True, **kw):
    """One device call on copies of v / depth: (out, depth' or None, removed or None) on the host."""
    import torch
    d = dev(v)
    z = dev(depth) if depth is not None else None
    n = torch.full((v.shape[0],), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if removed else None
    out = ctx.filter_speckles_dev(d, d_depth=z, d_out=d if in_place else None, d_removed=n, **kw)
    out = out[0] if removed else out
    if in_place:
        assert out.data_ptr() == d.data_ptr()
    else:
        same(host(d), v, "the source of an out-of-place call")
    return host(out), host(z) if z is not None else None, host(n).view(np.uint32) if removed else None


def check(ctx, v, what, depth=None, in_place=False, **kw):
    want, want_z, want_n = expect(v, depth, **kw)
    got, got_z, got_n = run(ctx, v, depth, in_place, **kw)
    same(got, want, f"{what}: out")
    same(got_n, want_n, f"{what}: removed")
    if depth is not None:
        same(got_z, want_z, f"{what}: depth")
    return want, want_n


@gpu
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_shapes_are_the_restatement_bit_for_bit(rows, cols):
    big = rows * cols > 100000
    # (the one large frame: two planes whose components stay small enough for the restatement to take a second, two parameter sets)
    v = planes(rows, cols)[[4, 8]] if big else planes(rows, cols)
    depth = R.depth_pattern(v.shape, rows)
    changed = kept = 0
    with api.Context(0, rows, cols, v.shape[0]) as ctx:
        for max_diff, max_size in [(16, 5), (32, 200)] if big else grid(rows, cols, full=(rows, cols) == (33, 129)):
            want, n = check(ctx, v, f"{rows}x{cols} max_diff {max_diff} max_size {max_size}", depth, max_diff=max_diff, max_size=max_size)
            changed += int(n.sum())
            kept += int((want != -16).sum())
    assert changed > 0 and (kept > 0 or rows * cols == 1)


@gpu
def test_the_block_whose_top_pair_is_no_edge_at_every_position_of_a_tile_corner():
    """[[-32, 32], [0, 0]] and its rotations at max_diff 32: one component of 4 through three edges, the fourth pair no edge.  Inside a
    tile (the left-neighbour skip of the tile-local kernel), across x = 63|64 and across y = 15|16 (the one-step-back skip of the
    border kernel, both directions), and across both."""
    rows, cols = 34, 130
    spots = [(3, 5), (8, 62), (8, 63), (9, 63), (14, 30), (15, 30), (15, 31), (15, 63), (14, 63), (15, 62), (14, 62), (31, 127), (0, 0), (0, 63), (15, 0)]
    frames = np.stack([R.block_plane(rows, cols, y, x, rot) for (y, x), rot in itertools.product(spots, range(4))])
    # ... and in a live neighbourhood: the block's values on a plane of far-away values that join nothing
    busy = frames.copy()
    far = (1000 + 100 * ((np.arange(rows)[:, None] + 2 * np.arange(cols)[None, :]) % 7)).astype(np.int16)
    busy[frames == -16] = np.broadcast_to(far, frames.shape)[frames == -16]
    with api.Context(0, rows, cols, frames.shape[0]) as ctx:
        for v, name in ((frames, "alone"), (busy, "among singletons")):
            want, n = check(ctx, v, f"block {name}, max_size 3", max_size=3, max_diff=32)
            if name == "alone":
                assert (n == 0).all() and np.array_equal(want, v)              # one component of 4: kept.  Split in two: removed
            want, n = check(ctx, v, f"block {name}, max_size 4", max_size=4, max_diff=32)
            if name == "alone":
                assert (n == 4).all() and (want == -16).all()
            check(ctx, v, f"block {name}, max_diff 31", max_size=1, max_diff=31)


@gpu
def test_ramps_and_serpentines_across_three_by_three_tiles():
    rows, cols = 48, 192
    frames, kws = [], []
    for max_diff in (1, 32, 100):
        frames += [R.ramp(rows, cols, max_diff), R.ramp(rows, cols, max_diff + 1)]
        kws += [dict(max_diff=max_diff), dict(max_diff=max_diff)]
    with api.Context(0, rows, cols, 4) as ctx:
        for v, kw in zip(frames, kws):
            one = v[None]
            want, n = check(ctx, one, f"ramp {kw}, window n - 1", max_size=rows * cols - 1, **kw)
            check(ctx, one, f"ramp {kw}, window n", max_size=rows * cols, **kw)
            check(ctx, one, f"ramp {kw}, window 1", max_size=1, **kw)
        # one component of rows * cols pixels, then rows * cols singletons
        assert expect(frames[2][None], max_size=rows * cols - 1, max_diff=32)[2][0] == 0
        assert expect(frames[3][None], max_size=1, max_diff=32)[2][0] == rows * cols
        for max_size in (200, 3000):
            v = np.stack([R.serpentine(rows, cols, max_size), R.serpentine(rows, cols, max_size + 1),
                          R.serpentine(rows, cols, max_size)[:, ::-1].copy(), R.serpentine(rows, cols, max_size + 1)[::-1].copy()])
            want, n = check(ctx, v, f"serpentines at {max_size}", R.depth_pattern(v.shape, 3), max_size=max_size, max_diff=0)
            assert n.tolist() == [max_size, 0, max_size, 0]                    # the threshold, counted across tiles
        # a serpentine down the columns: chains across horizontal tile edges
        v = np.stack([np.ascontiguousarray(R.serpentine(cols, rows, n).T) for n in (3000, 3001)])
        want, n = check(ctx, v, "column serpentines", max_size=3000, max_diff=0)
        assert n.tolist() == [3000, 0]


@gpu
def test_int16_extremes_and_other_new_vals():
    with api.Context(0, 20, 70, len(PLANES)) as ctx:
        for v in (np.array([[[-32768, 32767]]], np.int16), np.array([[[-32768], [32767]]], np.int16)):
            # joined at 65535: one component of 2; not at 65534: two singletons
            for max_diff, max_size, gone in ((65535, 2, 2), (65535, 1, 0), (65534, 1, 2), (65534, 0, 0)):
                want, n = check(ctx, v, f"extremes {v.shape} {max_diff} {max_size}", max_diff=max_diff, max_size=max_size)
                assert n[0] == gone
        # a checkerboard of the two: every neighbour is the other extreme
        board = np.where((np.arange(20)[:, None] + np.arange(70)[None, :]) % 2 == 0, -32768, 32767).astype(np.int16)[None]
        for max_diff, max_size, gone in ((65535, 1400, 1400), (65535, 1399, 0), (65534, 1, 1400), (65534, 0, 0)):
            want, n = check(ctx, board, f"checkerboard {max_diff} {max_size}", R.depth_pattern(board.shape, 1), max_diff=max_diff, max_size=max_size)
            assert n[0] == gone
        for new_val in (-16, 0, 123):
            v = np.array(planes(20, 70, len(PLANES), new_val))
            v[:, 0, 0] = -16 if new_val != -16 else 7
            for max_diff, max_size in ((16, 5), (0, 200), (32, 1)):
                check(ctx, v, f"new_val {new_val} {max_diff} {max_size}", R.depth_pattern(v.shape, 5), max_diff=max_diff, max_size=max_size, new_val=new_val)
        check(ctx, np.full((2, 20, 70), -16, np.int16), "nothing live", R.depth_pattern((2, 20, 70)), max_size=1400)
        v = np.full((1, 20, 70), 77, np.int16)
        assert check(ctx, v, "constant, n - 1", max_size=1399, max_diff=0)[1][0] == 0 and check(ctx, v, "constant, n", max_size=1400, max_diff=0)[1][0] == 1400


@gpu
def test_in_place_and_out_of_place_with_and_without_the_companions():
    import torch
    for rows, cols in ((33, 129), (32, 128)):                 # one pixel a thread; four
        v = planes(rows, cols)
        b = v.shape[0]
        depth = R.depth_pattern(v.shape, 9)
        kw = dict(max_size=5, max_diff=16)
        want, want_z, want_n = expect(v, depth, **kw)
        assert 0 < want_n.sum() < (v != -16).sum()
        with api.Context(0, rows, cols, b) as ctx:
            for in_place, with_depth, with_removed in itertools.product((False, True), repeat=3):
                got, got_z, got_n = run(ctx, v, depth if with_depth else None, in_place, with_removed, **kw)
                what = f"{rows}x{cols} in_place {in_place} depth {with_depth} removed {with_removed}"
                same(got, want, what + ": out")
                if with_depth:
                    same(got_z, want_z, what + ": depth")
                if with_removed:
                    same(got_n, want_n, what + ": removed")
            # 2-byte-but-not-4-byte aligned planes: source, output, both, in place
            n = v.size
            for src_off, out_off in ((0, 1), (1, 0), (1, 1), (3, 1), (1, None)):
                sbuf = torch.full((n + 4,), 0x7A7A, dtype=torch.int16, device="cuda")
                obuf = torch.full((n + 4,), 0x7A7A, dtype=torch.int16, device="cuda")
                src = sbuf[src_off:src_off + n].view(b, rows, cols)
                src.copy_(dev(v))
                out = src if out_off is None else obuf[out_off:out_off + n].view(b, rows, cols)
                assert src.data_ptr() % 4 == 2 or out.data_ptr() % 4 == 2
                z = dev(depth)
                got, got_n = ctx.filter_speckles_dev(src, d_depth=z, d_out=out, removed=True, **kw)
                what = f"{rows}x{cols} offsets {src_off} {out_off}"
                same(host(got), want, what + ": out")
                same(host(z), want_z, what + ": depth")
                same(host(got_n).view(np.uint32), want_n, what + ": removed")
                if out_off is not None:
                    guard = torch.cat([obuf[:out_off], obuf[out_off + n:], sbuf[:src_off], sbuf[src_off + n:]])
                    assert bool((guard == 0x7A7A).all()), what + ": wrote outside its plane"
                    same(host(src), v, what + ": source")


@gpu
def test_batches_repeats_and_dirty_scratch():
    import torch
    rows, cols, b = 33, 129, 5
    v = planes(rows, cols)[:b]
    depth = R.depth_pattern(v.shape, 2)
    kw = dict(max_size=5, max_diff=16)
    want, want_z, want_n = expect(v, depth, **kw)
    with api.Context(0, 40, 140, 6) as ctx:                      # a context larger than the call: strides are the call's
        first = run(ctx, v, depth, **kw)
        for name, got, w in zip(("out", "depth", "removed"), first, (want, want_z, want_n)):
            same(got, w, f"batch of {b}: {name}")
        for f in range(b):                                       # frame by frame equals the batch call
            got, got_z, got_n = run(ctx, v[f:f + 1], depth[f:f + 1], **kw)
            same(got[0], want[f], f"frame {f} alone: out")
            same(got_z[0], want_z[f], f"frame {f} alone: depth")
            assert got_n[0] == want_n[f]
        # the frames in another order, at another position of the batch
        order = [3, 0, 4, 1, 2]
        got, got_z, got_n = run(ctx, v[order], depth[order], **kw)
        same(got, want[order], "reordered: out")
        same(got_n, want_n[order], "reordered: removed")
        # scratch planes full of another call's leftovers: a completion, then a filter of other planes with other parameters
        sparse = torch.zeros((6, 40, 140), dtype=torch.float32, device="cuda")
        sparse[:, ::3, ::5] = 7.5
        ctx.complete_dev(sparse)
        run(ctx, np.array(planes(40, 140)[:6]), None, max_size=1400, max_diff=65535)
        for i in range(3):
            again = run(ctx, v, depth, **kw)
            for name, got, w in zip(("out", "depth", "removed"), again, (want, want_z, want_n)):
                same(got, w, f"repeat {i} behind other calls: {name}")


@gpu
def test_every_refusal_returns_invalid_and_writes_nothing():
    import torch
    rows, cols, b = 8, 16, 2
    px = b * rows * cols
    lib = L.lib()
    # one buffer, so that overlapping arguments can be named: disp | out | depth | removed, each region 16-byte aligned
    off = {"disp": 0, "out": 2 * px, "depth": 4 * px, "removed": 8 * px, "end": 8 * px + 16}
    buf = torch.full((off["end"],), 0xA5, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    assert base % 16 == 0
    A = {k: base + v for k, v in off.items()}
    good = api.make_speckle_params()

    def prm(**kw):
        p = api.make_speckle_params()
        for k, v in kw.items():
            setattr(p, k, v)                                    # past make_speckle_params, which would raise
        return p

    with api.Context(0, rows, cols, b) as ctx:
        def call(ctx_h=ctx._h, disp=A["disp"], out=A["out"], depth=A["depth"], r=rows, c=cols, n=b, params=good, removed=A["removed"]):
            return lib.dcmt_filter_speckles_dev(ctx_h, disp, out, depth, r, c, n, ctypes.byref(params) if params is not None else None, removed, None)

        refused = [call(ctx_h=None), call(disp=None), call(out=None), call(params=None), call(disp=None, out=None)]
        refused += [call(r=rows + 1), call(c=cols + 1), call(n=b + 1), call(r=0), call(c=0), call(n=0), call(r=-1), call(n=-1)]
        refused += [call(params=prm(max_size=-1)), call(params=prm(max_size=-2 ** 31)), call(params=prm(max_diff=-1)), call(params=prm(max_diff=65536)),
                    call(params=prm(max_diff=2 ** 31 - 1)), call(params=prm(new_val=-32769)), call(params=prm(new_val=32768)), call(params=prm(new_val=2 ** 31 - 1))]
        refused += [call(disp=A["disp"] + 1), call(out=A["out"] + 1), call(disp=A["disp"] + 1, out=A["disp"] + 1), call(depth=A["depth"] + 1),
                    call(depth=A["depth"] + 2), call(removed=A["removed"] + 1), call(removed=A["removed"] + 2)]
        # overlaps: out over disp other than exactly; depth over either plane; removed over anything
        refused += [call(out=A["disp"] + 2), call(out=A["disp"] + 2 * px - 2), call(disp=A["disp"] + 2), call(depth=A["disp"]), call(depth=A["out"]),
                    call(depth=A["out"] + 2 * px - 4), call(out=A["disp"], depth=A["disp"]), call(disp=A["depth"]), call(out=A["depth"] + 4 * px - 2),
                    call(removed=A["disp"]), call(removed=A["out"] + 2 * px - 4), call(removed=A["depth"]), call(removed=A["depth"] + 4 * px - 4),
                    call(removed=A["disp"] + 4, depth=None), call(out=A["removed"] - 2 * px + 4)]
        assert len(refused) > 40 and all(st == L.E_INVALID for st in refused), refused
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all()), "a refused call wrote something"
        # the same arguments without a fault are taken
        assert call() == L.OK and call(out=A["disp"]) == L.OK and call(depth=None, removed=None) == L.OK
        assert call(params=prm(max_size=0, max_diff=65535, new_val=-32768)) == L.OK and call(params=prm(max_size=2 ** 31 - 1, max_diff=0, new_val=32767)) == L.OK
        assert call(disp=A["disp"] + 2, out=A["disp"] + 2, n=1) == L.OK and call(removed=A["removed"] + 4) == L.OK
        torch.cuda.synchronize()
        assert not bool((buf[off["removed"]:off["removed"] + 8] == 0xA5).all())
    for bad in (dict(max_size=-1), dict(max_diff=65536), dict(new_val=40000)):
        with api.Context(0, rows, cols, b) as ctx, pytest.raises(ValueError):
            ctx.filter_speckles_dev(torch.zeros((b, rows, cols), dtype=torch.int16, device="cuda"), **bad)


@functools.lru_cache(maxsize=None)
def matched(kind, rows, cols, D):
    if kind == "box":
        left, right = G.box_scene(rows, cols, D, 1)[:2]
    elif kind == "shifted":
        left, right = G.shifted_pair(rows, cols, 100 + rows + cols)
    else:
        left, right = G.random_pair(rows, cols, 3)
    kw = dict(baseline=0.5, focal=64.0)
    d16, depth = G.vectorised(left, right, num_disparities=D, **kw)
    for a in (left, right, d16, depth):
        a.setflags(write=False)
    return left, right, d16, depth


@gpu
def test_queued_behind_the_matcher_on_a_stream_without_host_syncs():
    """Behind a delay kernel on a non-default stream, without the host ever waiting: the copy of the real images over decoys, then
    sgm_dev with speckle_window / speckle_range, then sgm_dev -> filter_speckles_dev, then evaluate_dev of the filtered depth.  Both
    routes must be the restatements chained on the CPU -- a kernel that ran early, or on another stream, reads the decoys or an
    unfiltered plane -- and the marker behind the delay must still be pending when the last call returns."""
    import torch
    rows, cols, D = 24, 96, 32
    kinds = ("box", "shifted", "random")
    b = len(kinds)
    kw = dict(baseline=0.5, focal=64.0, num_disparities=D)
    m = [matched(k, rows, cols, D) for k in kinds]
    real_l, real_r = np.stack([x[0] for x in m]), np.stack([x[1] for x in m])
    d16, depth = np.stack([x[2] for x in m]), np.stack([x[3] for x in m])
    want16, want_depth, want_n = expect(d16, depth, max_size=200, max_diff=32)
    assert want_n[2] == (d16[2] != -16).sum() > 100 and want_n[0] == 0 and (want16 != -16).sum() > 1000      # the random pair's blobs all go
    ticks = _ticks_per_ms()
    s = _stream_beside_the_null_stream(ticks)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    gt = dev(np.where(want_depth > 0, want_depth + f32(0.25), 0).astype(f32))
    with api.Context(0, rows, cols, b) as ctx:
        want_eval = host(ctx.evaluate_dev(gt, dev(want_depth)))
        torch.cuda.synchronize()
        decoy_l, decoy_r = dev(real_r[::-1]), dev(real_l[::-1])
        l, r = decoy_l.clone(), decoy_r.clone()
        rl, rr = dev(real_l), dev(real_r)
        a16 = torch.full((b, rows, cols), 0x5A5A, dtype=torch.int16, device="cuda")
        b16, c16 = a16.clone(), a16.clone()
        az = torch.full((b, rows, cols), -7.0, dtype=torch.float32, device="cuda")
        bz = az.clone()
        n = torch.full((b,), -1, dtype=torch.int32, device="cuda")
        ev = torch.full((b, 7), -1.0, dtype=torch.float64, device="cuda")
        work = torch.zeros(2 * one, dtype=torch.uint8, device="cuda")

        def calls():
            ctx.sgm_dev(l, r, d_disp16=a16, d_depth=az, d_work=work, stream=s.cuda_stream, speckle_window=200, speckle_range=2, **kw)
            ctx.sgm_dev(l, r, d_disp16=b16, d_depth=bz, d_work=work, stream=s.cuda_stream, **kw)
            ctx.filter_speckles_dev(b16, d_depth=bz, d_out=c16, d_removed=n, stream=s.cuda_stream)
            ctx.evaluate_dev(gt, bz, d_out=ev, stream=s.cuda_stream)

        torch.cuda.synchronize()
        calls()                                                 # warm-up on the decoys: code objects loaded
        s.synchronize()
        assert not np.array_equal(host(a16), want16)
        t0 = time.perf_counter()
        calls()
        t_call = time.perf_counter() - t0
        s.synchronize()
        for t in (a16, b16, c16):
            t.fill_(0x5A5A)
        az.fill_(-7.0)
        bz.fill_(-7.0)
        torch.cuda.synchronize()
        d_ms = min(1000.0, max(100.0, 20.0 * t_call * 1e3))
        marker = _delayed(s, d_ms, ticks)
        with torch.cuda.stream(s):
            l.copy_(rl)
            r.copy_(rr)
            calls()
            pending = not marker.query()
            got = [t.clone() for t in (a16, az, b16, c16, bz, n, ev)]
            l.copy_(decoy_l)
            r.copy_(decoy_r)
        s.synchronize()
        assert pending, f"the marker behind a {d_ms:.0f} ms delay was complete when the calls returned (t_call {t_call * 1e3:.3f} ms)"
        same(host(got[0]), want16, "sgm_dev with a speckle window: disp16")
        same(host(got[1]), want_depth, "sgm_dev with a speckle window: depth")
        same(host(got[2]), d16, "sgm_dev: disp16 (the filter's source, untouched)")
        same(host(got[3]), want16, "sgm_dev -> filter_speckles_dev: out")
        same(host(got[4]), want_depth, "sgm_dev -> filter_speckles_dev: depth")
        same(host(got[5]).view(np.uint32), want_n, "sgm_dev -> filter_speckles_dev: removed")
        same(host(got[6]), want_eval, "-> evaluate_dev")
        # a window of 0 and no window at all: the matcher alone, no further call
        same(host(ctx.sgm_dev(rl, rr, speckle_window=0, speckle_range=2, **kw)), d16, "speckle_window 0")
        only_depth = ctx.sgm_dev(rl, rr, disp16=False, depth=True, speckle_window=200, speckle_range=2, **kw)
        same(host(only_depth), want_depth, "depth alone with a speckle window")


@gpu
def test_65535_frames_of_8_by_8():
    import torch
    rows = cols = 8
    b = 65535
    pats = np.stack([R.random_plane(rows, cols, 3, 0.7, 11), R.random_plane(rows, cols, 1, 0.9, 12), R.block_plane(rows, cols, 3, 3, 0),
                     np.full((rows, cols), -16, np.int16), R.serpentine(rows, cols, 21), R.serpentine(rows, cols, 20), R.ramp(rows, cols, 16)])
    zpat = R.depth_pattern(pats.shape, 4)
    kw = dict(max_size=20, max_diff=16)
    want, want_z, want_n = expect(pats, zpat, **kw)
    assert want_n.tolist()[3:6] == [0, 0, 20] and want_n[0] > 0
    index = (torch.arange(b, device="cuda") * 5 + 3) % len(pats)             # the last frame is not the first pattern
    v, z = dev(pats)[index], dev(zpat)[index]
    with api.Context(0, rows, cols, b) as ctx:
        for in_place in (False, True):
            src, zz = v.clone(), z.clone()
            out, n = ctx.filter_speckles_dev(src, d_depth=zz, d_out=src if in_place else None, removed=True, **kw)
            torch.cuda.synchronize()
            bad = (out != dev(want)[index]).flatten(1).any(1) | (zz.view(torch.int32) != dev(want_z).view(torch.int32)[index]).flatten(1).any(1) | \
                (n != dev(want_n.view(np.int32))[index])
            assert not bool(bad.any()), f"in_place {in_place}: {int(bad.sum())} frames differ, the first {int(bad.nonzero()[0])}"


@gpu
def test_a_call_whose_scratch_plane_passes_four_gibibytes():
    """4100 frames of 512 x 512: 2^30 + 2^20 * 4 pixels, a scratch plane of 4.3 GB -- frame offsets into the planes, the source and the depth
    are beyond 2^32 bytes (and, in the planes, 2^30 words).  Two frames alternate; every frame is compared on the device."""
    import torch
    rows = cols = 512
    b = 4100
    assert b * rows * cols > 2 ** 30
    need = b * rows * cols * (4 + 4 + 2 + 2 + 4 + 2)            # the context's planes, source, output, depth, a comparison's temporaries
    free, _ = torch.cuda.mem_get_info()
    if free < need * 1.25:
        pytest.skip(f"needs {need / 1e9:.1f} GB + a quarter, {free / 1e9:.1f} GB are free on this device")
    pats = np.stack([R.random_plane(rows, cols, 3, 0.7, 21), R.random_plane(rows, cols, 8, 0.9, 22)])
    zpat = R.depth_pattern(pats.shape, 6)
    kw = dict(max_size=30, max_diff=16)
    want, want_z, want_n = expect(pats, zpat, **kw)
    assert (want_n > 1000).all() and ((want != -16).sum(axis=(1, 2)) > 1000).all()
    dp, dz, dw, dwz = dev(pats), dev(zpat), dev(want), dev(want_z).view(torch.int32)
    src = torch.empty((b, rows, cols), dtype=torch.int16, device="cuda")
    z = torch.empty((b, rows, cols), dtype=torch.float32, device="cuda")
    for k in range(2):
        src[k::2] = dp[k]
        z[k::2] = dz[k]
    with api.Context(0, rows, cols, b) as ctx:
        out, n = ctx.filter_speckles_dev(src, d_depth=z, removed=True, **kw)
        torch.cuda.synchronize()
        for k in range(2):
            bad = (out[k::2] != dw[k]).flatten(1).any(1) | (z[k::2].view(torch.int32) != dwz[k]).flatten(1).any(1) | (n[k::2] != int(want_n[k]))
            assert not bool(bad.any()), f"pattern {k}: {int(bad.sum())} frames differ, the first {2 * int(bad.nonzero()[0]) + k}"
        del out
        out = ctx.filter_speckles_dev(src, d_out=src, **kw)     # in place, no companions
        torch.cuda.synchronize()
        for k in range(2):
            bad = (out[k::2] != dw[k]).flatten(1).any(1)
            assert not bool(bad.any()), f"in place, pattern {k}: {int(bad.sum())} frames differ"


@gpu
def test_host_forms_agree_with_the_device_entry():
    rows, cols = 33, 129
    v = planes(rows, cols)[4]
    depth = R.depth_pattern(v.shape, 8)
    kw = dict(max_size=5, max_diff=16)
    want, want_z, want_n = R.with_depth(R.vectorised, v, depth, **kw)
    with api.Context(0, rows, cols, 1) as ctx:
        out, n = ctx.filter_speckles(v, **kw)
        same(out, want, "host entry: out")
        assert n == want_n > 0
        out, z, n = ctx.filter_speckles(v, depth, **kw)
        same(out, want, "host entry with depth: out")
        same(z, want_z, "host entry with depth: depth")
        assert n == want_n
        wide = np.full((rows, cols + 5), 9, np.int16)           # rows further apart than they need to be
        wide[:, :cols] = v
        same(ctx.filter_speckles(wide[:, :cols], **kw)[0], want, "host entry, padded rows")
        with pytest.raises(ValueError):
            ctx.filter_speckles(v, max_diff=-1)
        # Context.sgm with a window: the matcher's host form, then the filter's
        left, right, d16, dz = matched("random", 24, 96, 32)
        w16, wz, wn = R.with_depth(R.vectorised, d16, dz)
        g16, gz = ctx.sgm(left, right, depth=True, speckle_window=200, speckle_range=2, baseline=0.5, focal=64.0, num_disparities=32)
        same(g16, w16, "Context.sgm with a speckle window: disp16")
        same(gz, wz, "Context.sgm with a speckle window: depth")
    out, n = api.filter_speckles(v, **kw)
    same(out, want, "filter_speckles")
    assert n == want_n
    same(api.filter_speckles(np.where(v == -16, 123, v).astype(np.int16), new_val=123, **kw)[0], np.where(want == -16, 123, want).astype(np.int16),
         "filter_speckles, new_val 123")
    same(api.stereo_sgm(left, right, speckle_window=200, speckle_range=2, num_disparities=32), w16, "stereo_sgm with a speckle window")
    same(api.stereo_sgm(left, right, num_disparities=32), d16, "stereo_sgm without")
