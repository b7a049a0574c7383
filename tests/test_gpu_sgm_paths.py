"""Eight-path aggregation on the device: dcmt_sgm_paths_dev / dcmt_sgm_paths and paths=8 on the Python surface, bit for bit against
tests/sgm_paths_restatement.py (its vectorised form, which tests/test_sgm_paths.py holds against the pixel-by-pixel one without a GPU).
Every output is an integer or an IEEE quotient of integers: every comparison is exact.

Shapes: where the wrapped walk of k_sgm_diag can go wrong -- one pixel, one row (every walk is one pixel), one column (every pixel
restarts), 2 x 2 and 5 x 2 (a wrap that moves the column by one), a square, more columns than rows, 23 x 5 (several wraps a wave),
idle lanes (D = 16, 48), two disparities a lane (D = 128), a width that is no multiple of the waves of a workgroup, 4097 columns and
the KITTI width.  Both volumes are read back from the workspace and compared element for element.  The helpers are those of
tests/test_gpu_sgm.py."""
import ctypes
import functools
import time

import numpy as np
import pytest

import sgm_paths_restatement as P
import sgm_restatement as R
import test_gpu_sgm as G
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

gpu = pytest.mark.gpu
dev, host, same, pair, stack = G.dev, G.host, G.same, G.pair, G.stack

# (rows, cols, D)
SHAPES = [(1, 1, 64), (1, 9, 64), (9, 1, 64), (2, 2, 64), (5, 2, 64), (6, 6, 64), (7, 19, 64), (23, 5, 64), (16, 70, 16), (9, 65, 48), (11, 130, 128),
          (24, 257, 64), (3, 4097, 16), (12, 1242, 64)]
PENALTIES = [(0, 0), (200, 800), (1800, 1800), (0, 1800)]
VOLUME_SHAPES = [(7, 19, 64), (23, 5, 64), (11, 130, 128)]


@functools.lru_cache(maxsize=8)
def volumes(kind, rows, cols, D, seed=0, p1=200, p2=800, paths=8):
    return P.vectorised_volumes(*pair(kind, rows, cols, D, seed), D, p1, p2, paths)


@functools.lru_cache(maxsize=None)
def reference(kind, rows, cols, D, seed=0, p1=200, p2=800, uniqueness=10, disp12_max_diff=1, paths=8):
    """disp16 of one pair: computed once, shared, read-only."""
    d16 = R.vectorised_select(volumes(kind, rows, cols, D, seed, p1, p2, paths)[1], uniqueness, disp12_max_diff)
    d16.setflags(write=False)
    return d16


def raw_paths_dev(ctx, l, r, d16, depth, work, params, paths, stream=None):
    """dcmt_sgm_paths_dev itself, with nothing of the Python surface in front of it."""
    b, rows, cols = l.shape
    return L.lib().dcmt_sgm_paths_dev(ctx._h, l.data_ptr(), r.data_ptr(), d16.data_ptr() if d16 is not None else None,
                                      depth.data_ptr() if depth is not None else None, rows, cols, b, ctypes.byref(params), paths,
                                      work.data_ptr(), work.numel(), stream)


@gpu
@pytest.mark.parametrize("rows,cols,D", SHAPES)
def test_shapes_are_the_restatement_bit_for_bit(rows, cols, D):
    kinds = ("shifted", "random", "same")
    lefts, rights = stack(kinds, rows, cols, D)
    want = np.stack([reference(k, rows, cols, D) for k in kinds])
    what = f"{rows}x{cols} D {D}, eight paths"
    with api.Context(0, rows, cols, len(kinds)) as ctx:
        d16, depth = ctx.sgm_dev(dev(lefts), dev(rights), depth=True, num_disparities=D, paths=8)
        same(host(d16), want, what + ": disp16")
        same(host(depth), R.depth_of(want), what + ": depth")
    if cols > 2 * 8 and rows >= 7:
        assert (np.abs(want[0][:, 8:-4] - 48) <= 8).mean() > 0.8, what        # the reference itself: 3 px found


@gpu
@pytest.mark.parametrize("rows,cols,D", VOLUME_SHAPES)
def test_both_volumes_are_the_restatement_element_for_element(rows, cols, D):
    """C and S as the five launches leave them in the caller's workspace, every element, over the penalty grid, the comb among the
    inputs.  The workspace holds the batch and a frame more, filled with 0xFF; behind the batch's frames it must still hold 0xFF."""
    import torch
    kinds = ("shifted", "random", "comb")
    b = len(kinds)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    lefts, rights = stack(kinds, rows, cols, D)
    l, r = dev(lefts), dev(rights)
    with api.Context(0, rows, cols, b) as ctx:
        for p1, p2 in PENALTIES:
            work = torch.full(((b + 1) * one,), 0xFF, dtype=torch.uint8, device="cuda")
            d16 = ctx.sgm_dev(l, r, d_work=work, num_disparities=D, p1=p1, p2=p2, paths=8)
            for f, kind in enumerate(kinds):
                C, S = G.workspace_volumes(work, f, rows, cols, D)
                wantC, wantS = volumes(kind, rows, cols, D, 0, p1, p2)
                same(C, wantC.astype(np.uint16), f"{rows}x{cols} D {D} p1 {p1} p2 {p2} {kind}: C")
                same(S, wantS.astype(np.uint16), f"{rows}x{cols} D {D} p1 {p1} p2 {p2} {kind}: S")
                if p2 == 0:
                    assert np.array_equal(wantS, 8 * wantC)
            assert bool((work[b * one:] == 0xFF).all()), f"{rows}x{cols} D {D}: the workspace was written behind its {b} frames"
            same(host(d16), np.stack([reference(k, rows, cols, D, 0, p1, p2) for k in kinds]), f"{rows}x{cols} D {D} p1 {p1} p2 {p2}: disp16")


@gpu
def test_the_bound_is_attained_on_the_device():
    """comb_pair(12, 3 D, D) with p1 = p2 = 1800: S reaches 65400 (tests/test_sgm_paths.py), and the device holds it in uint16."""
    import torch
    rows, D = 12, 16
    cols = 3 * D
    left, right = pair("comb", rows, cols, D)
    wantC, wantS = volumes("comb", rows, cols, D, 0, 1800, 1800)
    assert int(wantS.max()) == 65400
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    work = torch.full((one,), 0xFF, dtype=torch.uint8, device="cuda")
    with api.Context(0, rows, cols, 1) as ctx:
        d16 = ctx.sgm_dev(dev(left[None]), dev(right[None]), d_work=work, num_disparities=D, p1=1800, p2=1800, paths=8)
    C, S = G.workspace_volumes(work, 0, rows, cols, D)
    same(S, wantS.astype(np.uint16), "the comb at the bound: S")
    same(host(d16)[0], reference("comb", rows, cols, D, 0, 1800, 1800), "the comb at the bound: disp16")


@gpu
def test_four_paths_through_the_new_entry_point_are_the_old_entry_point():
    import torch
    rows, cols, D = 24, 96, 32
    kinds = ("box", "random", "shifted", "comb")
    b = len(kinds)
    lefts, rights = stack(kinds, rows, cols, D)
    l, r = dev(lefts), dev(rights)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    p = api.make_sgm_params(num_disparities=D)
    with api.Context(0, rows, cols, b) as ctx:
        old_work = torch.full((b * one,), 0xFF, dtype=torch.uint8, device="cuda")
        old16, old_depth = ctx.sgm_dev(l, r, depth=True, d_work=old_work, num_disparities=D)
        new_work = torch.full((b * one,), 0x77, dtype=torch.uint8, device="cuda")
        new16 = torch.full((b, rows, cols), 0x5A5A, dtype=torch.int16, device="cuda")
        new_depth = torch.full((b, rows, cols), -7.0, dtype=torch.float32, device="cuda")
        assert raw_paths_dev(ctx, l, r, new16, new_depth, new_work, p, 4) == L.OK
        same(host(new16), host(old16), "paths = 4: disp16")
        same(host(new_depth), host(old_depth), "paths = 4: depth")
        same(host(new_work), host(old_work), "paths = 4: both volumes of every frame")
        same(host(old16), np.stack([G.reference(k, rows, cols, D) for k in kinds]), "dcmt_sgm_dev: the four-path restatement")
        same(host(ctx.sgm_dev(l, r, num_disparities=D, paths=4)), host(old16), "sgm_dev(paths=4)")


@gpu
def test_the_paths_are_honoured():
    rows, cols, D = 24, 64, 16
    left, right = pair("box", rows, cols, D, 1)
    want8, want4 = reference("box", rows, cols, D, 1), G.reference("box", rows, cols, D, 1)
    assert np.array_equal(want4, reference("box", rows, cols, D, 1, paths=4))
    differ = int((want8 != want4).sum())
    print(f"box_scene(24, 64, 16, seed=1): the restatements with four and eight paths differ on {differ} pixels")
    assert differ == 19
    with api.Context(0, rows, cols, 1) as ctx:
        got8 = host(ctx.sgm_dev(dev(left[None]), dev(right[None]), num_disparities=D, paths=8))[0]
        got4 = host(ctx.sgm_dev(dev(left[None]), dev(right[None]), num_disparities=D, paths=4))[0]
    same(got8, want8, "paths = 8")
    same(got4, want4, "paths = 4")
    assert int((got8 != got4).sum()) == differ


@gpu
def test_chunks_determinism_and_a_dirty_workspace():
    import torch
    rows, cols, D, b = 24, 96, 32, 5
    kinds = ("box", "random", "shifted", "same", "comb")
    lefts, rights = stack(kinds, rows, cols, D)
    l, r = dev(lefts), dev(rights)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    with api.Context(0, rows, cols, b) as ctx:
        alone = np.stack([host(ctx.sgm_dev(l[f:f + 1], r[f:f + 1], num_disparities=D, paths=8))[0] for f in range(b)])
        same(alone, np.stack([reference(k, rows, cols, D) for k in kinds]), "one frame at a time")
        work = torch.full((2 * one + 8,), 0xFF, dtype=torch.uint8, device="cuda")          # dirty, and a few bytes over
        d16, depth = ctx.sgm_dev(l, r, depth=True, d_work=work, num_disparities=D, paths=8)
        same(host(d16), alone, "batch of 5 through a workspace of 2: disp16")
        same(host(depth), R.depth_of(alone), "batch of 5 through a workspace of 2: depth")
        first = host(work)
        again16, again_depth = ctx.sgm_dev(l, r, depth=True, d_work=work, num_disparities=D, paths=8)
        same(host(again16), host(d16), "second run: disp16")
        same(host(again_depth), host(depth), "second run: depth")
        same(host(work), first, "second run: the workspace")
        # three chunks: slot 0 ends with the volumes of frame 4, slot 1 with those of frame 3
        for slot, f in ((0, 4), (1, 3)):
            C, S = G.workspace_volumes(work, slot, rows, cols, D)
            wantC, wantS = volumes(kinds[f], rows, cols, D)
            same(C, wantC.astype(np.uint16), f"slot {slot}: C of frame {f}")
            same(S, wantS.astype(np.uint16), f"slot {slot}: S of frame {f}")


@gpu
def test_host_forms_agree_with_the_device_entry():
    rows, cols, D = 24, 257, 64
    left, right = pair("shifted", rows, cols, D)
    want = reference("shifted", rows, cols, D)
    lib = L.lib()
    with api.Context(0, rows, cols, 1) as ctx:
        on_device = host(ctx.sgm_dev(dev(left[None]), dev(right[None]), num_disparities=D, paths=8))[0]
        same(on_device, want, "device entry")
        d16, depth = ctx.sgm(left, right, depth=True, paths=8)
        same(d16, on_device, "Context.sgm(paths=8): disp16")
        same(depth, R.depth_of(want), "Context.sgm(paths=8): depth")
        same(ctx.sgm(left, right, disp16=False, depth=True, max_depth=20.0, paths=8), R.depth_of(want, max_depth=20.0), "Context.sgm(paths=8): depth alone")
        wide = np.full((rows, cols + 5), 9, np.uint8)          # rows further apart than they need to be
        wide[:, :cols] = left
        same(ctx.sgm(wide[:, :cols], right, paths=8), want, "Context.sgm(paths=8), padded rows")
        # the C call itself: eight, four, and what it refuses
        p = api.make_sgm_params()
        raw = np.full((rows, cols), 77, np.int16)
        call = lambda params, paths: lib.dcmt_sgm_paths(ctx._h, left.ctypes.data, cols, right.ctypes.data, cols, rows, cols, ctypes.byref(params),
                                                        raw.ctypes.data, 2 * cols, None, 0, paths)
        for paths in (0, 5, 16):
            assert call(p, paths) == L.E_INVALID
        steep = api.make_sgm_params(p2=1801)
        assert call(steep, 8) == L.E_INVALID and (raw == 77).all()
        assert call(p, 8) == L.OK
        same(raw, want, "dcmt_sgm_paths, 8")
        assert call(steep, 4) == L.OK
        same(raw, G.reference("shifted", rows, cols, D, 0, 200, 1801), "dcmt_sgm_paths, 4, p2 = 1801")
        same(ctx.sgm(left, right), G.reference("shifted", rows, cols, D), "Context.sgm without the keyword: four paths")
        with pytest.raises(ValueError):
            ctx.sgm(left, right, paths=8, p2=1801)
        with pytest.raises(ValueError):
            ctx.sgm(left, right, paths=5)
        with pytest.raises(ValueError):
            ctx.sgm_dev(dev(left[None]), dev(right[None]), paths=8, p2=1801)
        with pytest.raises(ValueError):
            ctx.sgm_dev(dev(left[None]), dev(right[None]), paths=16)
    same(api.stereo_sgm(left, right, paths=8), want, "stereo_sgm(paths=8)")
    d16, depth = api.stereo_sgm(left, right, depth=True, uniqueness=0, disp12_max_diff=-1, paths=8)
    loose = reference("shifted", rows, cols, D, 0, 200, 800, 0, -1)
    same(d16, loose, "stereo_sgm(paths=8), no checks: disp16")
    same(depth, R.depth_of(loose), "stereo_sgm(paths=8), no checks: depth")


@gpu
def test_the_speckle_filter_chains_behind_eight_paths():
    rows, cols, D = 24, 96, 32
    kw = dict(num_disparities=D, baseline=0.5, focal=64.0, paths=8)
    left, right = pair("random", rows, cols, D)
    plain16, plain_depth = api.stereo_sgm(left, right, depth=True, **kw)
    same(plain16, reference("random", rows, cols, D), "unfiltered")
    want16, removed = api.filter_speckles(plain16, max_size=200, max_diff=32)
    assert removed > 0
    want_depth = np.where(want16 != plain16, np.float32(0), plain_depth)
    g16, gz = api.stereo_sgm(left, right, depth=True, speckle_window=200, speckle_range=2, **kw)
    same(g16, want16, "stereo_sgm(paths=8) with a speckle window: disp16")
    same(gz, want_depth, "stereo_sgm(paths=8) with a speckle window: depth")
    with api.Context(0, rows, cols, 1) as ctx:
        d16, dz = ctx.sgm_dev(dev(left[None]), dev(right[None]), depth=True, speckle_window=200, speckle_range=2, **kw)
        same(host(d16)[0], want16, "sgm_dev(paths=8) with a speckle window: disp16")
        same(host(dz)[0], want_depth, "sgm_dev(paths=8) with a speckle window: depth")


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
        def call(ctx_h=ctx._h, left=A["left"], right=A["right"], disp=A["disp"], depth=A["depth"], r=rows, c=cols, n=b, params=good, paths=8,
                 work=A["work"], work_bytes=2 * one):
            return lib.dcmt_sgm_paths_dev(ctx_h, left, right, disp, depth, r, c, n, ctypes.byref(params) if params is not None else None, paths, work,
                                          work_bytes, None)

        refused = [call(paths=v) for v in (0, 5, 16, -8, 1, 2, 3, 7, 12, 1 << 20)]
        refused += [call(params=prm(p2=1801)), call(params=prm(p1=1801, p2=1801)), call(params=prm(p2=10000)), call(paths=4, params=prm(p2=10001))]
        # the refusals of dcmt_sgm_dev, once each
        refused += [call(ctx_h=None), call(left=None), call(right=None), call(disp=None, depth=None), call(params=None), call(work=None)]
        refused += [call(params=prm(num_disparities=24)), call(params=prm(p1=-1)), call(params=prm(p1=801)), call(params=prm(uniqueness=101)),
                    call(params=prm(baseline=np.nan)), call(params=prm(focal=0.0)), call(params=prm(max_depth=-1.0))]
        refused += [call(disp=A["disp"] + 1), call(depth=A["depth"] + 2), call(work=A["work"] + 8), call(work_bytes=one - 1)]
        refused += [call(r=rows + 1), call(c=cols + 1), call(n=b + 1), call(r=0)]
        refused += [call(disp=A["left"]), call(depth=A["right"] + px - 4), call(disp=A["depth"]), call(disp=A["work"]), call(work=A["left"], work_bytes=one)]
        assert len(refused) > 35 and all(st == L.E_INVALID for st in refused), refused
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all()), "a refused call wrote something"
        # the same arguments without a fault are taken
        assert call() == L.OK and call(params=prm(p1=1800, p2=1800)) == L.OK and call(paths=4, params=prm(p2=1801)) == L.OK and call(disp=None) == L.OK
        assert call(work_bytes=one) == L.OK
        torch.cuda.synchronize()
        assert not bool((buf[off["disp"]:off["work"]] == 0xA5).all())
        assert bool((buf[:off["disp"]] == 0xA5).all()), "a call wrote to its inputs"


@gpu
def test_queued_on_a_stream_behind_pending_work_without_host_syncs():
    """As tests/test_gpu_sgm.py does it for the four-path call: behind a delay kernel on a non-default stream, the copy of the real
    inputs over decoys, the call (two chunks, five launches each), clones of the outputs and the restoring of the decoys are enqueued
    without the host ever waiting.  The clones must be the real inputs' bits, and the marker behind the delay must still be pending
    when the call returns."""
    import torch
    rows, cols, D, b = 24, 96, 32, 3
    real = stack(("box", "shifted", "random"), rows, cols, D)
    decoy = stack(("random", "same", "box"), rows, cols, D)[::-1]          # other images, left and right swapped
    want = np.stack([reference(k, rows, cols, D) for k in ("box", "shifted", "random")])
    ticks = G._ticks_per_ms()
    s = G._stream_beside_the_null_stream(ticks)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    with api.Context(0, rows, cols, b) as ctx:
        decoy_l, decoy_r = dev(decoy[0]), dev(decoy[1])
        l, r = decoy_l.clone(), decoy_r.clone()
        real_l, real_r = dev(real[0]), dev(real[1])
        d16 = torch.full((b, rows, cols), 0x5A5A, dtype=torch.int16, device="cuda")
        depth = torch.full((b, rows, cols), -7.0, dtype=torch.float32, device="cuda")
        work = torch.zeros(2 * one, dtype=torch.uint8, device="cuda")
        call = lambda: ctx.sgm_dev(l, r, d_disp16=d16, d_depth=depth, d_work=work, stream=s.cuda_stream, num_disparities=D, paths=8)
        torch.cuda.synchronize()
        call()                                                  # warm-up on the decoys: code objects loaded
        s.synchronize()
        assert not np.array_equal(host(d16), want)
        t0 = time.perf_counter()
        call()
        t_call = time.perf_counter() - t0
        s.synchronize()
        d16.fill_(0x5A5A)
        depth.fill_(-7.0)
        torch.cuda.synchronize()
        d_ms = min(1000.0, max(100.0, 20.0 * t_call * 1e3))
        marker = G._delayed(s, d_ms, ticks)
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
