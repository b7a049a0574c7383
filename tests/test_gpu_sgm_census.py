"""The census matching cost on the device: dcmt_sgm_cost_dev / dcmt_sgm_cost, cost= on the Python surface and dcmt_shim::stereo_sgm_cost,
bit for bit against tests/sgm_census_restatement.py (its vectorised form, which tests/test_sgm_census.py holds against the
pixel-by-pixel one without a GPU).  Every output is an integer or an IEEE quotient: every comparison is exact.

Shapes: one pixel, one row, one column, frames narrower than the census window and the box; idle lanes and a second pass of the
staging loop (D = 16 at 70 columns, D = 48 at 65); two disparities a lane (D = 128); the last width of the LDS route and the first
beyond it, without a guide (16 bytes a column: 4096) and with one (18: 3640); the KITTI width.  Every shape runs without a guide and,
in one batch, with an all-zero and a dense guide.  Both volumes are read back from the workspace and compared element for element.
The helpers are those of tests/test_gpu_sgm.py."""
import ctypes
import functools
import os
import subprocess
import time

import numpy as np
import pytest

import sgm_census_restatement as CR
import sgm_guided_restatement as GR
import sgm_restatement as R
import test_gpu_sgm as G
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

gpu = pytest.mark.gpu
dev, host, same = G.dev, G.host, G.same
f32 = np.float32

LDS_PER_COL = 16                                # kSgmLdsPerColCensus: what tests/plan_sgm_census_test.cpp holds the plan to
LDS_LAST = (64 * 1024) // LDS_PER_COL           # 4096
LDS_LAST_GUIDED = (64 * 1024) // (LDS_PER_COL + 2)      # 3640
# (rows, cols, D)
SHAPES = [(1, 1, 64), (1, 9, 64), (9, 1, 64), (3, 3, 16), (6, 6, 64), (7, 19, 64), (16, 70, 16), (9, 65, 48), (11, 130, 128), (24, 257, 64),
          (3, LDS_LAST, 16), (3, LDS_LAST + 1, 16), (3, LDS_LAST_GUIDED, 16), (3, LDS_LAST_GUIDED + 1, 16), (12, 1242, 64)]
VOLUME_SHAPES = [(7, 19, 64), (23, 5, 64), (11, 130, 128)]
VOLUME_KINDS = ("shifted", "quantised", "constant")
LARGEST = {4: 10000, 8: 1800}                   # p2 (and p1) at the limit of the path count


@functools.lru_cache(maxsize=None)
def pair(kind, rows, cols, D):
    if kind == "constant":
        out = CR.constant_pair(rows, cols)
    elif kind == "quantised":
        out = CR.quantised_pair(rows, cols, 100 + rows + cols)
    else:
        return G.pair(kind, rows, cols, D)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dense_guide(rows, cols, D):
    g = GR.guide_kinds(rows, cols, D)["dense"]
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=16)
def volumes(kind, rows, cols, D, paths, p1=200, p2=800, guided=False):
    """(C, S) of one pair, without a guide or with the dense one at the default weight and cap."""
    left, right = pair(kind, rows, cols, D)
    return CR.vectorised_volumes(left, right, dense_guide(rows, cols, D) if guided else None, D, p1, p2, paths)


@functools.lru_cache(maxsize=None)
def reference(kind, rows, cols, D, paths, p1=200, p2=800, guided=False):
    """disp16 of one pair: computed once, shared, read-only."""
    d16 = R.vectorised_select(volumes(kind, rows, cols, D, paths, p1, p2, guided)[1], 10, 1)
    d16.setflags(write=False)
    return d16


def stack(kinds, rows, cols, D):
    lefts, rights = zip(*(pair(k, rows, cols, D) for k in kinds))
    return np.stack(lefts), np.stack(rights)


@gpu
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("rows,cols,D", SHAPES)
def test_shapes_are_the_restatement_bit_for_bit(rows, cols, D, paths):
    left, right = pair("shifted", rows, cols, D)
    plain, guided = reference("shifted", rows, cols, D, paths), reference("shifted", rows, cols, D, paths, guided=True)
    what = f"{rows}x{cols} D {D}, {paths} paths"
    planes = np.stack([np.zeros((rows, cols), f32), dense_guide(rows, cols, D)])
    with api.Context(0, rows, cols, 2) as ctx:
        d16, depth = ctx.sgm_dev(dev(left[None]), dev(right[None]), depth=True, num_disparities=D, paths=paths, cost="census")
        same(host(d16)[0], plain, what + ", no guide: disp16")
        same(host(depth)[0], R.depth_of(plain), what + ", no guide: depth")
        d16, depth = ctx.sgm_dev(dev(np.stack([left] * 2)), dev(np.stack([right] * 2)), depth=True, num_disparities=D, paths=paths, cost="census",
                                 d_guide=dev(planes))
        want = np.stack([plain, guided])
        same(host(d16), want, what + ", an all-zero and a dense guide: disp16")
        same(host(depth), R.depth_of(want), what + ", an all-zero and a dense guide: depth")
    if rows >= 6 and cols >= 19:                                    # the guide matters at this shape
        assert not np.array_equal(plain, guided)


@gpu
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("rows,cols,D", VOLUME_SHAPES)
def test_both_volumes_are_the_restatement_element_for_element(rows, cols, D, paths):
    """C and S as the launches leave them in the caller's workspace, every element, at the default penalties and at the largest the
    path count allows, on the shifted, the four-grey-level and the constant pair; then C' and S with the dense guide.  The workspace
    holds the batch and a frame more, filled with 0xFF; behind the batch's frames it must still hold 0xFF."""
    import torch
    b = len(VOLUME_KINDS)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    lefts, rights = stack(VOLUME_KINDS, rows, cols, D)
    l, r = dev(lefts), dev(rights)
    g = dev(np.stack([dense_guide(rows, cols, D)] * b))
    with api.Context(0, rows, cols, b) as ctx:
        for p1, p2, guided in ((200, 800, False), (LARGEST[paths], LARGEST[paths], False), (200, 800, True)):
            what = f"{rows}x{cols} D {D} {paths} paths p1 {p1} p2 {p2}" + (" dense guide" if guided else "")
            work = torch.full(((b + 1) * one,), 0xFF, dtype=torch.uint8, device="cuda")
            d16 = ctx.sgm_dev(l, r, d_work=work, num_disparities=D, p1=p1, p2=p2, paths=paths, cost="census", d_guide=g if guided else None)
            for f, kind in enumerate(VOLUME_KINDS):
                C, S = G.workspace_volumes(work, f, rows, cols, D)
                wantC, wantS = volumes(kind, rows, cols, D, paths, p1, p2, guided)
                same(C, wantC.astype(np.uint16), f"{what} {kind}: C")
                same(S, wantS.astype(np.uint16), f"{what} {kind}: S")
                same(host(d16)[f], reference(kind, rows, cols, D, paths, p1, p2, guided), f"{what} {kind}: disp16")
            assert bool((work[b * one:] == 0xFF).all()), f"{what}: the workspace was written behind its {b} frames"
    assert not volumes("constant", rows, cols, D, paths)[0].any()                  # C is 0 on the constant pair: S is too
    assert int(volumes("shifted", rows, cols, D, paths)[0].max()) > 2000


@gpu
@pytest.mark.parametrize("paths", [4, 8])
def test_cost_0_through_the_new_entry_point_is_the_old_one(paths):
    """dcmt_sgm_cost_dev with DCMT_SGM_COST_ABSDIFF against dcmt_sgm_guided_dev: disp16, depth and the whole workspace, byte for byte,
    with and without a guide."""
    import torch
    rows, cols, D = 24, 96, 32
    kinds = ("box", "random", "shifted", "comb")
    b = len(kinds)
    lefts, rights = G.stack(kinds, rows, cols, D)
    l, r = dev(lefts), dev(rights)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    p = api.make_sgm_params(num_disparities=D)
    dense = dev(np.stack([dense_guide(rows, cols, D)] * b))
    with api.Context(0, rows, cols, b) as ctx:
        for what, g in (("without a guide", None), ("with a guide", dense)):
            outs = []
            for fill, call in ((0xFF, lambda *a: L.lib().dcmt_sgm_guided_dev(*a[:13], *a[14:])), (0x77, L.lib().dcmt_sgm_cost_dev)):
                work = torch.full((b * one,), fill, dtype=torch.uint8, device="cuda")
                d16 = torch.full((b, rows, cols), 0x5A5A, dtype=torch.int16, device="cuda")
                depth = torch.full((b, rows, cols), -7.0, dtype=torch.float32, device="cuda")
                st = call(ctx._h, l.data_ptr(), r.data_ptr(), g.data_ptr() if g is not None else None, d16.data_ptr(), depth.data_ptr(), rows, cols, b,
                          ctypes.byref(p), paths, 100, 1000, 0, work.data_ptr(), work.numel(), None)
                assert st == L.OK, what
                outs.append((host(d16), host(depth), host(work)))
            same(outs[1][0], outs[0][0], what + ": disp16")
            same(outs[1][1], outs[0][1], what + ": depth")
            same(outs[1][2], outs[0][2], what + ": both volumes of every frame")
            census = host(ctx.sgm_dev(l, r, num_disparities=D, paths=paths, cost="census", d_guide=g))
            assert not np.array_equal(census, outs[0][0])           # and cost 1 is another matcher
        same(host(ctx.sgm_dev(l, r, num_disparities=D, paths=paths, cost="absdiff")), host(ctx.sgm_dev(l, r, num_disparities=D, paths=paths)), "cost='absdiff'")


@gpu
def test_chunks_determinism_and_a_dirty_workspace():
    import torch
    rows, cols, D, b, paths = 24, 96, 32, 5, 8
    left, right = pair("shifted", rows, cols, D)
    kinds = GR.guide_kinds(rows, cols, D)
    names = ("sparse", "dense", "zero", "hostile", "border")
    planes = np.stack([kinds[n] for n in names])
    vols = [CR.vectorised_volumes(left, right, g, D, 200, 800, paths) for g in planes]
    want = np.stack([R.vectorised_select(S, 10, 1) for _, S in vols])
    assert len({w.tobytes() for w in want}) >= 4                   # the frames differ by their guides alone
    l, r, g = dev(np.stack([left] * b)), dev(np.stack([right] * b)), dev(planes)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    with api.Context(0, rows, cols, b) as ctx:
        work = torch.full((2 * one + 8,), 0xFF, dtype=torch.uint8, device="cuda")          # dirty, and a few bytes over
        d16, depth = ctx.sgm_dev(l, r, depth=True, d_work=work, num_disparities=D, paths=paths, d_guide=g, cost="census")
        same(host(d16), want, "batch of 5 through a workspace of 2: disp16")
        same(host(depth), R.depth_of(want), "batch of 5 through a workspace of 2: depth")
        first = host(work)
        again16, again_depth = ctx.sgm_dev(l, r, depth=True, d_work=work, num_disparities=D, paths=paths, d_guide=g, cost="census")
        same(host(again16), host(d16), "second run: disp16")
        same(host(again_depth), host(depth), "second run: depth")
        same(host(work), first, "second run: the workspace")
        for slot, f in ((0, 4), (1, 3)):                            # three chunks: slot 0 ends with frame 4, slot 1 with frame 3
            C, S = G.workspace_volumes(work, slot, rows, cols, D)
            same(C, vols[f][0].astype(np.uint16), f"slot {slot}: C' of frame {f}")
            same(S, vols[f][1].astype(np.uint16), f"slot {slot}: S of frame {f}")
        # without a guide, four paths, through one frame of workspace
        plain = np.stack([reference("shifted", rows, cols, D, 4)] * b)
        small = torch.full((one,), 0xFF, dtype=torch.uint8, device="cuda")
        same(host(ctx.sgm_dev(l, r, d_work=small, num_disparities=D, cost="census")), plain, "batch of 5 through a workspace of 1, no guide")


SHIM_DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_sgm_census_test.cpp")
SHIM_INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv", "with_16s")]


@gpu
def test_host_forms_and_the_shim_agree_with_the_device_entry(tmp_path):
    rows, cols, D, paths = 24, 257, 64, 8
    left, right = pair("shifted", rows, cols, D)
    guide = dense_guide(rows, cols, D)
    want, want_plain4 = reference("shifted", rows, cols, D, paths, guided=True), reference("shifted", rows, cols, D, 4)
    lib = L.lib()
    with api.Context(0, rows, cols, 1) as ctx:
        on_device = host(ctx.sgm_dev(dev(left[None]), dev(right[None]), num_disparities=D, paths=paths, d_guide=dev(guide[None]), cost="census"))[0]
        same(on_device, want, "device entry")
        d16, depth = ctx.sgm(left, right, depth=True, paths=paths, guide=guide, cost="census")
        same(d16, want, "Context.sgm(cost='census', guide=): disp16")
        same(depth, R.depth_of(want), "Context.sgm(cost='census', guide=): depth")
        same(ctx.sgm(left, right, cost="census"), want_plain4, "Context.sgm(cost='census')")
        # the C call itself with padded strides everywhere
        p = api.make_sgm_params()
        wl, wr = np.full((rows, cols + 5), 9, np.uint8), np.full((rows, cols + 7), 9, np.uint8)
        wl[:, :cols], wr[:, :cols] = left, right
        wg = np.full((rows, cols + 3), 7.0, f32)
        wg[:, :cols] = guide
        raw = np.full((rows, cols + 2), 77, np.int16)
        call = lambda cost, g=wg.ctypes.data: lib.dcmt_sgm_cost(ctx._h, wl.ctypes.data, wl.strides[0], wr.ctypes.data, wr.strides[0], g, wg.strides[0], rows, cols,
                                                                ctypes.byref(p), raw.ctypes.data, raw.strides[0], None, 0, paths, 100, 1000, cost)
        assert call(2) == L.E_INVALID and call(-1) == L.E_INVALID and (raw == 77).all()
        assert call(1) == L.OK
        same(raw[:, :cols], want, "dcmt_sgm_cost, padded strides")
        assert (raw[:, cols:] == 77).all()
        assert call(1, None) == L.OK
        same(raw[:, :cols], reference("shifted", rows, cols, D, paths), "dcmt_sgm_cost, no guide")
        with pytest.raises(ValueError):
            ctx.sgm(left, right, cost="Census")
        with pytest.raises(ValueError):
            ctx.sgm_dev(dev(left[None]), dev(right[None]), cost=1)
    same(api.stereo_sgm(left, right, paths=paths, guide=guide, cost="census"), want, "stereo_sgm(cost='census', guide=)")
    same(api.stereo_sgm(left, right, cost="census"), want_plain4, "stereo_sgm(cost='census')")
    # the speckle filter chains behind it: a noise pair, whose map is all speckles
    srows, scols, sD = 24, 96, 32
    sleft, sright = pair("random", srows, scols, sD)
    kw = dict(num_disparities=sD, paths=paths, cost="census")
    plain16, plain_depth = api.stereo_sgm(sleft, sright, depth=True, **kw)
    same(plain16, CR.vectorised(sleft, sright, None, paths, num_disparities=sD)[0], "unfiltered")
    want16, removed = api.filter_speckles(plain16, max_size=200, max_diff=32)
    assert removed > 0
    g16, gz = api.stereo_sgm(sleft, sright, depth=True, speckle_window=200, speckle_range=2, **kw)
    same(g16, want16, "stereo_sgm(cost='census') with a speckle window: disp16")
    same(gz, np.where(want16 != plain16, f32(0), plain_depth), "stereo_sgm(cost='census') with a speckle window: depth")
    with api.Context(0, srows, scols, 1) as ctx:
        d16 = ctx.sgm_dev(dev(sleft[None]), dev(sright[None]), speckle_window=200, speckle_range=2, **kw)
        same(host(d16)[0], want16, "sgm_dev(cost='census') with a speckle window")
    # the shim, through a compiled C++ caller
    for name, a in (("left.u8", left), ("right.u8", right), ("guide.f32", guide)):
        a.tofile(tmp_path / name)
    exe = tmp_path / "shim_sgm_census_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + SHIM_INCLUDES + [SHIM_DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    files = ("left.u8", "right.u8", "guide.f32", "guided8.i16", "plain4.i16")
    run = subprocess.run([str(exe), str(rows), str(cols), str(D)] + [str(tmp_path / f) for f in files], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)
    same(np.fromfile(tmp_path / "guided8.i16", dtype=np.int16).reshape(rows, cols), want, "dcmt_shim::stereo_sgm_cost, a guide, eight paths")
    same(np.fromfile(tmp_path / "plain4.i16", dtype=np.int16).reshape(rows, cols), want_plain4, "dcmt_shim::stereo_sgm_cost, no guide, four paths")


@gpu
def test_every_refusal_returns_invalid_and_writes_nothing():
    import torch
    rows, cols, b, D = 8, 16, 2, 16
    px = b * rows * cols
    lib = L.lib()
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    # one buffer, so that overlapping arguments can be named: left | right | disp16 | depth | guide | work, each region 16-byte aligned
    off = {"left": 0, "right": px, "disp": 2 * px, "depth": 4 * px, "guide": 8 * px, "work": 12 * px, "end": 12 * px + 2 * one}
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
        def call(ctx_h=ctx._h, left=A["left"], right=A["right"], guide=A["guide"], disp=A["disp"], depth=A["depth"], r=rows, c=cols, n=b, params=good,
                 paths=8, weight=100, cap=1000, cost=1, work=A["work"], work_bytes=2 * one):
            return lib.dcmt_sgm_cost_dev(ctx_h, left, right, guide, disp, depth, r, c, n, ctypes.byref(params) if params is not None else None, paths,
                                         weight, cap, cost, work, work_bytes, None)

        # a cost that does not exist, with and without a guide, with either path count
        refused = [call(cost=v) for v in (2, -1, 3, 256, 2 ** 31 - 1, -2 ** 31)] + [call(cost=2, guide=None), call(cost=-1, guide=None, paths=4)]
        # a sample of the older refusals, with census and with absolute differences
        for cost in (1, 0):
            refused += [call(cost=cost, guide=A["guide"] + 2), call(cost=cost, weight=-1), call(cost=cost, weight=10001), call(cost=cost, cap=-1),
                        call(cost=cost, cap=1001), call(cost=cost, paths=4, cap=9201), call(cost=cost, params=prm(p2=801)),
                        call(cost=cost, depth=None, params=prm(baseline=np.nan)), call(cost=cost, guide=A["disp"]), call(cost=cost, guide=A["work"]),
                        call(cost=cost, paths=5), call(cost=cost, params=prm(p2=1801), cap=0), call(cost=cost, ctx_h=None), call(cost=cost, left=None),
                        call(cost=cost, disp=None, depth=None), call(cost=cost, params=None), call(cost=cost, work=None),
                        call(cost=cost, params=prm(num_disparities=24)), call(cost=cost, params=prm(p1=801)), call(cost=cost, params=prm(uniqueness=101)),
                        call(cost=cost, params=prm(max_depth=-1.0)), call(cost=cost, disp=A["disp"] + 1), call(cost=cost, work=A["work"] + 8),
                        call(cost=cost, work_bytes=one - 1), call(cost=cost, r=rows + 1), call(cost=cost, n=b + 1), call(cost=cost, disp=A["left"]),
                        call(cost=cost, disp=A["work"])]
        assert len(refused) > 60 and all(st == L.E_INVALID for st in refused), refused
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all()), "a refused call wrote something"
        # the same arguments with cost 1 are taken (the guide's 0xA5 bytes are negative floats: no hints, which is fine)
        assert call() == L.OK and call(paths=4, cap=9200) == L.OK and call(guide=None, weight=-1, cap=-1) == L.OK and call(guide=None, paths=4) == L.OK
        assert call(cost=0) == L.OK and call(depth=None, params=prm(max_depth=np.nan)) == L.OK and call(disp=None) == L.OK and call(work_bytes=one) == L.OK
        torch.cuda.synchronize()
        assert not bool((buf[off["disp"]:off["guide"]] == 0xA5).all())
        assert bool((buf[:off["disp"]] == 0xA5).all()) and bool((buf[off["guide"]:off["work"]] == 0xA5).all()), "a call wrote to its inputs"


@gpu
def test_grey_conversion_then_census_matching_on_a_stream_without_host_syncs():
    """bgr_convert_dev (grey) -> sgm_dev(cost="census") behind a delay kernel on a non-default stream, as tests/test_gpu_sgm_guided.py
    queues the guided matcher: the copies of the real frames over decoys, the three calls, clones of the outputs and the restoring of
    the decoys are enqueued without the host ever waiting.  The clones must be the real inputs' results, and the marker behind the
    delay must still be pending when the chain has been enqueued."""
    import torch
    rows, cols, D, b, paths = 24, 96, 32, 3, 8
    rng = np.random.default_rng(9)

    def colour(grey):
        """BGR frames whose three channels differ: the grey value of the conversion is not any one of them"""
        out = np.stack([grey, grey, grey], axis=-1).astype(np.int32) + rng.integers(-20, 21, grey.shape + (3,))
        return np.clip(out, 0, 255).astype(np.uint8)

    real = [colour(a) for a in G.stack(("box", "shifted", "random"), rows, cols, D)]
    decoy = [colour(a) for a in G.stack(("random", "same", "box"), rows, cols, D)[::-1]]
    ticks = G._ticks_per_ms()
    s = G._stream_beside_the_null_stream(ticks)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    with api.Context(0, rows, cols, b) as ctx:
        want_grey = [host(ctx.bgr_convert_dev(dev(a), lab=False, gray=True)) for a in real]        # tested elsewhere: the grey planes as they are
        want = np.stack([CR.vectorised(want_grey[0][f], want_grey[1][f], None, paths, num_disparities=D)[0] for f in range(b)])
        assert (want >= 0).mean() > 0.2
        decoy_l, decoy_r = dev(decoy[0]), dev(decoy[1])
        bl, br = decoy_l.clone(), decoy_r.clone()
        real_l, real_r = dev(real[0]), dev(real[1])
        gl = torch.full((b, rows, cols), 0x33, dtype=torch.uint8, device="cuda")
        gr = torch.full((b, rows, cols), 0x44, dtype=torch.uint8, device="cuda")
        d16 = torch.full((b, rows, cols), 0x5A5A, dtype=torch.int16, device="cuda")
        depth = torch.full((b, rows, cols), -7.0, dtype=torch.float32, device="cuda")
        work = torch.zeros(2 * one, dtype=torch.uint8, device="cuda")

        def chain():
            ctx.bgr_convert_dev(bl, lab=False, d_gray=gl, stream=s.cuda_stream)
            ctx.bgr_convert_dev(br, lab=False, d_gray=gr, stream=s.cuda_stream)
            ctx.sgm_dev(gl, gr, d_disp16=d16, d_depth=depth, d_work=work, stream=s.cuda_stream, num_disparities=D, paths=paths, cost="census")

        torch.cuda.synchronize()
        chain()                                                 # warm-up on the decoys: code objects loaded
        s.synchronize()
        assert not np.array_equal(host(d16), want)
        t0 = time.perf_counter()
        chain()
        t_call = time.perf_counter() - t0
        s.synchronize()
        d16.fill_(0x5A5A)
        depth.fill_(-7.0)
        gl.fill_(0x33)
        gr.fill_(0x44)
        torch.cuda.synchronize()
        d_ms = min(1000.0, max(100.0, 20.0 * t_call * 1e3))
        marker = G._delayed(s, d_ms, ticks)
        with torch.cuda.stream(s):
            bl.copy_(real_l)
            br.copy_(real_r)
            chain()
            pending = not marker.query()
            got16, got_depth, got_l, got_r = d16.clone(), depth.clone(), gl.clone(), gr.clone()
            bl.copy_(decoy_l)
            br.copy_(decoy_r)
        s.synchronize()
        assert pending, f"the marker behind a {d_ms:.0f} ms delay was complete when the chain returned (t_call {t_call * 1e3:.3f} ms)"
        same(host(got_l), want_grey[0], "behind the delay: the left grey plane")
        same(host(got_r), want_grey[1], "behind the delay: the right grey plane")
        same(host(got16), want, "behind the delay: disp16")
        same(host(got_depth), R.depth_of(want), "behind the delay: depth")
