"""LiDAR-guided stereo matching on the device: dcmt_sgm_guided_dev / dcmt_sgm_guided, d_guide= / guide= on the Python surface and
dcmt_shim::stereo_sgm_guided, bit for bit against tests/sgm_guided_restatement.py (its vectorised form, which tests/test_sgm_guided.py
holds against the pixel-by-pixel one without a GPU).  Every output is an integer or an IEEE quotient: every comparison is exact.

Shapes: one pixel, one row, one column, small frames; idle lanes and a second pass of the staging loop (D = 16 at 70 columns, D = 48
at 65); two disparities a lane (D = 128); the last width of the guided LDS route (18 bytes a column: 3640) and the first beyond it;
4097 columns, beyond the unguided route too; the KITTI width.  Every guide kind of sgm_guided_restatement.guide_kinds rides in one
batch.  Both volumes are read back from the workspace and compared element for element.  The helpers are those of
tests/test_gpu_sgm.py."""
import ctypes
import functools
import os
import subprocess
import time

import numpy as np
import pytest

import sgm_guided_restatement as GR
import sgm_paths_restatement as P
import sgm_restatement as R
import test_gpu_sgm as G
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

gpu = pytest.mark.gpu
dev, host, same, pair = G.dev, G.host, G.same, G.pair
f32 = np.float32

LDS_LAST = (64 * 1024) // 18                    # 3640: what tests/plan_sgm_guided_test.cpp holds the plan to
# (rows, cols, D)
SHAPES = [(1, 1, 64), (1, 9, 64), (9, 1, 64), (6, 6, 64), (7, 19, 64), (16, 70, 16), (9, 65, 48), (11, 130, 128), (24, 257, 64),
          (3, LDS_LAST, 16), (3, LDS_LAST + 1, 16), (3, 4097, 16), (12, 1242, 64)]
VOLUME_SHAPES = [(7, 19, 64), (23, 5, 64), (11, 130, 128)]
# (p1, p2, weight, cap) per path count: nothing, the defaults, a cap that binds at once, the largest sum
GRID = {4: [(200, 800, 0, 0), (200, 800, 100, 1000), (200, 800, 1000, 100), (5000, 5000, 5000, 5000)],
        8: [(200, 800, 0, 0), (200, 800, 100, 1000), (200, 800, 1000, 100), (900, 900, 900, 900)]}


@functools.lru_cache(maxsize=None)
def guides(rows, cols, D):
    """(names, f32 [kinds][rows][cols]): every guide kind, for the "shifted" pair of the shape; read-only."""
    kinds = GR.guide_kinds(rows, cols, D)
    names = tuple(kinds) if rows * cols * D <= 400_000 else ("sparse", "dense", "hostile")        # a few seconds a case
    planes = np.stack([kinds[n] for n in names])
    planes.setflags(write=False)
    return names, planes


@functools.lru_cache(maxsize=16)
def volumes(rows, cols, D, paths, p1=200, p2=800, weight=100, cap=1000, kind="shifted"):
    """[(C', S)] per guide kind of guides(rows, cols, D)."""
    left, right = pair(kind, rows, cols, D)
    return [GR.vectorised_volumes(left, right, g, D, p1, p2, paths, weight, cap) for g in guides(rows, cols, D)[1]]


@functools.lru_cache(maxsize=None)
def reference(rows, cols, D, paths, p1=200, p2=800, weight=100, cap=1000, kind="shifted"):
    """disp16 [kinds][rows][cols]: computed once, shared, read-only."""
    d16 = np.stack([R.vectorised_select(S, 10, 1) for _, S in volumes(rows, cols, D, paths, p1, p2, weight, cap, kind)])
    d16.setflags(write=False)
    return d16


def repeated(kind, rows, cols, D, n):
    left, right = pair(kind, rows, cols, D)
    return np.stack([left] * n), np.stack([right] * n)


def raw_guided_dev(ctx, l, r, g, d16, depth, work, params, paths, weight, cap, stream=None):
    """dcmt_sgm_guided_dev itself, with nothing of the Python surface in front of it."""
    b, rows, cols = l.shape
    return L.lib().dcmt_sgm_guided_dev(ctx._h, l.data_ptr(), r.data_ptr(), g.data_ptr() if g is not None else None,
                                       d16.data_ptr() if d16 is not None else None, depth.data_ptr() if depth is not None else None, rows, cols, b,
                                       ctypes.byref(params), paths, weight, cap, work.data_ptr(), work.numel(), stream)


@gpu
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("rows,cols,D", SHAPES)
def test_shapes_are_the_restatement_bit_for_bit(rows, cols, D, paths):
    names, planes = guides(rows, cols, D)
    lefts, rights = repeated("shifted", rows, cols, D, len(names))
    want = reference(rows, cols, D, paths)
    what = f"{rows}x{cols} D {D}, {paths} paths, guides {names}"
    with api.Context(0, rows, cols, len(names)) as ctx:
        d16, depth = ctx.sgm_dev(dev(lefts), dev(rights), depth=True, num_disparities=D, paths=paths, d_guide=dev(planes))
        same(host(d16), want, what + ": disp16")
        same(host(depth), R.depth_of(want), what + ": depth")
    if "zero" in names:                                             # the all-zero guide: the unguided restatement
        unguided = (P.vectorised if paths == 8 else R.vectorised)(*pair("shifted", rows, cols, D), num_disparities=D)[0]
        assert np.array_equal(want[names.index("zero")], unguided)
    if rows >= 6 and cols >= 19:                                    # the guides matter at this shape
        assert not np.array_equal(want[names.index("dense")], want[names.index("sparse")])


@gpu
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("rows,cols,D", VOLUME_SHAPES)
def test_both_volumes_are_the_restatement_element_for_element(rows, cols, D, paths):
    """C' and S as the launches leave them in the caller's workspace, every element, over the weight / cap grid.  The workspace holds
    the batch and a frame more, filled with 0xFF; behind the batch's frames it must still hold 0xFF."""
    import torch
    names, planes = guides(rows, cols, D)
    b = len(names)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    lefts, rights = repeated("shifted", rows, cols, D, b)
    l, r, g = dev(lefts), dev(rights), dev(planes)
    with api.Context(0, rows, cols, b) as ctx:
        for p1, p2, weight, cap in GRID[paths]:
            what = f"{rows}x{cols} D {D} {paths} paths p1 {p1} p2 {p2} weight {weight} cap {cap}"
            work = torch.full(((b + 1) * one,), 0xFF, dtype=torch.uint8, device="cuda")
            d16 = ctx.sgm_dev(l, r, d_work=work, num_disparities=D, p1=p1, p2=p2, paths=paths, d_guide=g, guide_weight=weight, guide_cap=cap)
            want = volumes(rows, cols, D, paths, p1, p2, weight, cap)
            for f, name in enumerate(names):
                C, S = G.workspace_volumes(work, f, rows, cols, D)
                same(C, want[f][0].astype(np.uint16), f"{what} {name}: C'")
                same(S, want[f][1].astype(np.uint16), f"{what} {name}: S")
            assert bool((work[b * one:] == 0xFF).all()), f"{what}: the workspace was written behind its {b} frames"
            same(host(d16), reference(rows, cols, D, paths, p1, p2, weight, cap), what + ": disp16")
            if weight == 0:                                         # bit for bit the unguided volumes
                plain = (P.vectorised_volumes(*pair("shifted", rows, cols, D), D, p1, p2, paths))
                assert all(np.array_equal(w[0], plain[0]) and np.array_equal(w[1], plain[1]) for w in want)


@gpu
@pytest.mark.parametrize("paths,penalty,bound", [(4, 5000, 65500), (8, 900, 65400)])
def test_the_comb_at_the_bound_on_the_device(paths, penalty, bound):
    """comb_pair(12, 48, 16), a hint of 0 on every pixel, weight = cap = p1 = p2: S reaches the bound (tests/test_sgm_guided.py), and
    the device holds it in uint16."""
    import torch
    rows, cols, D = 12, 48, 16
    left, right = pair("comb", rows, cols, D)
    guide = np.full((rows, cols), GR.FAR, f32)
    wantC, wantS = GR.vectorised_volumes(left, right, guide, D, penalty, penalty, paths, penalty, penalty)
    assert int(wantS.max()) == bound
    work = torch.full((api.sgm_workspace_bytes(rows, cols, D, 1),), 0xFF, dtype=torch.uint8, device="cuda")
    with api.Context(0, rows, cols, 1) as ctx:
        d16 = ctx.sgm_dev(dev(left[None]), dev(right[None]), d_work=work, num_disparities=D, p1=penalty, p2=penalty, paths=paths,
                          d_guide=dev(guide[None]), guide_weight=penalty, guide_cap=penalty)
    C, S = G.workspace_volumes(work, 0, rows, cols, D)
    assert int(S.max()) == bound
    same(C, wantC.astype(np.uint16), "the comb at the bound: C'")
    same(S, wantS.astype(np.uint16), "the comb at the bound: S")
    same(host(d16)[0], R.vectorised_select(wantS, 10, 1), "the comb at the bound: disp16")


@gpu
@pytest.mark.parametrize("paths", [4, 8])
def test_the_old_entry_points_through_the_new_one(paths):
    import torch
    rows, cols, D = 24, 96, 32
    kinds = ("box", "random", "shifted", "comb")
    b = len(kinds)
    lefts, rights = G.stack(kinds, rows, cols, D)
    l, r = dev(lefts), dev(rights)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    p = api.make_sgm_params(num_disparities=D)
    with api.Context(0, rows, cols, b) as ctx:
        old_work = torch.full((b * one,), 0xFF, dtype=torch.uint8, device="cuda")
        old16, old_depth = ctx.sgm_dev(l, r, depth=True, d_work=old_work, num_disparities=D, paths=paths)      # dcmt_sgm_dev / dcmt_sgm_paths_dev
        want = np.stack([R.vectorised_select(P.vectorised_volumes(*pair(k, rows, cols, D), D, 200, 800, paths)[1], 10, 1) for k in kinds])
        same(host(old16), want, "the old entry point: the unguided restatement")
        zero = torch.zeros((b, rows, cols), dtype=torch.float32, device="cuda")
        dense = dev(np.stack([GR.guide_kinds(rows, cols, D)["dense"]] * b))
        # NULL with integers the call would refuse of a guide; an all-zero guide; a dense guide at weight 0
        for what, g, weight, cap in (("d_guide = NULL", None, -5, 1 << 30), ("an all-zero guide", zero, 100, 1000), ("weight 0", dense, 0, 1000)):
            new_work = torch.full((b * one,), 0x77, dtype=torch.uint8, device="cuda")
            new16 = torch.full((b, rows, cols), 0x5A5A, dtype=torch.int16, device="cuda")
            new_depth = torch.full((b, rows, cols), -7.0, dtype=torch.float32, device="cuda")
            assert raw_guided_dev(ctx, l, r, g, new16, new_depth, new_work, p, paths, weight, cap) == L.OK, what
            same(host(new16), host(old16), what + ": disp16")
            same(host(new_depth), host(old_depth), what + ": depth")
            same(host(new_work), host(old_work), what + ": both volumes of every frame")
        same(host(ctx.sgm_dev(l, r, num_disparities=D, paths=paths, guide_weight=-5, guide_cap=-5)), host(old16), "sgm_dev without a guide")


@gpu
def test_chunks_determinism_and_a_dirty_workspace():
    import torch
    rows, cols, D, b, paths = 24, 96, 32, 5, 8
    left, right = pair("shifted", rows, cols, D)
    kinds = GR.guide_kinds(rows, cols, D)
    names = ("sparse", "dense", "zero", "hostile", "border")
    planes = np.stack([kinds[n] for n in names])
    vols = [GR.vectorised_volumes(left, right, g, D, 200, 800, paths) for g in planes]
    want = np.stack([R.vectorised_select(S, 10, 1) for _, S in vols])
    assert len({w.tobytes() for w in want}) >= 4                   # the frames differ by their guides alone
    l, r, g = dev(np.stack([left] * b)), dev(np.stack([right] * b)), dev(planes)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    with api.Context(0, rows, cols, b) as ctx:
        alone = np.stack([host(ctx.sgm_dev(l[f:f + 1], r[f:f + 1], num_disparities=D, paths=paths, d_guide=g[f:f + 1]))[0] for f in range(b)])
        same(alone, want, "one frame at a time")
        work = torch.full((2 * one + 8,), 0xFF, dtype=torch.uint8, device="cuda")          # dirty, and a few bytes over
        d16, depth = ctx.sgm_dev(l, r, depth=True, d_work=work, num_disparities=D, paths=paths, d_guide=g)
        same(host(d16), alone, "batch of 5 through a workspace of 2: disp16 (the guide is indexed by frame across chunks)")
        same(host(depth), R.depth_of(alone), "batch of 5 through a workspace of 2: depth")
        first = host(work)
        again16, again_depth = ctx.sgm_dev(l, r, depth=True, d_work=work, num_disparities=D, paths=paths, d_guide=g)
        same(host(again16), host(d16), "second run: disp16")
        same(host(again_depth), host(depth), "second run: depth")
        same(host(work), first, "second run: the workspace")
        for slot, f in ((0, 4), (1, 3)):                            # three chunks: slot 0 ends with frame 4, slot 1 with frame 3
            C, S = G.workspace_volumes(work, slot, rows, cols, D)
            same(C, vols[f][0].astype(np.uint16), f"slot {slot}: C' of frame {f}")
            same(S, vols[f][1].astype(np.uint16), f"slot {slot}: S of frame {f}")


SHIM_DRIVER = os.path.join(ROOT, "tests", "mock_opencv", "shim_sgm_guided_test.cpp")
SHIM_INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv", "with_16s")]


@gpu
def test_host_forms_agree_with_the_device_entry(tmp_path):
    rows, cols, D, paths = 24, 257, 64, 8
    left, right = pair("shifted", rows, cols, D)
    guide = GR.guide_kinds(rows, cols, D)["dense"]
    want = R.vectorised_select(GR.vectorised_volumes(left, right, guide, D, 200, 800, paths)[1], 10, 1)
    lib = L.lib()
    with api.Context(0, rows, cols, 1) as ctx:
        on_device = host(ctx.sgm_dev(dev(left[None]), dev(right[None]), num_disparities=D, paths=paths, d_guide=dev(guide[None])))[0]
        same(on_device, want, "device entry")
        d16, depth = ctx.sgm(left, right, depth=True, paths=paths, guide=guide)
        same(d16, on_device, "Context.sgm(guide=): disp16")
        same(depth, R.depth_of(want), "Context.sgm(guide=): depth")
        wide = np.full((rows, cols + 3), 7.0, f32)                  # rows further apart than they need to be
        wide[:, :cols] = guide
        same(ctx.sgm(left, right, paths=paths, guide=wide[:, :cols]), want, "Context.sgm(guide=), padded guide rows")
        # the C call itself with a padded guide stride
        p = api.make_sgm_params()
        raw = np.full((rows, cols), 77, np.int16)
        call = lambda weight, cap, stride=wide.strides[0]: lib.dcmt_sgm_guided(
            ctx._h, left.ctypes.data, cols, right.ctypes.data, cols, wide.ctypes.data, stride, rows, cols, ctypes.byref(p), raw.ctypes.data, 2 * cols,
            None, 0, paths, weight, cap)
        assert call(100, 1001) == L.E_INVALID and call(10001, 1000) == L.E_INVALID and call(100, -1) == L.E_INVALID
        assert call(100, 1000, 4 * cols - 4) == L.E_INVALID and (raw == 77).all()
        assert call(100, 1000) == L.OK
        same(raw, want, "dcmt_sgm_guided, a padded guide stride")
        four = R.vectorised_select(GR.vectorised_volumes(left, right, guide, D, 200, 800, 4, 100, 9200)[1], 10, 1)
        same(ctx.sgm(left, right, guide=guide, guide_cap=9200), four, "Context.sgm(guide=, guide_cap=9200): four paths")
        with pytest.raises(ValueError):
            ctx.sgm(left, right, guide=guide, guide_cap=9201)
        with pytest.raises(ValueError):
            ctx.sgm_dev(dev(left[None]), dev(right[None]), d_guide=dev(guide[None]), paths=8, guide_cap=1001)
        with pytest.raises(ValueError):
            ctx.sgm_dev(dev(left[None]), dev(right[None]), d_guide=dev(guide[None]), baseline=float("nan"))
    same(api.stereo_sgm(left, right, paths=paths, guide=guide), want, "stereo_sgm(guide=)")
    # the speckle filter chains behind it: a noise pair, whose guided map is all speckles (521 pixels in the restatement)
    srows, scols, sD = 24, 96, 32
    sleft, sright = pair("random", srows, scols, sD)
    kw = dict(num_disparities=sD, paths=paths, guide=GR.guide_kinds(srows, scols, sD)["dense"])
    plain16, plain_depth = api.stereo_sgm(sleft, sright, depth=True, **kw)
    same(plain16, GR.vectorised(sleft, sright, kw["guide"], paths, num_disparities=sD)[0], "unfiltered")
    want16, removed = api.filter_speckles(plain16, max_size=200, max_diff=32)
    assert removed > 0
    g16, gz = api.stereo_sgm(sleft, sright, depth=True, speckle_window=200, speckle_range=2, **kw)
    same(g16, want16, "stereo_sgm(guide=) with a speckle window: disp16")
    same(gz, np.where(want16 != plain16, f32(0), plain_depth), "stereo_sgm(guide=) with a speckle window: depth")
    with api.Context(0, srows, scols, 1) as ctx:
        d16 = ctx.sgm_dev(dev(sleft[None]), dev(sright[None]), num_disparities=sD, paths=paths, d_guide=dev(kw["guide"][None]), speckle_window=200,
                          speckle_range=2)
        same(host(d16)[0], want16, "sgm_dev(d_guide=) with a speckle window")
    # the shim, through a compiled C++ caller
    for name, a in (("left.u8", left), ("right.u8", right), ("guide.f32", guide)):
        a.tofile(tmp_path / name)
    exe = tmp_path / "shim_sgm_guided_test"
    lib_dir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O1"] + SHIM_INCLUDES + [SHIM_DRIVER, "-o", str(exe), "-L" + lib_dir, "-ldcmt_hip", "-Wl,-rpath," + lib_dir,
                    "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True)
    run = subprocess.run([str(exe), str(rows), str(cols), str(D)] + [str(tmp_path / f) for f in ("left.u8", "right.u8", "guide.f32", "disp16.i16")],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)
    same(np.fromfile(tmp_path / "disp16.i16", dtype=np.int16).reshape(rows, cols), want, "dcmt_shim::stereo_sgm_guided")


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
                 paths=8, weight=100, cap=1000, work=A["work"], work_bytes=2 * one):
            return lib.dcmt_sgm_guided_dev(ctx_h, left, right, guide, disp, depth, r, c, n, ctypes.byref(params) if params is not None else None, paths,
                                           weight, cap, work, work_bytes, None)

        # the new refusals, once each
        refused = [call(guide=A["guide"] + 1), call(guide=A["guide"] + 2), call(weight=-1), call(weight=10001), call(cap=-1)]
        refused += [call(cap=1001), call(paths=4, cap=9201), call(params=prm(p2=801)), call(paths=4, params=prm(p2=9001))]
        refused += [call(depth=None, params=prm(baseline=np.nan)), call(depth=None, params=prm(focal=np.inf)), call(depth=None, params=prm(baseline=0.0)),
                    call(depth=None, params=prm(focal=-1.0))]
        refused += [call(guide=A["disp"]), call(guide=A["disp"] + 2 * px - 4), call(guide=A["depth"]), call(guide=A["depth"] - 4), call(guide=A["work"]),
                    call(guide=A["work"] + 2 * one - 4), call(work=A["guide"], work_bytes=one), call(disp=A["guide"]), call(depth=A["guide"])]
        # the refusals of dcmt_sgm_paths_dev, once each
        refused += [call(paths=v) for v in (0, 5, 16)] + [call(params=prm(p2=1801), cap=0), call(paths=4, params=prm(p2=10001), cap=0)]
        refused += [call(ctx_h=None), call(left=None), call(right=None), call(disp=None, depth=None), call(params=None), call(work=None)]
        refused += [call(params=prm(num_disparities=24)), call(params=prm(p1=-1)), call(params=prm(p1=801)), call(params=prm(uniqueness=101)),
                    call(params=prm(baseline=np.nan)), call(params=prm(focal=0.0)), call(params=prm(max_depth=-1.0))]
        refused += [call(disp=A["disp"] + 1), call(depth=A["depth"] + 2), call(work=A["work"] + 8), call(work_bytes=one - 1)]
        refused += [call(r=rows + 1), call(c=cols + 1), call(n=b + 1), call(r=0)]
        refused += [call(disp=A["left"]), call(depth=A["right"] + px - 4), call(disp=A["depth"]), call(disp=A["work"]), call(work=A["left"], work_bytes=one)]
        assert len(refused) > 50 and all(st == L.E_INVALID for st in refused), refused
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all()), "a refused call wrote something"
        # the same arguments without a fault are taken (the guide's 0xA5 bytes are negative floats: no hints, which is fine)
        assert call() == L.OK and call(paths=4, cap=9200) == L.OK and call(params=prm(p1=900, p2=900), cap=900) == L.OK and call(weight=10000) == L.OK
        assert call(weight=0, cap=0) == L.OK and call(depth=None, params=prm(max_depth=np.nan)) == L.OK and call(disp=None) == L.OK
        assert call(n=1, guide=A["left"], disp=A["depth"], depth=None) == L.OK and call(work_bytes=one) == L.OK     # the guide may share memory with the images
        assert call(guide=None, weight=-1, cap=-1) == L.OK and call(guide=None, depth=None, params=prm(baseline=np.nan)) == L.OK
        torch.cuda.synchronize()
        assert not bool((buf[off["disp"]:off["guide"]] == 0xA5).all())
        assert bool((buf[:off["disp"]] == 0xA5).all()) and bool((buf[off["guide"]:off["work"]] == 0xA5).all()), "a call wrote to its inputs"


@gpu
def test_projection_then_guided_matching_on_a_stream_without_host_syncs():
    """project_points_dev(nearest=True) -> sgm_dev(d_guide=) behind a delay kernel on a non-default stream, as tests/test_gpu_sgm_paths.py
    queues the matcher: the copies of the real inputs over decoys, both calls, clones of the outputs and the restoring of the decoys
    are enqueued without the host ever waiting.  The clones must be the real inputs' results, and the marker behind the delay must
    still be pending when the chain has been enqueued."""
    import torch
    rows, cols, D, b, paths = 24, 96, 32, 3, 8
    kinds = ("box", "shifted", "random")
    real = G.stack(kinds, rows, cols, D)
    decoy = G.stack(("random", "same", "box"), rows, cols, D)[::-1]
    T, Pm = np.eye(4, dtype=f32), np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32)
    rng = np.random.default_rng(5)

    def sweeps(per_frame):
        """points that land on pixel centres at depths whose hints spread over 1..8, some twice so that the nearest wins"""
        pts, offsets = [], [0]
        for _ in range(b):
            u, v = rng.integers(0, cols, per_frame), rng.integers(0, rows, per_frame)
            z = (GR.BF / rng.uniform(1.0, 8.0, per_frame)).astype(f32)
            pts.append(np.stack([(u + 0.5) * z, (v + 0.5) * z, z, np.zeros(per_frame)], axis=1).astype(f32))
            offsets.append(offsets[-1] + per_frame)
        return np.concatenate(pts), np.array(offsets, np.int32)

    real_pts, offsets = sweeps(400)
    decoy_pts, _ = sweeps(400)
    ticks = G._ticks_per_ms()
    s = G._stream_beside_the_null_stream(ticks)
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    with api.Context(0, rows, cols, b) as ctx:
        d_off = dev(offsets)
        want_guide = host(ctx.project_points_dev(dev(real_pts), d_off, T, Pm, rows, cols, nearest=True))        # tested elsewhere: the guide as it is
        hinted = [(GR.vectorised_hints(gd, GR.BF, D) >= 0).mean() for gd in want_guide]
        assert all(0.05 < h < 0.5 for h in hinted), hinted
        want = np.stack([GR.vectorised(real[0][f], real[1][f], want_guide[f], paths, num_disparities=D)[0] for f in range(b)])
        assert not np.array_equal(want, np.stack([P.vectorised(real[0][f], real[1][f], num_disparities=D)[0] for f in range(b)]))
        decoy_l, decoy_r, decoy_p = dev(decoy[0]), dev(decoy[1]), dev(decoy_pts)
        l, r, pts = decoy_l.clone(), decoy_r.clone(), decoy_p.clone()
        real_l, real_r, real_p = dev(real[0]), dev(real[1]), dev(real_pts)
        guide = torch.full((b, rows, cols), -3.0, dtype=torch.float32, device="cuda")
        d16 = torch.full((b, rows, cols), 0x5A5A, dtype=torch.int16, device="cuda")
        depth = torch.full((b, rows, cols), -7.0, dtype=torch.float32, device="cuda")
        work = torch.zeros(2 * one, dtype=torch.uint8, device="cuda")

        def chain():
            ctx.project_points_dev(pts, d_off, T, Pm, rows, cols, guide, stream=s.cuda_stream, nearest=True)
            ctx.sgm_dev(l, r, d_disp16=d16, d_depth=depth, d_work=work, stream=s.cuda_stream, num_disparities=D, paths=paths, d_guide=guide)

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
        guide.fill_(-3.0)
        torch.cuda.synchronize()
        d_ms = min(1000.0, max(100.0, 20.0 * t_call * 1e3))
        marker = G._delayed(s, d_ms, ticks)
        with torch.cuda.stream(s):
            l.copy_(real_l)
            r.copy_(real_r)
            pts.copy_(real_p)
            chain()
            pending = not marker.query()
            got16, got_depth, got_guide = d16.clone(), depth.clone(), guide.clone()
            l.copy_(decoy_l)
            r.copy_(decoy_r)
            pts.copy_(decoy_p)
        s.synchronize()
        assert pending, f"the marker behind a {d_ms:.0f} ms delay was complete when the chain returned (t_call {t_call * 1e3:.3f} ms)"
        same(host(got_guide), want_guide, "behind the delay: the guide")
        same(host(got16), want, "behind the delay: disp16")
        same(host(got_depth), R.depth_of(want), "behind the delay: depth")
