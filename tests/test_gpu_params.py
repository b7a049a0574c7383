"""Non-default dcmt_params.max_depth / valid_thresh on every route of the cascade, bit for bit against the C oracle through
api.Context.  Nothing has a tolerance.

The inputs are the edge frames of tests/param_cases.py: tests/test_oracle_params.py shows on the CPU that the oracle's result on them
moves in at least 5 % of the pixels with each parameter, so a kernel that ignored one (a literal 0.1f in a compare, a literal 100.0f in
an invert) cannot pass.  The parameter grid is P.GRID.

Shapes: 33x70 (partial staged tiles, one streaming strip, an even width: two columns per lane, k_pre_p) and 70x333 (several strips
with a partial right-edge strip at every strip width 34..120, more than one row band, an odd width: one column per lane, k_pre_s);
70x332 where the 16-bit route needs an even width and several strips.  Routes are asserted from dcmt_last_path(), against names
that tests read out of dcmt_plan.h."""
import os
import re

import numpy as np
import pytest

import bilateral_restatement as B
import no_extrapolate_restatement as R
import param_cases as P
from conftest import ROOT, assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api
from oracle import oracle as O

pytestmark = pytest.mark.gpu
f32 = np.float32
SHAPES = ((33, 70), (70, 333))
MAXB = 16
ITERS = 6                         # max_fill_iters of the oracle and the host loop; more than any frame here needs
ENTRY_POINTS = ((50.0, 0.1), (100.0, 2.5), (30.0, 1.0))
CLONE = "bilateral_clone"
grid = pytest.mark.parametrize("mt", P.GRID, ids=P.pid)
entry_grid = pytest.mark.parametrize("mt", ENTRY_POINTS, ids=P.pid)

with open(os.path.join(ROOT, "depth_completion_mt_amd", "csrc", "dcmt_plan.h")) as _f:
    PLAN_NAMES = set(re.findall(r'"([^"\n]*)"', _f.read()))


def plan_name(s):
    """a path fragment, as dcmt_plan.h writes it"""
    assert s in PLAN_NAMES, f"dcmt_plan.h has no {s!r}"
    return s


STAGED = plan_name("k_pre_v1") + plan_name(" + k_fill31_v1 + k_post_v1 (staged tile kernels)")
STAGED_NOEXT = plan_name("k_pre_v1") + plan_name(" + k_post_v1 (staged tile kernels)")
STAGED_LABELED = plan_name("k_pre_labeled_v1") + plan_name(" + k_fill31_v1 + k_post_v1 (staged tile kernels)")
COPY = plan_name(" + copy to dst")
LABEL_STAGE = plan_name("k_label_bbox + k_label_stage + ")
Q16_NAMES = (plan_name("k_pre_p<Q16OUT>"), plan_name("k_pre_p<U16,Q16OUT>"), plan_name(" + k_fp_q"))


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, 70, 333, MAXB)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy()


def mp(mt, **kw):
    kw.setdefault("max_fill_iters", ITERS)
    return api.make_params(max_depth=mt[0], valid_thresh=mt[1], **kw)


def first_kernel(path):
    return path.split(" + ")[0].split(" (")[0]


def no_16_bit(path):
    return not any(n.strip(" +") in path for n in Q16_NAMES)


def stops_and_blurs(lo):
    """(stop_after, blur): every stage from lo on, both blurs where the blur runs (stages 10 and 11), alternating below"""
    out = [(s, ("gaussian", "none")[s % 2]) for s in range(lo, 10)]
    return out + [(s, b) for s in (10, 11) for b in ("gaussian", "none")]


# ---- staged tiles ----------------------------------------------------------------------------------------------------------------
@grid
def test_staged_tiles(ctx, mt):
    """k_pre_v1, k_fill31_v1, k_post_v1: batch 1 (host entry point, synchronised loop) and 2, force_staged at batch 5; stop_after 2..11"""
    M, t = mt
    for rows, cols in SHAPES:
        x = P.batch_frames(rows, cols, 5, M, t)
        for stop, blur in stops_and_blurs(2):
            w = P.batch_want(rows, cols, 5, M, t, blur=blur, stop=stop, max_fill_iters=ITERS)
            what = f"staged {rows}x{cols} {P.pid(mt)} stop {stop} {blur}"
            for f in (0, 1, 2):                                   # edge, gap, empty columns
                got = ctx.complete(x[f], mp(mt, stop_after=stop, blur_type=blur), allow_not_converged=True)
                assert ctx.last_path() == STAGED, ctx.last_path()
                assert_bit_equal(got, w[f], what + f" host, frame {f}")
            got = host(ctx.complete_dev(dev(x[1:3]), None, mp(mt, stop_after=stop, blur_type=blur, spec_fill_iters=ITERS)))
            assert ctx.last_path() == STAGED, ctx.last_path()
            assert_bit_equal(got, w[1:3], what + " batch 2")
            got = host(ctx.complete_dev(dev(x), None, mp(mt, stop_after=stop, blur_type=blur, spec_fill_iters=ITERS, force_staged=True)))
            assert ctx.last_path() == STAGED, ctx.last_path()
            assert_bit_equal(got, w, what + " batch 5, force_staged")
        # a k0 that is no preset takes the staged kernels at every batch size
        for stop in (3, 11):
            w = P.batch_want(rows, cols, 5, M, t, k0="custom", stop=stop, max_fill_iters=ITERS)
            got = host(ctx.complete_dev(dev(x), None, mp(mt, k0=P.K0_CUSTOM, stop_after=stop, spec_fill_iters=ITERS)))
            assert ctx.last_path() == STAGED, ctx.last_path()
            assert_bit_equal(got, w, f"custom k0 {rows}x{cols} {P.pid(mt)} stop {stop}")


# ---- streaming kernels, f32 ------------------------------------------------------------------------------------------------------
@grid
def test_streaming_f32(ctx, mt):
    """k_pre_p (even width) / k_pre_s (odd width), k_fill_s, k_post_s, k_fp_s, k_tail: batch 5 and force_fused at batch 1; the host
    entry point (synchronised loop) and the device one with 1 and 6 speculative applications (k_tail's redo chain); stop_after 6..11"""
    M, t = mt
    for rows, cols in SHAPES:
        x = P.batch_frames(rows, cols, 5, M, t)
        pre = plan_name("k_pre_p" if cols % 2 == 0 else "k_pre_s")
        for k0 in ("as_compiled", "diamond"):
            for stop, blur in stops_and_blurs(6):
                if k0 == "diamond" and stop not in (6, 11):
                    continue
                what = f"streaming {rows}x{cols} {P.pid(mt)} {k0} stop {stop} {blur}"
                w = P.batch_want(rows, cols, 5, M, t, k0=k0, blur=blur, stop=stop, max_fill_iters=ITERS)
                got = ctx.complete(x, mp(mt, k0=k0, stop_after=stop, blur_type=blur), allow_not_converged=True)
                path = ctx.last_path()
                assert first_kernel(path) == pre and no_16_bit(path), path
                assert ("k_fp_s" in path) == (stop == 11), path
                assert_bit_equal(got, w, what + " host")
                for f in (1, 2):
                    got = ctx.complete(x[f], mp(mt, k0=k0, stop_after=stop, blur_type=blur, force_fused=True), allow_not_converged=True)
                    assert first_kernel(ctx.last_path()) == pre, ctx.last_path()
                    assert_bit_equal(got, w[f], what + f" host, force_fused, frame {f}")
                for spec in (1, ITERS):
                    # `spec` applications of the loop, then the tail: the oracle with its loop capped there
                    ws = w if spec == ITERS or stop < 8 else P.batch_want(rows, cols, 5, M, t, k0=k0, blur=blur, stop=stop, max_fill_iters=spec)
                    got = host(ctx.complete_dev(dev(x), None, mp(mt, k0=k0, stop_after=stop, blur_type=blur, spec_fill_iters=spec)))
                    path = ctx.last_path()
                    assert first_kernel(path) == pre and no_16_bit(path), path
                    assert_bit_equal(got, ws, what + f" device, spec_fill_iters {spec}")
                    got = host(ctx.complete_dev(dev(x[1:2]), None, mp(mt, k0=k0, stop_after=stop, blur_type=blur, spec_fill_iters=spec, force_fused=True)))
                    assert first_kernel(ctx.last_path()) == pre, ctx.last_path()
                    assert_bit_equal(got, ws[1:2], what + f" device, force_fused, spec_fill_iters {spec}")


def test_gap_frames_run_the_redo_chain(ctx):
    """what the "gap" frames are there for: under every grid point the fused kernel leaves them with holes (the loop runs twice)"""
    for M, t in P.GRID:
        x = P.batch_frames(70, 333, 5, M, t)
        ctx.complete(x, mp((M, t)))
        iters, st = ctx.last_fill_iters(5)
        assert st == L.OK and max(iters) >= 2, (M, t, iters)
        want = [O.img_completion(x[f], P.oparams(M, t, max_fill_iters=ITERS), return_info=True)[1]["fill_iters"] for f in range(5)]
        assert iters == want, (M, t, iters, want)


# ---- the other entry points ------------------------------------------------------------------------------------------------------
@entry_grid
def test_uint16_entry_point(ctx, mt):
    M, t = mt
    for rows, cols in SHAPES:
        x = P.batch_frames(rows, cols, 5, M, t, on_grid=True)
        u16 = np.round(x * 256.0).astype(np.uint16)
        assert np.array_equal(u16.astype(f32) * f32(1.0 / 256.0), x)
        w = P.batch_want(rows, cols, 5, M, t, on_grid=True, max_fill_iters=ITERS)
        got = host(ctx.complete_u16_dev(dev(u16.view(np.int16)), 1.0 / 256.0, None, mp(mt, spec_fill_iters=ITERS)))
        path = ctx.last_path()
        assert first_kernel(path) == plan_name("k_pre_p<U16>" if cols % 2 == 0 else "k_pre_s") and no_16_bit(path), path
        assert_bit_equal(got, w, f"uint16 {rows}x{cols} {P.pid(mt)} batch 5")
        got = host(ctx.complete_u16_dev(dev(u16[:2].view(np.int16)), 1.0 / 256.0, None, mp(mt, spec_fill_iters=ITERS)))
        assert ctx.last_path() == STAGED, ctx.last_path()
        assert_bit_equal(got, w[:2], f"uint16 {rows}x{cols} {P.pid(mt)} batch 2 (staged)")


@entry_grid
def test_labeled_entry_points(ctx, mt):
    """the three label-stage kernels (streaming route), k_pre_labeled_v1 (staged), host and device, use_superpixel 0 and 1"""
    from test_gpu_fuzz import _labels
    M, t = mt
    for rows, cols in SHAPES:
        x = P.batch_frames(rows, cols, 5, M, t)
        for kind in range(3):
            g = np.random.Generator(np.random.PCG64(300 + 10 * kind + rows))
            lab, n = _labels(g, rows, cols)
            labs = np.ascontiguousarray(np.broadcast_to(lab, x.shape))
            for sp in (1, 0):
                for stop in (4, 11):
                    w = np.stack([O.interpolate_with_superpixels(x[f], lab, n, P.oparams(M, t, stop_after=stop, max_fill_iters=ITERS), use_superpixel=sp)
                                  for f in range(5)])
                    what = f"labeled {rows}x{cols} {P.pid(mt)} labels {kind} use_superpixel {sp} stop {stop}"
                    got = ctx.complete(x, mp(mt, stop_after=stop), labels=labs, n_labels=n, use_superpixel=sp, allow_not_converged=True)
                    path = ctx.last_path()
                    if sp and stop == 11:
                        assert path.startswith(LABEL_STAGE + "k_pre_"), path
                    assert no_16_bit(path), path
                    assert_bit_equal(got, w, what + " host")
                    got = host(ctx.complete_dev(dev(x), None, mp(mt, stop_after=stop, spec_fill_iters=ITERS), d_labels=dev(labs), n_labels=n, use_superpixel=sp))
                    assert_bit_equal(got, w, what + " device")
                    got = host(ctx.complete_dev(dev(x[:2]), None, mp(mt, stop_after=stop, spec_fill_iters=ITERS), d_labels=dev(labs[:2]), n_labels=n, use_superpixel=sp))
                    if sp:
                        assert ctx.last_path() == STAGED_LABELED, ctx.last_path()
                    assert_bit_equal(got, w[:2], what + " device, batch 2 (staged)")


@entry_grid
def test_normalize_in_front(ctx, mt):
    M, t = mt
    for rows, cols in SHAPES:
        x = P.batch_frames(rows, cols, 5, M, t)
        for stop in (6, 11):
            w = np.stack([O.img_completion(O.normalize_minmax(x[f], 0, 80), P.oparams(M, t, stop_after=stop, max_fill_iters=ITERS)) for f in range(5)])
            for b in (5, 2):
                got = host(ctx.complete_dev(dev(x[:b]), None, mp(mt, stop_after=stop, normalize=(0, 80), spec_fill_iters=ITERS)))
                assert_bit_equal(got, w[:b], f"normalize {rows}x{cols} {P.pid(mt)} stop {stop} batch {b}")
            got = ctx.complete(x, mp(mt, stop_after=stop, normalize=(0, 80)), allow_not_converged=True)
            assert_bit_equal(got, w, f"normalize {rows}x{cols} {P.pid(mt)} stop {stop} host")


@entry_grid
def test_in_place(ctx, mt):
    """d_dst == d_src: the whole chain needs no copy; the probes whose first kernel would write dst end in "+ copy to dst" """
    M, t = mt
    for rows, cols in SHAPES:
        x = P.batch_frames(rows, cols, 5, M, t)
        for b, stop, copy in ((5, 11, False), (5, 6, True), (5, 8, False), (2, 11, False), (2, 4, True), (2, 5, True)):
            d = dev(x[:b])
            out = ctx.complete_dev(d, d, mp(mt, stop_after=stop, spec_fill_iters=ITERS))
            assert out.data_ptr() == d.data_ptr()
            assert ctx.last_path().endswith(COPY) == copy, (stop, b, ctx.last_path())
            assert_bit_equal(host(out), P.batch_want(rows, cols, b, M, t, stop=stop, max_fill_iters=ITERS), f"in place {rows}x{cols} {P.pid(mt)} stop {stop} batch {b}")


# ---- no extrapolation, the bilateral finish ---------------------------------------------------------------------------------------
@grid
def test_no_extrapolation(ctx, mt):
    """extrapolate=False: k_local at batch 1 and 5, the staged kernels with force_staged; stop_after 9..11 and three blurs against the
    restatement under (M, t), on the edge frames and on the adversarial planes built around (M, t)"""
    M, t = mt
    i = P.GRID.index(mt)
    for rows, cols in SHAPES:
        planes = [P.edge_frame(rows, cols, P.SEEDS[0], M, t, v) for v in P.VARIANTS]
        adv = R.adversarial_planes(rows, cols, M, t)
        planes += [adv["threshold"], adv["far"]]
        x = np.stack(planes)
        k0 = ("as_compiled", "diamond")[(i + rows) % 2]
        assert sum(int(R.uninverted_pixels(p, k0, M, t).sum()) for p in planes) > 0, "no median-valid pixel whose blurred value is below thr"
        x9 = np.stack([R.restatement_oracle(p, k0, "none", 9, max_depth=M, valid_thresh=t) for p in planes])
        x10b = host(ctx.bilateral5_dev(dev(x9)))
        for stop in (9, 10, 11):
            for blur in ("gaussian", "none", CLONE):
                if blur == CLONE:
                    w = (x9, x10b, B.invert(x10b, M, t))[stop - 9]
                else:
                    w = np.stack([R.restatement_oracle(p, k0, blur, stop, max_depth=M, valid_thresh=t) for p in planes])
                what = f"no extrapolation {rows}x{cols} {P.pid(mt)} {k0} stop {stop} {blur}"
                prm = lambda **kw: mp(mt, k0=k0, stop_after=stop, blur_type=blur, extrapolate=False, **kw)
                got = host(ctx.complete_dev(dev(x), None, prm()))
                assert first_kernel(ctx.last_path()) == plan_name("k_local"), ctx.last_path()
                assert_bit_equal(got, w, what + " k_local batch 5")
                got = host(ctx.complete_dev(dev(x[3:4]), None, prm()))
                assert first_kernel(ctx.last_path()) == plan_name("k_local"), ctx.last_path()
                assert_bit_equal(got, w[3:4], what + " k_local batch 1")
                got = host(ctx.complete_dev(dev(x), None, prm(force_staged=True)))
                assert ctx.last_path().startswith(STAGED_NOEXT), ctx.last_path()
                assert_bit_equal(got, w, what + " staged")


@grid
def test_bilateral_finish(ctx, mt):
    """blur_type="bilateral_clone": the filter runs on X9 (the oracle's, bit for bit) and k_bilateral5's store inverts with (M, t)"""
    M, t = mt
    for rows, cols in SHAPES:
        x = P.batch_frames(rows, cols, 5, M, t)
        x9 = P.batch_want(rows, cols, 5, M, t, blur="none", stop=9, max_fill_iters=ITERS)
        x10 = host(ctx.bilateral5_dev(dev(x9)))
        x11 = B.invert(x10, M, t)
        if f32(M) != f32(P.DEFAULT[0]):     # the store depends on max_depth (on valid_thresh: the planes of test_no_extrapolation, whose X9 has holes)
            assert (x11.view(np.uint32) != B.invert(x10, P.DEFAULT[0], t).view(np.uint32)).mean() >= P.MIN_SENSITIVITY
        for b, kw in ((5, {}), (2, {})):
            got = host(ctx.complete_dev(dev(x[:b]), None, mp(mt, blur_type=CLONE, stop_after=10, spec_fill_iters=ITERS, **kw)))
            assert ctx.last_path().endswith(plan_name(" + bilateral5")), ctx.last_path()
            assert_bit_equal(got, x10[:b], f"bilateral_clone {rows}x{cols} {P.pid(mt)} stop 10 batch {b}")
            got = host(ctx.complete_dev(dev(x[:b]), None, mp(mt, blur_type=CLONE, spec_fill_iters=ITERS, **kw)))
            assert_bit_equal(got, x11[:b], f"bilateral_clone {rows}x{cols} {P.pid(mt)} stop 11 batch {b}")
        assert_bit_equal(ctx.complete(x, mp(mt, blur_type=CLONE), allow_not_converged=True), x11, "bilateral_clone, host")


# ---- the 16-bit route ------------------------------------------------------------------------------------------------------------
Q16_SHAPES = ((33, 70), (70, 332))


def test_16_bit_route_is_for_the_default_parameters_only(monkeypatch):
    """DCMT_Q16_MIN_WAVES=0, frames on the 1/256 m grid, batch 16: a call with non-default parameters names no 16-bit kernel and equals
    the oracle.  Then default and non-default calls in turn on one context, eight of each: every default call still takes the 16-bit
    form (no non-default call has touched the context's flag ring or its skip counter) and equals the oracle, every non-default call
    stays off it and equals the oracle."""
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")
    for rows, cols in Q16_SHAPES:
        xd = P.batch_frames(rows, cols, MAXB, *P.DEFAULT, on_grid=True, codable=True)
        wd = P.batch_want(rows, cols, MAXB, *P.DEFAULT, on_grid=True, codable=True, max_fill_iters=ITERS)
        with api.Context(0, rows, cols, MAXB) as c:
            for mt in P.GRID:
                x = P.batch_frames(rows, cols, MAXB, *mt, on_grid=True)
                got = host(c.complete_dev(dev(x), None, mp(mt, spec_fill_iters=ITERS)))
                path = c.last_path()
                assert first_kernel(path) == plan_name("k_pre_p") and no_16_bit(path), path
                assert_bit_equal(got, P.batch_want(rows, cols, MAXB, *mt, on_grid=True, max_fill_iters=ITERS), f"{rows}x{cols} {P.pid(mt)} on the grid")
                # ... and on the frames of the default call, which the 16-bit route would accept
                got = host(c.complete_dev(dev(xd), None, mp(mt, spec_fill_iters=ITERS)))
                assert no_16_bit(c.last_path()), c.last_path()
                assert_bit_equal(got, P.batch_want(rows, cols, MAXB, *mt, on_grid=True, codable=True, frame_for=P.DEFAULT, max_fill_iters=ITERS),
                                 f"{rows}x{cols} {P.pid(mt)} on the default call's frames")
        with api.Context(0, rows, cols, MAXB) as c:
            for k, mt in enumerate(P.GRID):
                got = host(c.complete_dev(dev(xd), None, mp(P.DEFAULT, spec_fill_iters=ITERS)))
                path = c.last_path()
                assert path.startswith(Q16_NAMES[0]) and Q16_NAMES[2] in path, (k, path)
                assert_bit_equal(got, wd, f"{rows}x{cols} default call {k}")
                x = P.batch_frames(rows, cols, MAXB, *mt, on_grid=True)
                got = host(c.complete_dev(dev(x), None, mp(mt, spec_fill_iters=ITERS)))
                assert no_16_bit(c.last_path()), (k, c.last_path())
                assert_bit_equal(got, P.batch_want(rows, cols, MAXB, *mt, on_grid=True, max_fill_iters=ITERS), f"{rows}x{cols} non-default call {k} {P.pid(mt)}")


# ---- the scaling relation --------------------------------------------------------------------------------------------------------
def test_scaling_relation_on_the_device(ctx, monkeypatch):
    """complete(s x; s M, s t) == s complete(x; M, t) for s = 0.5, 2, 0.25 and (M, t) = (100, 0.1f), the right-hand side computed by the
    library itself at its default parameters -- the route that is held to the compiled reference.  That ties the non-default results to
    it without the extended oracle.  Frames without an empty column at X5 only (the extension's literal 100 does not scale); with the
    16-bit form on the default side where the frames are on the grid (at s = 0.5 the scaled side is off it and takes f32)."""
    M, t = f32(P.DEFAULT[0]), f32(P.DEFAULT[1])
    def relation(c, x, what, q16):
        for k0 in ("as_compiled", "diamond"):
            for blur in ("gaussian", "none"):
                for b, kw in ((len(x), {}), (2, {}), (len(x), dict(force_staged=True))):
                    base = host(c.complete_dev(dev(x[:b]), None, api.make_params(k0=k0, blur_type=blur, max_fill_iters=ITERS, spec_fill_iters=ITERS, **kw)))
                    if q16 and b > 2 and not kw:
                        assert Q16_NAMES[2] in c.last_path(), c.last_path()
                    for s in (0.5, 2.0, 0.25):
                        s = f32(s)
                        got = host(c.complete_dev(dev(x[:b] * s), None, mp((M * s, t * s), k0=k0, blur_type=blur, spec_fill_iters=ITERS, **kw)))
                        assert no_16_bit(c.last_path()), c.last_path()
                        assert_bit_equal(got, base * s, f"{what} {k0} {blur} batch {b} {kw} s = {s}")
    for rows, cols in SHAPES:
        fr = P.scaling_frames(rows, cols)
        assert len(fr) >= 3 and any("gap" in w for w, _ in fr)
        relation(ctx, np.stack([x for _, x in fr][:5]), f"{rows}x{cols}", False)
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")
    for rows, cols in Q16_SHAPES:
        fr = P.scaling_frames(rows, cols, on_grid=True)
        assert len(fr) >= 3
        with api.Context(0, rows, cols, 8) as c:
            relation(c, np.stack([x for _, x in fr][:5]), f"{rows}x{cols} on the grid", True)


# ---- validation ------------------------------------------------------------------------------------------------------------------
BAD = [("max_depth", float("nan")), ("max_depth", float("inf")), ("max_depth", float("-inf")),
       ("valid_thresh", float("nan")), ("valid_thresh", float("inf")), ("valid_thresh", float("-inf")),
       ("valid_thresh", 0.0), ("valid_thresh", -0.0), ("valid_thresh", -1.0)]


def test_validation(ctx):
    """every completion entry point refuses a max_depth or valid_thresh outside the domain; the context is as good as before"""
    from test_gpu_fuzz import _labels
    rows, cols = 33, 70
    M, t = 30.0, 1.0
    x = P.batch_frames(rows, cols, 3, M, t, on_grid=True)
    u16 = dev(np.round(x * 256.0).astype(np.uint16).view(np.int16))
    lab, n = _labels(np.random.Generator(np.random.PCG64(1)), rows, cols)
    labs = np.ascontiguousarray(np.broadcast_to(lab, x.shape))
    d, dl = dev(x), dev(labs)
    calls = {
        "dcmt_complete_f32": lambda p: ctx.complete(x, p),
        "dcmt_complete_f32_dev": lambda p: ctx.complete_dev(d, None, p),
        "dcmt_complete_u16_dev": lambda p: ctx.complete_u16_dev(u16, 1.0 / 256.0, None, p),
        "dcmt_complete_labeled_f32": lambda p: ctx.complete(x, p, labels=labs, n_labels=n),
        "dcmt_complete_labeled_f32_dev": lambda p: ctx.complete_dev(d, None, p, d_labels=dl, n_labels=n),
    }
    want = P.batch_want(rows, cols, 3, M, t, on_grid=True, max_fill_iters=ITERS)
    for name, call in calls.items():
        for field, v in BAD:
            p = mp((M, t), spec_fill_iters=ITERS)
            setattr(p, field, v)
            with pytest.raises(api.DcmtError) as e:
                call(p)
            assert e.value.status == L.E_INVALID, (name, field, v)
        # the smallest positive f32 is inside the domain
        p = mp((M, np.nextafter(f32(0), f32(1))), spec_fill_iters=ITERS)
        call(p)
        got = ctx.complete_dev(d, None, mp((M, t), spec_fill_iters=ITERS))
        assert_bit_equal(host(got), want, f"a good call after the refusals of {name}")


# ---- dispatch toggles ------------------------------------------------------------------------------------------------------------
def test_dispatch_toggles_under_non_default_parameters(tmp_path):
    """The environment toggles pick other kernels for the same arithmetic: under (50, 0.5), 352x1216, batch 16 every one of them must
    reproduce the oracle.  A child process each (the toggles are read when a context is created); the first failure ends the loop."""
    import subprocess, sys, textwrap
    M, t = 50.0, 0.5
    rows, cols = 352, 1216
    frames = np.stack([P.edge_frame(rows, cols, P.frame_spec(i)[0], M, t, P.frame_spec(i)[1]) for i in range(16)])
    frames[7] = P.all_empty(rows, cols)
    check = (0, 1, 2, 4, 7, 15)                    # edge, gap, empty columns, another seed's gap, all empty, the last frame
    for i in (0, 1, 2, 4, 15):
        P.assert_sensitive(frames[i], M, t, f"frame {i}")
    want = np.stack([O.img_completion(frames[i], P.oparams(M, t)) for i in check])
    np.save(tmp_path / "frames.npy", frames)
    np.save(tmp_path / "want.npy", want)
    code = textwrap.dedent(f"""
        import sys; sys.path.insert(0, {ROOT!r})
        import numpy as np, torch
        from depth_completion_mt_amd import Context, make_params
        frames, want = np.load({str(tmp_path / "frames.npy")!r}), np.load({str(tmp_path / "want.npy")!r})
        p = dict(max_depth={M}, valid_thresh={t})
        with Context(0, {rows}, {cols}, 16) as ctx:
            got = ctx.complete(frames, make_params(**p))
            dev = ctx.complete_dev(torch.from_numpy(frames).cuda(), None, make_params(spec_fill_iters=8, **p)).cpu().numpy()
            path = ctx.last_path()
        assert "Q16OUT" not in path and "k_fp_q" not in path, path
        for k, i in enumerate({check!r}):
            assert np.array_equal(got[i].view(np.uint32), want[k].view(np.uint32)), ("host", i)
            assert np.array_equal(dev[i].view(np.uint32), want[k].view(np.uint32)), ("device", i)
        print("OK")
    """)
    for env in ({}, {"DCMT_PAIR": "0"}, {"DCMT_PAIR": "0", "DCMT_WIDE": "0"}, {"DCMT_FUSE_FP": "0"}, {"DCMT_TOP_TABLE": "0"},
                {"DCMT_ASSUME_FILLED": "0"}, {"DCMT_BANDS": "3"}, {"DCMT_FBANDS": "3"}, {"DCMT_Q16_MIN_WAVES": "0"}):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "OK" in r.stdout, (env, r.returncode, r.stdout[-500:], r.stderr[-1500:])
