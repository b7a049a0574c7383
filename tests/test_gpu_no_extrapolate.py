"""DCMT_FLAG_NO_EXTRAPOLATE on the device: make_params(extrapolate=False) through complete_dev, complete_u16_dev, the labeled form and
the host entry points, bit for bit against restatement (a) of tests/no_extrapolate_restatement.py -- the oracle's X5 (stop_after = 5),
its median5 and gaussian5, select and invert -- on every route: k_local with and without row bands, the staged kernels, overlapping
buffers, the bilateral finish, behind other work on a stream.

Shapes: 8x8 (the smallest k_local takes), 9x70 (one row over a ring of 8, two strips), 33x129 and 64x250 (several strips, the last
one a single column; rows that are no multiple of 8), 97x130 (bands of unequal height); 352x1216 once.  Batches 1, 3, 8 (the XCD
map) and 9.  bilateral_clone has no bit-exact statement of its own: X10 is what dcmt_bilateral5_dev makes of (a)'s X9, which is what
the definition says, and X11 its invert."""
import os

import numpy as np
import pytest

import bilateral_restatement as B
import no_extrapolate_restatement as R
import test_gpu_stream_order as SO
from conftest import assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth
from oracle import oracle as O

gpu = pytest.mark.gpu
f32 = np.float32
SHAPES = [(8, 8), (9, 70), (33, 129), (64, 250), (97, 130)]
MAXB = 9
CLONE = "bilateral_clone"
NOEXT = dict(extrapolate=False)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, 97, 250, MAXB)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the cached planes are read-only)


def host(t):
    return t.cpu().numpy()


_cache = {}


def cached(key, make):
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def frames(rows, cols, n=MAXB):
    """n frames on the 1/256 m grid (the uint16 payload holds the same depths): velodyne-like ones, and sparse random ones between."""
    def make():
        x = synth.synth_batch(n, rows, cols, 7 * rows + cols)
        for f in range(1, n, 3):
            x[f] = R.random_plane(rows, cols, 31 * f + rows, density=0.01)
        return (np.round(x * 256.0) / 256.0).astype(f32)
    return cached(("frames", rows, cols, n), make)


def want(x, key, k0="as_compiled", blur="gaussian", stop=11, labels=None, n_labels=0):
    """(a) for every frame of x, computed once per key"""
    def make():
        return np.stack([R.restatement_oracle(x[f], k0, blur, stop, None if labels is None else labels[f], n_labels) for f in range(x.shape[0])])
    return cached(("want", key, k0, blur, stop, labels is not None), make)


def p(**kw):
    return api.make_params(**NOEXT, **kw)


# ------------------------------------------------------------------------------------------------------------- against (a)
@gpu
@pytest.mark.parametrize("k0", ["as_compiled", "diamond"])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_bit_exact_against_the_restatement(ctx, rows, cols, k0):
    x = frames(rows, cols)
    key = (rows, cols)
    full = want(x, key, k0)
    for b in (1, 3, 8, 9):
        got = host(ctx.complete_dev(dev(x[:b]), None, p(k0=k0)))
        assert ctx.last_path().startswith("k_local"), ctx.last_path()
        assert_bit_equal(got, full[:b], f"{rows}x{cols} {k0} batch {b}")
        assert ctx.last_fill_iters(b) == ([0] * b, L.OK) and ctx.last_holes_after_extend(b) == [0] * b
    for stop in (9, 10, 11):
        for blur in ("none", "gaussian"):
            got = host(ctx.complete_dev(dev(x[:3]), None, p(k0=k0, blur_type=blur, stop_after=stop)))
            assert_bit_equal(got, want(x[:3], key + (3,), k0, blur, stop), f"{rows}x{cols} {k0} stop {stop} {blur}")
    # the bilateral finish: the chain in mode 9 into the median plane, then k_bilateral5
    x9 = want(x[:3], key + (3,), k0, "none", 9)
    x10 = host(ctx.bilateral5_dev(dev(x9)))
    assert_bit_equal(host(ctx.complete_dev(dev(x[:3]), None, p(k0=k0, blur_type=CLONE, stop_after=9))), x9, "bilateral_clone, stop 9")
    assert "bilateral5" not in ctx.last_path()
    assert_bit_equal(host(ctx.complete_dev(dev(x[:3]), None, p(k0=k0, blur_type=CLONE, stop_after=10))), x10, "bilateral_clone, stop 10")
    assert ctx.last_path().startswith("k_local") and ctx.last_path().endswith(" + bilateral5"), ctx.last_path()
    assert_bit_equal(host(ctx.complete_dev(dev(x[:3]), None, p(k0=k0, blur_type=CLONE))), B.invert(x10), "bilateral_clone, stop 11")
    # the host entry point and the drop-in
    assert_bit_equal(ctx.complete(x[:2], p(k0=k0)), full[:2], "host complete")
    assert ctx.last_path().startswith("k_local")


@gpu
@pytest.mark.parametrize("rows,cols", [(9, 70), (64, 250), (97, 130)])
def test_uint16_normalize_and_labels(ctx, rows, cols):
    x = frames(rows, cols)
    key = (rows, cols)
    u16 = np.round(x * 256.0).astype(np.uint16)
    assert np.array_equal(u16.astype(f32) * f32(1.0 / 256.0), x)
    for b in (1, 3, 8, 9):
        for k0 in ("as_compiled", "diamond"):
            got = host(ctx.complete_u16_dev(dev(u16[:b].view(np.int16)), 1.0 / 256.0, None, p(k0=k0)))
            assert ctx.last_path().startswith("k_local<U16>"), ctx.last_path()
            assert_bit_equal(got, want(x, key, k0)[:b], f"uint16 {rows}x{cols} {k0} batch {b}")
    # N1 in front: (a) on the oracle's normalised frames
    xn = cached(("norm", rows, cols), lambda: np.stack([O.normalize_minmax(x[f], 0, 80) for f in range(MAXB)]))
    for b in (3, 8):
        for stop in (9, 11):
            got = host(ctx.complete_dev(dev(x[:b]), None, p(normalize=(0, 80), stop_after=stop)))
            assert ctx.last_path().startswith("k_local<NORM>"), ctx.last_path()
            assert_bit_equal(got, want(xn, key + ("norm",), stop=stop)[:b], f"normalize {rows}x{cols} batch {b} stop {stop}")
    with pytest.raises(api.DcmtError) as e:
        ctx.complete_u16_dev(dev(u16[:1].view(np.int16)), 1.0 / 256.0, None, p(normalize=(0, 80)))
    assert e.value.status == L.E_UNSUPPORTED
    # labels from the oracle's SLIC at the smallest step
    def slic():
        g = np.random.Generator(np.random.PCG64(rows + cols))
        lab, n = [], 0
        for f in range(MAXB):
            img = (g.integers(0, 256, (rows, cols, 3)) // 64 * 64).astype(np.uint8)
            l, n = O.slic(img, 6, 40)
            lab.append(l)
        return np.stack(lab), n
    labels, n = cached(("slic", rows, cols), slic)
    for k0 in ("as_compiled", "diamond"):
        for b in (1, 3, 9):
            for stop in (9, 10, 11):
                got = host(ctx.complete_dev(dev(x[:b]), None, p(k0=k0, stop_after=stop, blur_type="none"), d_labels=dev(labels[:b]), n_labels=n))
                if rows >= 8 and n > 0:
                    assert ctx.last_path().startswith("k_label_bbox + k_label_stage + k_local<START4>"), ctx.last_path()
                assert_bit_equal(got, want(x, key + ("lab",), k0, "gaussian", stop, labels, n)[:b], f"labeled {rows}x{cols} {k0} batch {b} stop {stop}")
        staged = host(ctx.complete_dev(dev(x[:3]), None, p(k0=k0, force_staged=True), d_labels=dev(labels[:3]), n_labels=n))
        assert ctx.last_path() == "k_pre_labeled_v1 + k_post_v1 (staged tile kernels)"
        assert_bit_equal(staged, want(x, key + ("lab",), k0, "gaussian", 11, labels, n)[:3], f"labeled, staged {k0}")
    # use_superpixel = 0: the unlabeled cascade with the Gaussian forced
    got = host(ctx.complete_dev(dev(x[:3]), None, p(blur_type="none"), d_labels=dev(labels[:3]), n_labels=n, use_superpixel=0))
    assert_bit_equal(got, want(x, key)[:3], "use_superpixel = 0")
    assert_bit_equal(api.interpolate_with_superpixels(labels[0], n, x[0], extrapolate=False), want(x, key + ("lab",), "as_compiled", "gaussian", 11, labels, n)[0],
                     "api.interpolate_with_superpixels")
    assert_bit_equal(api.img_completion(x[0], extr=True, extrapolate=False), want(x, key)[0], "api.img_completion")
    assert_bit_equal(api.img_completion(x[0], extr=False), O.img_completion(x[0]), "extr itself stays ignored")


@gpu
def test_kitti_frame():
    x = cached("kitti", lambda: synth.synth_frame(352, 1216, 1))
    w = cached("kitti want", lambda: R.restatement_oracle(x))
    assert int((w == 0).sum()) == 150544
    with api.Context(0, 352, 1216, 1) as c:
        got = host(c.complete_dev(dev(x[None]), None, p()))[0]
        assert c.last_path() == "k_local (row bands)"
        assert_bit_equal(got, w, "352x1216")
        assert_bit_equal(host(c.complete_dev(dev(x[None]), None, p(force_staged=True)))[0], w, "352x1216, staged")


@gpu
def test_adversarial_planes(ctx):
    planes = R.adversarial_planes()
    x = np.stack(list(planes.values()))
    names = list(planes)
    for k0 in ("as_compiled", "diamond"):
        for blur in ("none", "gaussian"):
            for stop in (9, 10, 11):
                w = want(x, "adversarial", k0, blur, stop)
                for kw in ({}, {"force_staged": True}):
                    got = host(ctx.complete_dev(dev(x), None, p(k0=k0, blur_type=blur, stop_after=stop, **kw)))
                    for f, name in enumerate(names):
                        assert_bit_equal(got[f], w[f], f"{name} {k0} {blur} stop {stop} {kw}")
    got = host(ctx.complete_dev(dev(x), None, p()))
    z, full, far = names.index("all zero"), names.index("fully valid"), names.index("far")
    assert_bit_equal(got[z], x[z], "an all-zero frame stays all zero")
    assert_bit_equal(got[full], O.img_completion(x[full]), "X5 without a hole: the default call's bits")
    assert_bit_equal(got[full], host(ctx.complete_dev(dev(x[full:full + 1]), None, api.make_params(spec_fill_iters=4)))[0], "... on the device too")
    m = R.uninverted_pixels(x[far])
    assert m.any() and (got[far][m] < R.THR).all() and (got[far][m] > 0).all()


# ------------------------------------------------------------------------------------------------------------- routes
@gpu
@pytest.mark.parametrize("rows,cols", [(64, 250), (97, 130)])
def test_bit_identity_across_routes(ctx, monkeypatch, rows, cols):
    x = frames(rows, cols)
    ref = want(x, (rows, cols))
    refd = want(x, (rows, cols), "diamond")
    for bands in (1, 2, 3):
        monkeypatch.setenv("DCMT_LOCAL_BANDS", str(bands))
        with api.Context(0, rows, cols, MAXB) as c:
            monkeypatch.delenv("DCMT_LOCAL_BANDS")
            for b in (1, 8, 9):
                got = host(c.complete_dev(dev(x[:b]), None, p()))
                assert c.last_path() == ("k_local (row bands)" if bands > 1 else "k_local"), c.last_path()
                assert_bit_equal(got, ref[:b], f"{bands} bands, batch {b}")
            assert_bit_equal(host(c.complete_dev(dev(x), None, p(k0="diamond", blur_type="none"))), want(x, (rows, cols), "diamond", "none"), f"{bands} bands, diamond")
    assert "DCMT_LOCAL_BANDS" not in os.environ
    staged = host(ctx.complete_dev(dev(x), None, p(force_staged=True)))
    assert ctx.last_path() == "k_pre_v1 + k_post_v1 (staged tile kernels)"
    assert_bit_equal(staged, ref, "FORCE_STAGED")
    assert ctx.last_fill_iters(MAXB) == ([0] * MAXB, L.OK) and ctx.last_holes_after_extend(MAXB) == [0] * MAXB
    custom = host(ctx.complete_dev(dev(x), None, p(k0=O.k0_diamond())))
    assert ctx.last_path().startswith("k_local"), "a custom k0 that equals a preset is that preset"
    assert_bit_equal(custom, refd, "k0 given as the diamond's array")
    k = O.k0_diamond()
    k[0, 0] = 1                                                   # a custom k0: the staged kernels
    got = host(ctx.complete_dev(dev(x[:2]), None, p(k0=k)))
    assert ctx.last_path() == "k_pre_v1 + k_post_v1 (staged tile kernels)"
    p5 = O.default_params(stop_after=5)
    for i in range(25):
        p5.k0[i] = int(k.reshape(25)[i])
    x5 = [O.img_completion(x[f], p5) for f in range(2)]
    assert_bit_equal(got, np.stack([R._finish(v, 11, "gaussian", O.median5, O.gaussian5) for v in x5]), "custom k0")
    inside = host(ctx.complete_dev(dev(x), None, p()))
    for f in (0, 4, 8):
        assert_bit_equal(host(ctx.complete_dev(dev(x[f:f + 1]), None, p()))[0], inside[f], f"frame {f} alone against the same frame in a batch of 9")
    assert_bit_equal(host(ctx.complete_dev(dev(x), None, p(force_fused=True))), ref, "FORCE_FUSED changes nothing")
    assert_bit_equal(host(ctx.complete_dev(dev(x), None, p(max_fill_iters=1, spec_fill_iters=0))), ref, "the loop's parameters are ignored")
    assert_bit_equal(host(ctx.complete_dev(dev(x), None, p(blur_type=CLONE, force_staged=True))),
                     host(ctx.complete_dev(dev(x), None, p(blur_type=CLONE))), "bilateral_clone, staged against k_local")


@gpu
def test_in_place(ctx):
    import torch
    rows, cols, b = 64, 250, 3
    x = frames(rows, cols)[:b]
    ref = want(x, (rows, cols, b))
    n = x.size
    for shift, what in ((0, "d_dst is d_src"), (cols, "d_dst one row into d_src"), (1, "d_dst one element into d_src")):
        for kw, copy in (({}, True), ({"force_staged": True}, False), ({"blur_type": CLONE}, False)):
            buf = torch.full((n + 512,), -7.0, dtype=torch.float32, device="cuda")
            src, dst = buf[:n].view(b, rows, cols), buf[shift:shift + n].view(b, rows, cols)
            src.copy_(dev(x))
            out = ctx.complete_dev(src, src if shift == 0 else dst, p(**kw))
            path = ctx.last_path()
            assert path.endswith(" + copy to dst") == copy, (what, kw, path)
            if "blur_type" not in kw:
                assert_bit_equal(host(out), ref, f"{what} {kw}")
            else:
                assert_bit_equal(host(out), host(ctx.complete_dev(dev(x), None, p(**kw))), f"{what} {kw}")
            assert (host(buf[shift + n:]) == -7.0).all()
        # uint16: the payload's 2 bytes per pixel anywhere inside dst's 4
        u16 = np.round(x * 256.0).astype(np.uint16).view(np.int16)
        raw = torch.full((2 * n + 1024,), -7, dtype=torch.int16, device="cuda")
        for off in (0, 2 * shift, n):                             # the start of dst, shifted, its second half
            src16 = raw[off:off + n].view(b, rows, cols)
            dst = raw[:2 * n].view(torch.float32).view(b, rows, cols)
            src16.copy_(dev(u16))
            out = ctx.complete_u16_dev(src16, 1.0 / 256.0, dst, p())
            assert ctx.last_path() == "k_local<U16> (row bands) + copy to dst", ctx.last_path()
            assert_bit_equal(host(out), ref, f"uint16 in place, offset {off}")
            assert (host(raw[2 * n:]) == -7).all()
    # labeled: k_local reads X4 in scratch and needs no copy
    labels = SO.salt_and_pepper(np.random.Generator(np.random.PCG64(5)), x.shape)
    wl = want(x, (rows, cols, b, "sp"), labels=labels, n_labels=9)
    d = dev(x)
    assert_bit_equal(host(ctx.complete_dev(d, d, p(), d_labels=dev(labels), n_labels=9)), wl, "labeled, d_dst is d_src")
    assert "copy" not in ctx.last_path() and "k_local<START4>" in ctx.last_path()


@gpu
def test_refusals_and_probes(ctx):
    x = frames(64, 250)[:3]
    labels = SO.salt_and_pepper(np.random.Generator(np.random.PCG64(5)), x.shape)
    calls = (lambda q: ctx.complete_dev(dev(x), None, q), lambda q: ctx.complete(x, q),
             lambda q: ctx.complete_dev(dev(x), None, q, d_labels=dev(labels), n_labels=9),
             lambda q: ctx.complete_u16_dev(dev(np.zeros(x.shape, np.int16)), 1.0 / 256.0, None, q))
    ctx.complete_dev(dev(x), None, api.make_params(spec_fill_iters=4))
    before = ctx.last_path()
    for call in calls:
        for stop in (6, 7, 8):
            for kw in ({}, {"force_staged": True}):
                with pytest.raises(api.DcmtError) as e:
                    call(p(stop_after=stop, **kw))
                assert e.value.status == L.E_UNSUPPORTED
        with pytest.raises(api.DcmtError) as e:
            call(p(blur_type="bilateral"))
        assert e.value.status == L.E_UNSUPPORTED
    assert ctx.last_path() == before, "a refused call enqueues nothing and leaves the last call's state"
    # stop_after <= 5: the flag is ignored, bit for bit and in dispatch
    for stop in (2, 3, 4, 5):
        for kw in ({}, {"force_staged": True}):
            a = host(ctx.complete_dev(dev(x), None, p(stop_after=stop, **kw)))
            pa = ctx.last_path()
            bb = host(ctx.complete_dev(dev(x), None, api.make_params(stop_after=stop, **kw)))
            assert pa == ctx.last_path() and "k_local" not in pa
            assert_bit_equal(a, bb, f"stop_after {stop} {kw}")
    # the probes report zeros with DCMT_OK on every route, also where the call without the flag reports an error
    for kw in ({}, {"force_staged": True}, {"blur_type": CLONE}, {"stop_after": 9}):
        ctx.complete_dev(dev(x), None, p(**kw))
        assert ctx.last_fill_iters(3) == ([0, 0, 0], L.OK) and ctx.last_holes_after_extend(3) == [0, 0, 0], kw
    ctx.complete(x, p())
    assert ctx.last_fill_iters(3) == ([0, 0, 0], L.OK)


@gpu
def test_verbose_prints_the_header_lines_only(ctx, capfd):
    x = frames(64, 250)[0]
    import ctypes
    flush = lambda: ctypes.CDLL(None).fflush(None)               # the library prints through C stdio
    ctx.complete(x, p(verbose=True))
    flush()
    out = capfd.readouterr().out.strip().splitlines()
    assert out == ["NUMERO ROWS, COLS: 64 250", f"max range is{float(x.max()):g}"], out
    q = p()
    q.verbose = 2
    ctx.complete(x, q)
    flush()
    assert capfd.readouterr().out == ""


@gpu
def test_unchanged_behaviour(monkeypatch):
    """Default calls before and after a flagged call on one context give the oracle's bits: the staged route, the streaming f32 route,
    the 16-bit form (DCMT_Q16_MIN_WAVES lowered so that a batch of 8 takes it) and the labeled fast path with its box tables."""
    rows, cols, b = 64, 250, 8
    x = frames(rows, cols)[:b]
    default = cached("default 64x250", lambda: np.stack([O.img_completion(x[f]) for f in range(b)]))
    labels = SO.salt_and_pepper(np.random.Generator(np.random.PCG64(5)), x.shape)
    lab_default = cached("labeled default 64x250", lambda: np.stack([O.interpolate_with_superpixels(x[f], labels[f], 9) for f in range(b)]))
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "1")
    with api.Context(0, rows, cols, b) as c:
        monkeypatch.delenv("DCMT_Q16_MIN_WAVES")
        spec = dict(spec_fill_iters=SO.SPEC)

        def defaults(when):
            got = host(c.complete_dev(dev(x), None, api.make_params(**spec)))
            assert "k_fp_q" in c.last_path(), c.last_path()
            assert_bit_equal(got, default, f"16-bit form {when}")
            its, st = c.last_fill_iters(b)
            assert st == L.OK and min(its) >= 1
            got = host(c.complete_dev(dev(x), None, api.make_params(normalize=None, force_staged=True, **spec)))
            assert_bit_equal(got, default, f"staged {when}")
            got = host(c.complete_dev(dev(x[:1]), None, api.make_params(**spec)))
            assert "staged" in c.last_path()
            assert_bit_equal(got[0], default[0], f"one frame {when}")
            got = host(c.complete_dev(dev(x), None, api.make_params(**spec), d_labels=dev(labels), n_labels=9))
            assert c.last_path().startswith("k_label_bbox")
            assert_bit_equal(got, lab_default, f"labeled {when}")

        defaults("before")
        for kw in ({}, {"force_staged": True}, {"blur_type": CLONE}):
            c.complete_dev(dev(x), None, p(**kw))
            c.complete_dev(dev(x), None, p(**kw), d_labels=dev(labels), n_labels=9)
            c.complete_u16_dev(dev(np.round(x * 256.0).astype(np.uint16).view(np.int16)), 1.0 / 256.0, None, p(**kw))
        assert c.last_fill_iters(b) == ([0] * b, L.OK)
        defaults("after")


# ------------------------------------------------------------------------------------------------------------- stream order
def cloud_case(rows=64, cols=250, b=3):
    def inputs(which):
        return {"src": SO.sparse_frames(b, rows, cols, 500 + 50 * which)}

    def call(ctx, t, st):
        ctx.complete_dev(t["src"], t["dst"], p(), stream=st)
        ctx.depth_to_cloud_dev(t["dst"], None, d_offsets=t["offsets"], stream=st)

    def expect(inp):
        dst = np.stack([R.restatement_oracle(inp["src"][f]) for f in range(b)])
        counts = [int((dst[f] > 0).sum()) for f in range(b)]
        dense = [int((O.img_completion(inp["src"][f]) > 0).sum()) for f in range(b)]
        assert all(cnt < d for cnt, d in zip(counts, dense)), "the cloud holds no invented sky: fewer points than the default plane gives"
        return {"dst": dst, "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)}

    return SO.Case("complete without extrapolation + depth_to_cloud 64x250 batch 3", (rows, cols, b), inputs,
                   {"dst": SO.Out((b, rows, cols), f32), "offsets": SO.Out((b + 1,), np.int32, per_frame=False)}, call, expect)


@gpu
def test_queued_behind_other_work_on_a_stream():
    """The scheme of tests/test_gpu_stream_order.py, as test_gpu_bilateral.py uses it: the flagged call and depth_to_cloud_dev behind a
    delay on a non-default stream.  d_offsets[batch] is the number of pixels > 0 in the restatement."""
    got = SO.run_ordered(cloud_case())
    assert got["offsets"][-1] == int((got["dst"] > 0).sum())
