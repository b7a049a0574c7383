"""DCMT_BLUR_GAUSSIAN_VALID on the device: blur_type="gaussian_valid" through complete_dev / complete_u16_dev / the labeled form with
and without the extrapolation, and gaussian5_dev(valid_thresh=...), bit for bit (as uint32) against tests/gauss_valid_restatement.py.

The cascade's X9 comes from restatement (a) of tests/no_extrapolate_restatement.py (the oracle's X5 and its median5; the two
restatements agree bit for bit: tests/test_no_extrapolate.py), the finish from gv_arrays.

Shapes: 8x8 (the smallest k_local takes), 9x70 (one row over a ring of 8, two strips), 33x70, 70x131 and 33x257 (strip and band
seams, rows that are no multiple of 8, a last strip of few columns); 5x3 and 1x65 (staged for their size); 352x1216 once.  Batches
1, 3 and 5."""
import numpy as np
import pytest

import gauss_valid_restatement as GV
import no_extrapolate_restatement as R
import test_gpu_stream_order as SO
from conftest import assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth
from oracle import oracle as O

gpu = pytest.mark.gpu
f32 = np.float32
SHAPES = [(8, 8), (9, 70), (33, 70), (70, 131), (33, 257)]
MAXB = 5
VALID = "gaussian_valid"
SPEC = 16


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, 70, 257, MAXB)
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
        x = synth.synth_batch(n, rows, cols, 11 * rows + cols)
        for f in range(1, n, 2):
            x[f] = R.random_plane(rows, cols, 37 * f + rows, density=0.01)
        return (np.round(x * 256.0) / 256.0).astype(f32)
    return cached(("frames", rows, cols, n), make)


def want(x, key, k0="as_compiled", stop=11, labels=None, n_labels=0, max_depth=100.0, valid_thresh=0.1):
    """The restatement for every frame of x, computed once per key"""
    def make():
        out = []
        for f in range(x.shape[0]):
            x9 = R.restatement_oracle(x[f], k0, "none", 9, None if labels is None else labels[f], n_labels, max_depth, valid_thresh)
            out.append(x9 if stop == 9 else GV.finish(x9, stop, max_depth, valid_thresh))
        return np.stack(out)
    return cached(("want", key, str(k0), stop, labels is not None, max_depth, valid_thresh), make)


def p(**kw):
    return api.make_params(extrapolate=False, blur_type=VALID, **kw)


# ------------------------------------------------------------------------------------------------- without the extrapolation
@gpu
@pytest.mark.parametrize("k0", ["as_compiled", "diamond"])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_k_local_against_the_restatement(ctx, rows, cols, k0):
    x = frames(rows, cols)
    key = (rows, cols)
    full = want(x, key, k0)
    assert (full[0] < R.THR).any() or rows < 33, "the planes keep holes"
    for b in (1, 3, 5):
        got = host(ctx.complete_dev(dev(x[:b]), None, p(k0=k0)))
        assert ctx.last_path().startswith("k_local<VALID>"), ctx.last_path()
        assert_bit_equal(got, full[:b], f"{rows}x{cols} {k0} batch {b}")
        assert ctx.last_fill_iters(b) == ([0] * b, L.OK)
    for f in (0, 4):
        assert_bit_equal(host(ctx.complete_dev(dev(x[f:f + 1]), None, p(k0=k0)))[0], full[f], f"frame {f} alone")
    got = host(ctx.complete_dev(dev(x[:3]), None, p(k0=k0, stop_after=L.STAGE_BLUR)))
    assert_bit_equal(got, want(x, key, k0, 10)[:3], f"{rows}x{cols} {k0} stop BLUR")
    got = host(ctx.complete_dev(dev(x[:3]), None, p(k0=k0, stop_after=L.STAGE_MEDIAN5)))
    assert "VALID" not in ctx.last_path()
    assert_bit_equal(got, want(x, key, k0, 9)[:3], f"{rows}x{cols} {k0} stop MEDIAN5 ignores the blur")
    # the staged kernels give the same bits
    got = host(ctx.complete_dev(dev(x), None, p(k0=k0, force_staged=True)))
    assert ctx.last_path() == "k_pre_v1 + k_post_v1<VALID> (staged tile kernels)", ctx.last_path()
    assert_bit_equal(got, full, f"{rows}x{cols} {k0} FORCE_STAGED")
    # the host entry point
    assert_bit_equal(ctx.complete(x[:2], p(k0=k0)), full[:2], "host complete")


@gpu
def test_differs_from_the_gaussian_and_from_none(ctx):
    x = frames(70, 131)
    a = want(x, (70, 131))
    g = host(ctx.complete_dev(dev(x), None, api.make_params(extrapolate=False)))
    n = host(ctx.complete_dev(dev(x), None, api.make_params(extrapolate=False, blur_type="none")))
    assert (a.view(np.uint32) != g.view(np.uint32)).any() and (a.view(np.uint32) != n.view(np.uint32)).any()
    inv = a < R.THR
    assert inv.any() and np.array_equal(a.view(np.uint32)[inv], n.view(np.uint32)[inv]), "holes stay what the median left"


@gpu
@pytest.mark.parametrize("rows,cols", [(5, 3), (1, 65)])
def test_small_frames_take_the_staged_route(rows, cols):
    x = cached(("small", rows, cols), lambda: np.stack([GV.holes_plane(rows, cols, 5 + f, holes=0.5) for f in range(3)]))
    with api.Context(0, rows, cols, 3) as c:
        for stop in (10, 11):
            got = host(c.complete_dev(dev(x), None, p(stop_after=stop)))
            assert c.last_path() == "k_pre_v1 + k_post_v1<VALID> (staged tile kernels)", c.last_path()
            assert_bit_equal(got, want(x, ("small", rows, cols), stop=stop), f"{rows}x{cols} stop {stop}")


@gpu
def test_custom_k0(ctx):
    rows, cols = 33, 70
    x = frames(rows, cols)[:3]
    k = O.k0_diamond()
    k[0, 0] = 1
    got = host(ctx.complete_dev(dev(x), None, p(k0=k)))
    assert ctx.last_path() == "k_pre_v1 + k_post_v1<VALID> (staged tile kernels)"
    p5 = O.default_params(stop_after=5)
    for i in range(25):
        p5.k0[i] = int(k.reshape(25)[i])
    w = np.stack([GV.finish(O.median5(O.img_completion(x[f], p5)), 11) for f in range(3)])
    assert_bit_equal(got, w, "custom k0")


@gpu
def test_kitti_frame():
    x = cached("kitti", lambda: synth.synth_frame(352, 1216, 1))
    w = cached("kitti want", lambda: want(x[None], "kitti")[0])
    assert int((w == 0).sum()) == 150544
    with api.Context(0, 352, 1216, 1) as c:
        got = host(c.complete_dev(dev(x[None]), None, p()))[0]
        assert c.last_path() == "k_local<VALID> (row bands)"
        assert_bit_equal(got, w, "352x1216")
        assert_bit_equal(host(c.complete_dev(dev(x[None]), None, p(force_staged=True)))[0], w, "352x1216, staged")
        y = host(c.gaussian5_dev(dev(w[None]), valid_thresh=0.1))[0]
        assert_bit_equal(y, GV.gv_arrays(w), "gaussian5_dev(valid_thresh) 352x1216")
        h = cached("kitti holes", lambda: GV.holes_plane(352, 1216, 1))
        assert_bit_equal(host(c.gaussian5_dev(dev(h[None]), valid_thresh=0.1))[0], GV.gv_arrays(h), "gaussian5_dev(valid_thresh) 352x1216, 40 % holes")


@gpu
@pytest.mark.parametrize("rows,cols", [(9, 70), (70, 131)])
def test_uint16_normalize_and_labels(ctx, rows, cols):
    x = frames(rows, cols)
    key = (rows, cols)
    u16 = np.round(x * 256.0).astype(np.uint16)
    for b in (1, 3, 5):
        for k0 in ("as_compiled", "diamond"):
            got = host(ctx.complete_u16_dev(dev(u16[:b].view(np.int16)), 1.0 / 256.0, None, p(k0=k0)))
            assert ctx.last_path().startswith("k_local<U16,VALID>"), ctx.last_path()
            assert_bit_equal(got, want(x, key, k0)[:b], f"uint16 {rows}x{cols} {k0} batch {b}")
    xn = cached(("norm", rows, cols), lambda: np.stack([O.normalize_minmax(x[f], 0, 80) for f in range(MAXB)]))
    for b in (3, 5):
        for stop in (10, 11):
            got = host(ctx.complete_dev(dev(x[:b]), None, p(normalize=(0, 80), stop_after=stop)))
            assert ctx.last_path().startswith("k_local<NORM,VALID>"), ctx.last_path()
            assert_bit_equal(got, want(xn, key + ("norm",), stop=stop)[:b], f"normalize {rows}x{cols} batch {b} stop {stop}")
    # labels: the labeled entry points honour this blur (every other one they replace by the Gaussian)
    labels = SO.salt_and_pepper(np.random.Generator(np.random.PCG64(rows)), x.shape)
    for k0 in ("as_compiled", "diamond"):
        w = want(x, key + ("sp",), k0, 11, labels, 9)
        for b in (1, 5):
            got = host(ctx.complete_dev(dev(x[:b]), None, p(k0=k0), d_labels=dev(labels[:b]), n_labels=9))
            assert ctx.last_path().startswith("k_label_bbox + k_label_stage + k_local<START4,VALID>"), ctx.last_path()
            assert_bit_equal(got, w[:b], f"labeled {rows}x{cols} {k0} batch {b}")
        got = host(ctx.complete_dev(dev(x[:3]), None, p(k0=k0, force_staged=True), d_labels=dev(labels[:3]), n_labels=9))
        assert ctx.last_path() == "k_pre_labeled_v1 + k_post_v1<VALID> (staged tile kernels)", ctx.last_path()
        assert_bit_equal(got, w[:3], f"labeled, staged {k0}")
        assert_bit_equal(host(ctx.complete_dev(dev(x[:3]), None, p(k0=k0, stop_after=10), d_labels=dev(labels[:3]), n_labels=9)),
                         want(x, key + ("sp",), k0, 10, labels, 9)[:3], f"labeled, stop BLUR {k0}")
    assert_bit_equal(ctx.complete(x[0], p(), labels=labels[0], n_labels=9), want(x, key + ("sp",), "as_compiled", 11, labels, 9)[0], "labeled, host")
    assert_bit_equal(api.img_completion(x[0], blur_type=VALID, extrapolate=False), want(x, key)[0], "api.img_completion")


@gpu
@pytest.mark.parametrize("M,t", [(80.0, 0.25)])
def test_another_max_depth_and_valid_thresh(ctx, M, t):
    import param_cases as PC
    rows, cols = 70, 131
    x = cached(("edge", M, t), lambda: np.stack([PC.edge_frame(rows, cols, 3 + f, M, t) for f in range(3)]))
    w = want(x, ("edge", M, t), max_depth=M, valid_thresh=t)
    assert (w.view(np.uint32) != want(x, ("edge", M, t)).view(np.uint32)).any(), "the parameters matter on these frames"
    for kw in ({}, {"force_staged": True}):
        got = host(ctx.complete_dev(dev(x), None, p(max_depth=M, valid_thresh=t, **kw)))
        assert_bit_equal(got, w, f"max_depth {M} valid_thresh {t} {kw}")


@gpu
def test_adversarial_planes(ctx):
    planes = R.adversarial_planes()
    x = np.stack(list(planes.values()))[:, :, :]
    names = list(planes)
    for k0 in ("as_compiled", "diamond"):
        for stop in (10, 11):
            w = want(x, "adversarial", k0, stop)
            for kw in ({}, {"force_staged": True}):
                got = host(ctx.complete_dev(dev(x[:MAXB]), None, p(k0=k0, stop_after=stop, **kw)))
                for f, name in enumerate(names[:MAXB]):
                    assert_bit_equal(got[f], w[f], f"{name} {k0} stop {stop} {kw}")
                got = host(ctx.complete_dev(dev(x[MAXB:]), None, p(k0=k0, stop_after=stop, **kw)))
                for f, name in enumerate(names[MAXB:]):
                    assert_bit_equal(got[f], w[MAXB + f], f"{name} {k0} stop {stop} {kw}")
    full = names.index("fully valid")
    got = host(ctx.complete_dev(dev(x[full:full + 1]), None, p()))[0]
    assert_bit_equal(got, O.img_completion(x[full]), "a plane without a hole: the default call's bits")


@gpu
def test_in_place(ctx):
    import torch
    rows, cols, b = 70, 131, 3
    x = frames(rows, cols)[:b]
    ref = want(x, (rows, cols))[:b]
    n = x.size
    for shift, what in ((0, "d_dst is d_src"), (cols, "d_dst one row into d_src"), (1, "d_dst one element into d_src")):
        for kw, copy in (({}, True), ({"force_staged": True}, False)):
            buf = torch.full((n + 512,), -7.0, dtype=torch.float32, device="cuda")
            src, dst = buf[:n].view(b, rows, cols), buf[shift:shift + n].view(b, rows, cols)
            src.copy_(dev(x))
            out = ctx.complete_dev(src, src if shift == 0 else dst, p(**kw))
            assert ctx.last_path().endswith(" + copy to dst") == copy, (what, kw, ctx.last_path())
            assert_bit_equal(host(out), ref, f"{what} {kw}")
            assert (host(buf[shift + n:]) == -7.0).all()


# ------------------------------------------------------------------------------------------------- with the extrapolation
@gpu
def test_extrapolating_cascade_equals_the_gaussian_where_the_loop_converges(ctx):
    rows, cols = 70, 131
    x = frames(rows, cols)
    labels = SO.salt_and_pepper(np.random.Generator(np.random.PCG64(3)), x.shape)
    for kw in ({}, {"force_staged": True}, {"k0": "diamond"}):
        for stop in (10, 11):
            for b in (1, 5):
                a = host(ctx.complete_dev(dev(x[:b]), None, api.make_params(blur_type=VALID, spec_fill_iters=SPEC, stop_after=stop, **kw)))
                path = ctx.last_path()
                assert path.endswith(" + gauss5_valid"), path
                assert ctx.last_fill_iters(b)[1] == L.OK
                g = host(ctx.complete_dev(dev(x[:b]), None, api.make_params(spec_fill_iters=SPEC, stop_after=stop, **kw)))
                assert "gauss5_valid" not in ctx.last_path()
                assert_bit_equal(a, g, f"{kw} stop {stop} batch {b}")
    w = np.stack([O.img_completion(x[f]) for f in range(2)])
    assert_bit_equal(host(ctx.complete_dev(dev(x[:2]), None, api.make_params(blur_type=VALID, spec_fill_iters=SPEC))), w, "against the oracle")
    assert_bit_equal(ctx.complete(x[:2], api.make_params(blur_type=VALID)), w, "host complete")
    a = host(ctx.complete_dev(dev(x), None, api.make_params(blur_type=VALID, spec_fill_iters=SPEC), d_labels=dev(labels), n_labels=9))
    assert ctx.last_path().endswith(" + gauss5_valid"), ctx.last_path()
    g = host(ctx.complete_dev(dev(x), None, api.make_params(spec_fill_iters=SPEC), d_labels=dev(labels), n_labels=9))
    assert_bit_equal(a, g, "labeled")
    # stop_after = MEDIAN5 ignores the blur; in place needs no copy (the finish is the call's only writer of dst)
    ctx.complete_dev(dev(x), None, api.make_params(blur_type=VALID, spec_fill_iters=SPEC, stop_after=9))
    assert "gauss5_valid" not in ctx.last_path()
    d = dev(x)
    assert_bit_equal(host(ctx.complete_dev(d, d, api.make_params(blur_type=VALID, spec_fill_iters=SPEC))), np.stack([O.img_completion(f) for f in x]), "in place")
    assert "copy" not in ctx.last_path()


@gpu
def test_extrapolating_cascade_keeps_unclosed_holes_out_of_their_neighbours():
    """max_fill_iters = 1 on a frame whose interior gap two applications of the 31x31 fill cannot close: holes remain in X9, the call
    returns DCMT_E_NOT_CONVERGED as before, and the finish is GV of that plane."""
    rows, cols, b = 240, 64, 3
    x = synth.synth_batch(b, rows, cols, 21)
    x[:, 0:2] = f32(40.0)
    x[:, 4:232] = 0
    x = (np.round(x * 256.0) / 256.0).astype(f32)
    x9 = np.stack([O.img_completion(f, O.default_params(blur="none", stop_after=9, max_fill_iters=1)) for f in x])
    assert ((x9 < R.THR).all(2).sum(1) > 31).all(), "more than 31 whole rows of holes remain in every frame, on the CPU"
    w11 = np.stack([GV.finish(f, 11) for f in x9])
    g11 = np.stack([O.img_completion(f, O.default_params(max_fill_iters=1)) for f in x])
    assert (w11.view(np.uint32) != g11.view(np.uint32)).any(), "here the finish differs from the Gaussian"
    with api.Context(0, rows, cols, b) as c:
        for kw in ({}, {"force_staged": True}):
            got = c.complete(x, api.make_params(blur_type=VALID, max_fill_iters=1, **kw), allow_not_converged=True)
            assert c.last_status == L.E_NOT_CONVERGED
            assert c.last_path().endswith(" + gauss5_valid"), c.last_path()
            assert_bit_equal(got, w11, f"host, capped loop {kw}")
            got = host(c.complete_dev(dev(x), None, api.make_params(blur_type=VALID, max_fill_iters=1, spec_fill_iters=1, **kw)))
            assert c.last_fill_iters(b)[1] == L.E_NOT_CONVERGED
            assert_bit_equal(got, w11, f"device, capped loop {kw}")
            got = host(c.complete_dev(dev(x), None, api.make_params(blur_type=VALID, max_fill_iters=1, spec_fill_iters=1, stop_after=10, **kw)))
            assert_bit_equal(got, np.stack([GV.finish(f, 10) for f in x9]), f"device, capped loop, stop BLUR {kw}")
        with pytest.raises(api.DcmtError):
            c.complete(x, api.make_params(blur_type=VALID, max_fill_iters=1))


# ------------------------------------------------------------------------------------------------- the stand-alone call
def hole_planes(rows, cols, n=3):
    return cached(("holes", rows, cols, n), lambda: np.stack([GV.holes_plane(rows, cols, 100 * rows + cols + f) for f in range(n)]))


@gpu
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 2), (2, 1), (1, 65), (17, 1), (5, 3)] + SHAPES)
def test_stand_alone_against_the_restatement(ctx, rows, cols):
    x = hole_planes(rows, cols)
    w = cached(("gv", rows, cols), lambda: np.stack([GV.gv_arrays(f) for f in x]))
    got = host(ctx.gaussian5_dev(dev(x), valid_thresh=0.1))
    assert_bit_equal(got, w, f"{rows}x{cols}")
    assert_bit_equal(host(ctx.gaussian5_dev(dev(x[1:2]), valid_thresh=0.1))[0], w[1], "a frame alone")
    assert_bit_equal(ctx.gaussian5(x[1], valid_thresh=0.1), w[1], "dcmt_gaussian5_valid")
    wide = np.zeros((rows, cols + 3), f32)
    wide[:, :cols] = x[0]
    assert_bit_equal(ctx.gaussian5(wide[:, :cols], valid_thresh=0.1), w[0], "dcmt_gaussian5_valid, pitched rows")
    if rows * cols > 6:
        got = host(ctx.gaussian5_dev(dev(x), valid_thresh=0.7))
        assert_bit_equal(got, np.stack([GV.gv_arrays(f, 0.7) for f in x]), f"{rows}x{cols} thr 0.7")


@gpu
def test_stand_alone_nan_hole_free_in_place_and_guards(ctx):
    import torch
    rows, cols, b = 33, 70, 3
    # NaN and every other invalid value come back as they are
    xn = np.stack([GV.nan_plane(rows, cols, 3 + f) for f in range(b)])
    assert_bit_equal(host(ctx.gaussian5_dev(dev(xn), valid_thresh=0.1)), np.stack([GV.gv_arrays(f) for f in xn]), "NaN")
    # a hole-free plane: gaussian5_dev's bits
    full = np.stack([R.adversarial_planes()["fully valid"]] * 2)
    assert_bit_equal(host(ctx.gaussian5_dev(dev(full), valid_thresh=0.1)), host(ctx.gaussian5_dev(dev(full))), "hole-free")
    # in place
    x = hole_planes(rows, cols)
    w = np.stack([GV.gv_arrays(f) for f in x])
    d = dev(x)
    same = ctx.gaussian5_dev(d, d_dst=d, valid_thresh=0.1)
    assert same.data_ptr() == d.data_ptr()
    assert_bit_equal(host(same), w, "in place")
    # pointers one element off any wider alignment, inside guard bands that stay as they are; frames do not leak into their neighbours
    n = x.size
    src = torch.full((n + 64,), 55.0, dtype=torch.float32, device="cuda")
    dst = torch.full((n + 64,), -7.0, dtype=torch.float32, device="cuda")
    s, t = src[1:1 + n].view(b, rows, cols), dst[3:3 + n].view(b, rows, cols)
    s.copy_(dev(x))
    ctx.gaussian5_dev(s, t, valid_thresh=0.1)
    out = host(dst)
    assert_bit_equal(out[3:3 + n].reshape(b, rows, cols), w, "offset pointers")
    assert (out[:3] == -7.0).all() and (out[3 + n:] == -7.0).all() and (host(src)[1 + n:] == 55.0).all()
    y = x.copy()
    y[0], y[2] = 90.0, 0.0                                  # other neighbours: the middle frame keeps its bits
    assert_bit_equal(host(ctx.gaussian5_dev(dev(y), valid_thresh=0.1))[1], w[1], "frames are independent")


@gpu
def test_refusals(ctx):
    import torch
    lib = L.lib()
    buf = torch.zeros(3 * 8 * 16 + 64, dtype=torch.float32, device="cuda")
    s, t, far = buf[:384], buf[16:400], torch.zeros(384, dtype=torch.float32, device="cuda")
    call = lambda a, b, thr=0.1, r=8, c=16, n=3: lib.dcmt_gaussian5_valid_dev(ctx._h, a, b, r, c, n, thr, None)   # noqa: E731
    assert call(s.data_ptr(), far.data_ptr()) == L.OK
    assert call(s.data_ptr(), t.data_ptr()) == L.E_INVALID and call(t.data_ptr(), s.data_ptr()) == L.E_INVALID      # partial overlap
    assert call(s.data_ptr(), far.data_ptr() + 2) == L.E_INVALID and call(None, far.data_ptr()) == L.E_INVALID
    for thr in (0.0, -0.0, -0.1, float("nan"), float("inf"), float("-inf")):
        assert call(s.data_ptr(), far.data_ptr(), thr) == L.E_INVALID, thr
    assert call(s.data_ptr(), far.data_ptr(), r=71) == L.E_INVALID and call(s.data_ptr(), far.data_ptr(), n=MAXB + 1) == L.E_INVALID
    h = np.zeros((8, 16), f32)
    assert lib.dcmt_gaussian5_valid(ctx._h, h.ctypes.data, 64, h.ctypes.data, 64, 8, 16, 0.1) == L.OK               # src may be dst
    assert lib.dcmt_gaussian5_valid(ctx._h, h.ctypes.data, 60, h.ctypes.data, 64, 8, 16, 0.1) == L.E_INVALID
    assert lib.dcmt_gaussian5_valid(ctx._h, h.ctypes.data, 64, h.ctypes.data, 64, 8, 16, 0.0) == L.E_INVALID
    torch.cuda.synchronize()
    assert (host(far) == 0).all(), "the refusals write nothing"
    # the cascade: the values beyond the enum are refused as before, the reference's bilateral too
    x = frames(33, 70)[:2]
    q = api.make_params()
    for bad in (4, 6, -1):
        q.blur = bad
        with pytest.raises(api.DcmtError) as e:
            ctx.complete_dev(dev(x), None, q)
        assert e.value.status == L.E_INVALID
    for stop in (6, 7, 8):
        with pytest.raises(api.DcmtError) as e:
            ctx.complete_dev(dev(x), None, p(stop_after=stop))
        assert e.value.status == L.E_UNSUPPORTED


@gpu
def test_unchanged_behaviour(ctx):
    """The default calls name the kernels they named and give the oracle's bits, before and after calls with the new blur."""
    rows, cols = 70, 131
    x = frames(rows, cols)
    default = cached("default", lambda: np.stack([O.img_completion(f) for f in x]))
    noext = cached("noext", lambda: np.stack([R.restatement_oracle(f) for f in x]))

    def defaults(when):
        got = host(ctx.complete_dev(dev(x), None, api.make_params(spec_fill_iters=SPEC)))
        assert "gauss5_valid" not in ctx.last_path() and "VALID" not in ctx.last_path() and "k_fp_s" in ctx.last_path(), ctx.last_path()
        assert_bit_equal(got, default, f"default {when}")
        got = host(ctx.complete_dev(dev(x), None, api.make_params(extrapolate=False)))
        assert ctx.last_path() in ("k_local", "k_local (row bands)"), ctx.last_path()
        assert_bit_equal(got, noext, f"extrapolate=False {when}")
        got = host(ctx.complete_dev(dev(x), None, api.make_params(extrapolate=False, force_staged=True)))
        assert ctx.last_path() == "k_pre_v1 + k_post_v1 (staged tile kernels)"
        assert_bit_equal(got, noext, f"extrapolate=False, staged {when}")
        assert_bit_equal(host(ctx.gaussian5_dev(dev(default))), np.stack([O.gaussian5(f) for f in default]), f"gaussian5_dev {when}")

    defaults("before")
    ctx.complete_dev(dev(x), None, p())
    ctx.complete_dev(dev(x), None, p(force_staged=True))
    ctx.complete_dev(dev(x), None, api.make_params(blur_type=VALID, spec_fill_iters=SPEC))
    ctx.gaussian5_dev(dev(x), valid_thresh=0.1)
    defaults("after")


# ------------------------------------------------------------------------------------------------------------- stream order
def local_case(rows=70, cols=131, b=3):
    def inputs(which):
        return {"src": SO.sparse_frames(b, rows, cols, 600 + 50 * which)}

    def call(ctx, t, st):
        ctx.complete_dev(t["src"], t["dst"], p(), stream=st)

    def expect(inp):
        return {"dst": np.stack([GV.finish(R.restatement_oracle(f, "as_compiled", "none", 9), 11) for f in inp["src"]])}

    return SO.Case("complete gaussian_valid without extrapolation 70x131 batch 3", (rows, cols, b), inputs, {"dst": SO.Out((b, rows, cols), f32)}, call, expect)


def extrapolating_case(rows=64, cols=96, b=4):
    def inputs(which):
        return {"src": SO.sparse_frames(b, rows, cols, 700 + 50 * which, gap=True)}

    def call(ctx, t, st):
        ctx.complete_dev(t["src"], t["dst"], api.make_params(blur_type=VALID, spec_fill_iters=SPEC), stream=st)

    def expect(inp):
        return {"dst": np.stack([O.img_completion(f) for f in inp["src"]])}

    return SO.Case("complete gaussian_valid 64x96 batch 4", (rows, cols, b), inputs, {"dst": SO.Out((b, rows, cols), f32)}, call, expect)


def stand_alone_case(in_place, rows=48, cols=64, b=3):
    def inputs(which):
        return {"src": np.stack([GV.holes_plane(rows, cols, 10 * which + f) for f in range(b)])}

    def call(ctx, t, st):
        ctx.gaussian5_dev(t["src"], t["src"] if in_place else t["dst"], stream=st, valid_thresh=0.1)

    def expect(inp):                                          # (in place: the call made alone, as the scheme's other in-place cases)
        return {"dst": np.stack([GV.gv_arrays(f) for f in inp["src"]])}

    outputs = {"src": SO.Out((b, rows, cols), f32)} if in_place else {"dst": SO.Out((b, rows, cols), f32)}
    return SO.Case(f"gaussian5 valid {'in place' if in_place else 'out of place'}", (rows, cols, b), inputs, outputs, call, None if in_place else expect)


@gpu
@pytest.mark.parametrize("make", [local_case, extrapolating_case, lambda: stand_alone_case(False), lambda: stand_alone_case(True)],
                         ids=["k_local", "extrapolating", "stand-alone", "stand-alone in place"])
def test_queued_behind_other_work_on_a_stream(make):
    """The scheme of tests/test_gpu_stream_order.py: behind a delay on a non-default stream, producer copy, call and consumer copy
    with no host synchronisation between them."""
    SO.run_ordered(make())
