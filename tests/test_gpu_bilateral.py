"""The bilateral finish on the device: dcmt_bilateral5_dev / dcmt_bilateral5 and blur_type="bilateral_clone" in the cascade.
Every pixel is compared, nothing is masked out.  The yardstick is tests/bilateral_restatement.py's f64 form with the bound below;
the cascade's input to the filter is the oracle's plane behind the median (stop_after = 9), which the cascade matches bit for bit.

TOL = 2e-5 m: about three times the 7.1e-6 measured on a CPU for this operation order with every weight perturbed by 4e-6 relative,
far more than the device's exp errs; a fifth of the Gaussian's 1e-4 class.

Shapes of the stand-alone test: 1x1 and 2x2 (reflection at lengths 1 and 2), 1x70 (one over a strip of 60, a single row), 9x61 (one
over a strip, a band tail behind 8 rows), 33x70 and 48x64 (partial strips, several bands); batch 3, so that frame offsets matter."""
import numpy as np
import pytest

import bilateral_restatement as B
import test_gpu_stream_order as SO
from conftest import assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth
from oracle import oracle as O

gpu = pytest.mark.gpu
f32 = np.float32
TOL = 2e-5
SPEC = 16                    # spec_fill_iters: more applications than any frame here needs, so the device loop ends as the host's does
CLONE = "bilateral_clone"


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, 64, 96, 8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kitti_ctx():
    c = api.Context(0, 352, 1216, 1)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy()


def planes(rows, cols):
    """Three frames: a smooth ramp with noise of about a sigma, steps of a few sigmas with fine noise, uniform noise in [-20, 100]."""
    g = np.random.Generator(np.random.PCG64(1000 * rows + cols))
    yy, xx = np.mgrid[0:rows, 0:cols]
    ramp = 30.0 + 0.4 * xx + 0.7 * yy + g.normal(0.0, 1.0, (rows, cols))
    steps = 20.0 + 3.0 * ((xx // 5 + yy // 3) % 4) + g.normal(0.0, 0.3, (rows, cols))
    noise = g.uniform(-20.0, 100.0, (rows, cols))
    return np.stack([ramp, steps, noise]).astype(f32)


_cache = {}


def cached(key, make):
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def sparse(rows, cols, seed=3):
    return cached(("sparse", rows, cols, seed), lambda: synth.synth_frame(rows, cols, seed))


def median_plane(x, key, k0="as_compiled"):
    return cached(("median", key, k0), lambda: O.img_completion(x, O.default_params(k0=k0, blur="none", stop_after=9)))


def max_err(got, want64, what):
    e = float(np.abs(got.astype(np.float64) - want64).max())
    print(f"[bilateral] {what}: max |device - f64| = {e:.3g} m")
    return e


# ------------------------------------------------------------------------------------------------------------- stand-alone
@gpu
@pytest.mark.parametrize("sigmas", [(1.5, 2.0), (3.0, 1.0)])
@pytest.mark.parametrize("rows,cols", [(1, 1), (2, 2), (1, 70), (9, 61), (33, 70), (48, 64)])
def test_stand_alone_against_the_f64_restatement(ctx, rows, cols, sigmas):
    x = cached(("planes", rows, cols), lambda: planes(rows, cols))
    got = host(ctx.bilateral5_dev(dev(x), None, *sigmas))
    assert got.shape == x.shape and np.isfinite(got).all()
    for f in range(3):
        want = cached(("f64", rows, cols, f, sigmas), lambda: B.restatement_f64(x[f], *sigmas))
        assert max_err(got[f], want, f"{rows}x{cols} frame {f} sigma {sigmas}") <= TOL
    # the host twin and the module-level call: the same kernel, the same bits
    assert_bit_equal(ctx.bilateral5(x[1], *sigmas), got[1], "dcmt_bilateral5")
    wide = np.zeros((rows, cols + 3), f32)
    wide[:, :cols] = x[0]
    assert_bit_equal(ctx.bilateral5(wide[:, :cols], *sigmas), got[0], "dcmt_bilateral5, pitched rows")


@gpu
def test_module_level_call(ctx):
    x = cached(("planes", 33, 70), lambda: planes(33, 70))
    assert_bit_equal(api.bilateral_filter5(x[0]), host(ctx.bilateral5_dev(dev(x[:1])))[0], "bilateral_filter5")


@gpu
def test_constant_planes_and_in_place(ctx):
    c = np.stack([np.full((33, 70), v, f32) for v in (0.0, 7.25, 99.999)])
    assert_bit_equal(host(ctx.bilateral5_dev(dev(c))), c, "constant planes")
    x = cached(("planes", 33, 70), lambda: planes(33, 70))
    out = host(ctx.bilateral5_dev(dev(x)))
    d = dev(x)
    same = ctx.bilateral5_dev(d, d_dst=d)
    assert same.data_ptr() == d.data_ptr()
    assert_bit_equal(host(same), out, "in place")
    # an edge of 40 m between two constant halves stays where the Gaussian smears it
    e = np.full((1, 16, 32), 20.0, f32)
    e[:, :, 16:] = 60.0
    assert np.abs(host(ctx.bilateral5_dev(dev(e))) - e).max() <= 1e-6
    assert np.abs(host(ctx.gaussian5_dev(dev(e))) - e).max() > 1.0


@gpu
def test_refusals(ctx):
    import torch
    lib = L.lib()
    buf = torch.zeros(3 * 8 * 16 + 64, dtype=torch.float32, device="cuda")
    s, t, far = buf[:384], buf[16:400], torch.zeros(384, dtype=torch.float32, device="cuda")
    call = lambda a, b, sc=1.5, ss=2.0, r=8, c=16, n=3: lib.dcmt_bilateral5_dev(ctx._h, a, b, r, c, n, sc, ss, None)
    assert call(s.data_ptr(), far.data_ptr()) == L.OK
    assert call(s.data_ptr(), t.data_ptr()) == L.E_INVALID and call(t.data_ptr(), s.data_ptr()) == L.E_INVALID      # partial overlap
    assert call(s.data_ptr(), far.data_ptr() + 2) == L.E_INVALID and call(None, far.data_ptr()) == L.E_INVALID
    for sc, ss in ((0.0, 2.0), (1.5, 0.0), (-1.5, 2.0), (1.5, -2.0), (float("nan"), 2.0), (1.5, float("inf")), (1e-30, 2.0)):
        assert call(s.data_ptr(), far.data_ptr(), sc, ss) == L.E_INVALID, (sc, ss)
    assert call(s.data_ptr(), far.data_ptr(), r=65) == L.E_INVALID and call(s.data_ptr(), far.data_ptr(), n=9) == L.E_INVALID
    h = np.zeros((8, 16), f32)
    assert lib.dcmt_bilateral5(ctx._h, h.ctypes.data, 64, h.ctypes.data, 64, 8, 16, 1.5, 2.0) == L.OK              # src may be dst
    assert lib.dcmt_bilateral5(ctx._h, h.ctypes.data, 60, h.ctypes.data, 64, 8, 16, 1.5, 2.0) == L.E_INVALID
    assert lib.dcmt_bilateral5(ctx._h, h.ctypes.data, 64, h.ctypes.data, 64, 8, 16, 0.0, 2.0) == L.E_INVALID
    torch.cuda.synchronize()
    assert (host(far) == 0).all()


# ------------------------------------------------------------------------------------------------------------- the cascade
@gpu
@pytest.mark.parametrize("k0", ["as_compiled", "diamond"])
@pytest.mark.parametrize("rows,cols", [(48, 64), (33, 70), (352, 1216)])
def test_cascade_parity(ctx, kitti_ctx, rows, cols, k0):
    c = kitti_ctx if rows > 64 else ctx
    x = sparse(rows, cols)
    med = median_plane(x, (rows, cols), k0)
    want = cached(("cascade f64", rows, cols, k0), lambda: B.restatement_f64(med))
    d = dev(x[None])
    blur = host(c.complete_dev(d, None, api.make_params(k0=k0, blur_type=CLONE, stop_after=L.STAGE_BLUR, spec_fill_iters=SPEC)))[0]
    assert c.last_path().endswith(" + bilateral5")
    assert max_err(blur, want, f"cascade {rows}x{cols} {k0}") <= TOL
    fused = host(c.complete_dev(d, None, api.make_params(k0=k0, blur_type=CLONE, stop_after=L.STAGE_BLUR, spec_fill_iters=SPEC, force_fused=True)))[0]
    assert c.last_path().startswith("k_pre_") and c.last_path().endswith(" + bilateral5")
    assert_bit_equal(fused, blur, "FORCE_FUSED")
    final = host(c.complete_dev(d, None, api.make_params(k0=k0, blur_type=CLONE, spec_fill_iters=SPEC)))[0]
    assert_bit_equal(final, B.invert(blur), "stop_after = FINAL against the invert of stop_after = BLUR")
    m = host(c.complete_dev(d, None, api.make_params(k0=k0, blur_type=CLONE, stop_after=L.STAGE_MEDIAN5, spec_fill_iters=SPEC)))[0]
    assert_bit_equal(m, med, "stop_after = MEDIAN5 ignores the blur")
    assert "bilateral5" not in c.last_path()


@gpu
def test_all_zero_frame_stays_zero(ctx):
    z = np.zeros((4, 48, 64), f32)
    for kw in ({}, {"force_staged": True}):
        assert_bit_equal(host(ctx.complete_dev(dev(z), None, api.make_params(blur_type=CLONE, **kw))), z, f"all zero {kw}")
    assert_bit_equal(ctx.complete(z[0], api.make_params(blur_type=CLONE)), z[0], "all zero, host")


def route_frames():
    """Four 64x96 frames on the 1/256 m grid (so the uint16 payload holds the same depths); the last one with a 40-row gap, which
    the hole-closure loop has to close."""
    def make():
        x = SO.sparse_frames(4, 64, 96, 300, gap=True)
        return (np.round(x * 256.0) / 256.0).astype(f32)
    return cached("route frames", make)


@gpu
def test_bit_identity_across_routes(ctx):
    import torch
    x = route_frames()
    p = lambda **kw: api.make_params(blur_type=CLONE, spec_fill_iters=SPEC, **kw)
    ref = host(ctx.complete_dev(dev(x), None, p()))
    path = ctx.last_path()
    assert path.startswith("k_pre_") and path.endswith(" + bilateral5"), path
    its, st = ctx.last_fill_iters(4)
    assert st == L.OK and max(its) > 1 and max(its) < SPEC, its                # the loop ran, and dcmt_last_fill_iters keeps reporting
    # against the statement, on the oracle's median planes
    blur = host(ctx.complete_dev(dev(x), None, p(stop_after=L.STAGE_BLUR)))
    for f in range(4):
        assert max_err(blur[f], B.restatement_f64(median_plane(x[f], ("route", f))), f"route frame {f}") <= TOL
    assert_bit_equal(ref, B.invert(blur), "FINAL against the invert of BLUR")

    staged = host(ctx.complete_dev(dev(x), None, p(force_staged=True)))
    assert "staged tile kernels" in ctx.last_path() and ctx.last_path().endswith(" + bilateral5")
    assert_bit_equal(staged, ref, "FORCE_STAGED")
    assert_bit_equal(host(ctx.complete_dev(dev(x), None, p(force_fused=True))), ref, "FORCE_FUSED")
    for f in (0, 3):                                                           # batch 1: the staged route, and the streaming one
        assert_bit_equal(host(ctx.complete_dev(dev(x[f:f + 1]), None, p()))[0], ref[f], f"frame {f} alone")
        assert "staged tile kernels" in ctx.last_path()
        assert_bit_equal(host(ctx.complete_dev(dev(x[f:f + 1]), None, p(force_fused=True)))[0], ref[f], f"frame {f} alone, FORCE_FUSED")
        assert ctx.last_path().startswith("k_pre_")
    assert_bit_equal(ctx.complete(x, api.make_params(blur_type=CLONE)), ref, "host complete")
    assert ctx.last_path().endswith(" + bilateral5")
    assert_bit_equal(api.img_completion(x[3], blur_type=CLONE), ref[3], "img_completion")
    u16 = np.round(x * 256.0).astype(np.uint16)
    assert np.array_equal(u16.astype(f32) * f32(1.0 / 256.0), x)
    assert_bit_equal(host(ctx.complete_u16_dev(dev(u16.view(np.int16)), 1.0 / 256.0, None, p())), ref, "complete_u16_dev")
    assert ctx.last_path().endswith(" + bilateral5")
    assert_bit_equal(host(ctx.complete_u16_dev(dev(u16.view(np.int16)), 1.0 / 256.0, None, p(force_staged=True))), ref, "complete_u16_dev, FORCE_STAGED")

    # N1 in front: the routes agree with each other and with the statement on the oracle's normalised frames
    norm = host(ctx.complete_dev(dev(x), None, p(normalize=(0, 80))))
    assert ctx.last_path().endswith(" + bilateral5")
    assert_bit_equal(host(ctx.complete_dev(dev(x), None, p(normalize=(0, 80), force_staged=True))), norm, "normalize, FORCE_STAGED")
    assert_bit_equal(ctx.complete(x, api.make_params(blur_type=CLONE, normalize=(0, 80))), norm, "normalize, host")
    nblur = host(ctx.complete_dev(dev(x), None, p(normalize=(0, 80), stop_after=L.STAGE_BLUR)))
    assert_bit_equal(norm, B.invert(nblur), "normalize: FINAL against the invert of BLUR")
    for f in range(4):
        med = O.img_completion(O.normalize_minmax(x[f], 0, 80), O.default_params(blur="none", stop_after=9))
        assert max_err(nblur[f], B.restatement_f64(med), f"normalize frame {f}") <= TOL

    # dst on src, and one row and one element into it: the filter is the call's only writer of dst
    n = x.size
    for shift, what in ((0, "d_dst is d_src"), (96, "d_dst one row into d_src"), (1, "d_dst one element into d_src")):
        for kw in ({}, {"force_staged": True}):
            buf = torch.full((n + 128,), -7.0, dtype=torch.float32, device="cuda")
            src, dst = buf[:n].view(4, 64, 96), buf[shift:shift + n].view(4, 64, 96)
            src.copy_(dev(x))
            out = ctx.complete_dev(src, src if shift == 0 else dst, p(**kw))
            assert_bit_equal(host(out), ref, f"{what} {kw}")
            assert ctx.last_path().endswith(" + bilateral5") and "copy" not in ctx.last_path()
            assert (host(buf[shift + n:]) == -7.0).all()


@gpu
def test_unchanged_behaviour(ctx):
    x = route_frames()
    g = np.random.Generator(np.random.PCG64(5))
    labels = SO.salt_and_pepper(g, x.shape)
    for kw in ({}, {"force_staged": True}):
        a = host(ctx.complete_dev(dev(x), None, api.make_params(blur_type=CLONE, spec_fill_iters=SPEC, **kw), d_labels=dev(labels), n_labels=9))
        assert "bilateral5" not in ctx.last_path()
        b = host(ctx.complete_dev(dev(x), None, api.make_params(blur_type="gaussian", spec_fill_iters=SPEC, **kw), d_labels=dev(labels), n_labels=9))
        assert_bit_equal(a, b, f"the labeled call forces the Gaussian {kw}")
    assert_bit_equal(ctx.complete(x[0], api.make_params(blur_type=CLONE), labels=labels[0], n_labels=9),
                     ctx.complete(x[0], api.make_params(blur_type="gaussian"), labels=labels[0], n_labels=9), "labeled, host")
    for call in (lambda q: ctx.complete_dev(dev(x), None, q), lambda q: ctx.complete(x, q),
                 lambda q: ctx.complete_dev(dev(x), None, q, d_labels=dev(labels), n_labels=9)):
        for stop in (L.STAGE_FINAL, L.STAGE_CLOSE5):
            with pytest.raises(api.DcmtError) as e:
                call(api.make_params(blur_type="bilateral", stop_after=stop))
            assert e.value.status == L.E_UNSUPPORTED
    q = api.make_params()
    q.blur = 4
    with pytest.raises(api.DcmtError) as e:
        ctx.complete_dev(dev(x), None, q)
    assert e.value.status == L.E_INVALID
    # the Gaussian's own path names no new step
    ctx.complete_dev(dev(x), None, api.make_params(spec_fill_iters=SPEC))
    assert "bilateral5" not in ctx.last_path()


# ------------------------------------------------------------------------------------------------------------- stream order
def cascade_case(rows=64, cols=96, b=4):
    def inputs(which):
        return {"src": SO.sparse_frames(b, rows, cols, 400 + 50 * which, gap=True)}

    def call(ctx, t, st):
        ctx.complete_dev(t["src"], t["dst"], api.make_params(blur_type=CLONE, spec_fill_iters=SPEC), stream=st)

    return SO.Case("complete bilateral_clone 64x96 batch 4", (rows, cols, b), inputs, {"dst": SO.Out((b, rows, cols), f32)}, call)


def stand_alone_case(in_place, rows=48, cols=64, b=3):
    def inputs(which):
        return {"src": planes(rows, cols) + f32(which)}

    def call(ctx, t, st):
        ctx.bilateral5_dev(t["src"], t["src"] if in_place else t["dst"], stream=st)

    outputs = {"src": SO.Out((b, rows, cols), f32)} if in_place else {"dst": SO.Out((b, rows, cols), f32)}
    return SO.Case(f"bilateral5 {'in place' if in_place else 'out of place'}", (rows, cols, b), inputs, outputs, call)


@gpu
@pytest.mark.parametrize("make", [cascade_case, lambda: stand_alone_case(False), lambda: stand_alone_case(True)],
                         ids=["cascade", "stand-alone", "stand-alone in place"])
def test_queued_behind_other_work_on_a_stream(make):
    """The scheme of tests/test_gpu_stream_order.py: behind a delay on a non-default stream, producer copy, call and consumer copy
    with no host synchronisation between them; the clone holds the bits of the call made alone."""
    SO.run_ordered(make())
