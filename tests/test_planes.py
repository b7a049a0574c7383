"""The per-superpixel plane fit without a GPU: the two restatements of tests/planes_restatement.py against each other (the definition
of include/dcmt.h pixel by pixel on Python ints and np.float64 scalars, and vectorised), hand-worked cases, the clamp, keep_returns,
the recovery of exact facets and the trimmed refit on the restatement alone, the launch plan and the fit as the device compiles it
(tests/plan_planes_test.cpp, built against the headers alone), the struct layouts, the defaults, the exports and the refusals that
need no device."""
import ctypes

import numpy as np
import pytest

import planes_restatement as R
from depth_completion_mt_amd import _lib as L
from test_plan import _build_and_run

f32, f64, i32 = np.float32, np.float64, np.int32
SIZES = [(1, 1), (1, 70), (3, 33), (17, 65), (24, 70)]
GRID = [{}, dict(refit_tol=0.05), dict(refit_tol=0.5, min_points=8, min_extent=1, keep_returns=False), dict(min_extent=5, valid_thresh=0.5, max_depth=20.0)]


def both(depth, labels, n, what, **kw):
    """The two restatements agree bit for bit; returns (out, fits)."""
    lit, closed = R.literal_planes(depth, labels, n, **kw), R.closed_planes(depth, labels, n, **kw)
    assert lit[0].dtype == f32 and lit[0].shape == depth.shape and lit[1].dtype == R.FIT_DTYPE and lit[1].shape == (n,), what
    assert np.array_equal(lit[0].view(np.uint32), closed[0].view(np.uint32)), f"{what}: {int((lit[0].view(np.uint32) != closed[0].view(np.uint32)).sum())} pixels differ"
    assert lit[1].tobytes() == closed[1].tobytes(), f"{what}: fits differ at {np.flatnonzero(lit[1] != closed[1])[:5]}"
    return lit


@pytest.mark.parametrize("rows,cols", SIZES)
def test_restatements_agree(rows, cols):
    kinds = np.zeros(3, np.int64)
    for seed in range(2):
        depth = R.sparse_depth(rows, cols, 0.3, seed)
        cases = R.plane_cases(rows, cols) + [("voronoi", R.voronoi(rows, cols)), ("blocks", R.block_labels(rows, cols, 4)[0])]
        assert {c[0].split()[0] for c in cases} >= set(R.PLANES)
        for name, plane in cases:
            n = max(6, int(plane.max()) + 1) if name.split()[0] in ("rows", "blocks") else 6
            for kw in GRID:
                kinds += np.bincount(both(depth, plane, n, f"{name} {rows}x{cols} seed {seed} {kw}", **kw)[1]["kind"], minlength=3)
    z, lab, n, _ = R.facet_scene(rows, cols, 2, 0.4, 5)
    both(z, lab, n, f"facets {rows}x{cols}", refit_tol=0.1)
    assert kinds[R.NONE] > 0 and kinds[R.CONSTANT] > 0 and (kinds[R.PLANE] > 0 or rows == 1)


def frame(rows, cols, returns, label=0):
    """A frame of one label (or the label plane given) with the returns {(u, v): code} as depths whose code is exactly that."""
    z = np.zeros((rows, cols), f32)
    for (u, v), w in returns.items():
        z[v, u] = f32(65536.0) / f32(w)
        assert int(np.rint(R.W32 / z[v, u])) == w
    lab = np.full((rows, cols), label, i32) if np.isscalar(label) else np.asarray(label, i32)
    return z, lab


def test_hand_worked_cases():
    # three returns exactly on w = 3 u + 5 v + 1000: the plane itself, at every pixel inside the measured range
    z, lab = frame(4, 5, {(0, 0): 1000, (2, 0): 1006, (0, 2): 1010})
    out, fits = both(z, lab, 1, "three on a plane")
    assert fits[0]["kind"] == R.PLANE and fits[0]["a"] == 3.0 and fits[0]["b"] == 5.0 and abs(fits[0]["c"] - 1000.0) < 1e-9
    assert (fits[0]["seen"], fits[0]["used"], fits[0]["wmin"], fits[0]["wmax"]) == (3, 3, 1000, 1010)
    assert abs(f64(out[1, 1]) - 65536.0 / 1008.0) < 1e-5 and out[0, 0] == z[0, 0] and out[2, 0] == z[2, 0]
    # collinear returns: the determinant is exactly 0, the label is its mean
    z, lab = frame(6, 6, {(0, 0): 1000, (1, 1): 1001, (2, 2): 1005, (5, 5): 1006})
    out, fits = both(z, lab, 1, "collinear")
    assert fits[0]["kind"] == R.CONSTANT and fits[0]["c"] == 1003.0 and fits[0]["a"] == 0.0 and out[0, 5] == f32(65536.0 / 1003.0) and out[5, 5] == z[5, 5]
    # returns on one row: min_extent = 2 refuses them on the extent, min_extent = 1 on the determinant
    z, lab = frame(6, 10, {(0, 4): 1000, (5, 4): 2000, (9, 4): 3000})
    for me in (2, 1):
        out, fits = both(z, lab, 1, f"one row, min_extent {me}", min_extent=me)
        assert fits[0]["kind"] == R.CONSTANT and fits[0]["c"] == 2000.0 and out[0, 0] == f32(65536.0 / 2000.0)
    # a label with no return, labels -1 and >= n_labels: zeros, whatever depth they hold; the fits of the empty label are zeros
    lab = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [-1, -1, 2, 2], [7, 7, 2, 2]], i32)
    z, _ = frame(4, 4, {(0, 0): 1000, (1, 0): 1002, (0, 1): 1004, (0, 2): 500, (1, 3): 600, (2, 2): 900})
    out, fits = both(z, lab, 3, "empty and out of range")
    assert fits["kind"].tolist() == [R.PLANE, R.NONE, R.CONSTANT] and fits[1].tobytes() == bytes(48)
    assert (out[:2, 2:] == 0).all() and (out[2:, :2] == 0).all() and (out[:2, :2] != 0).all() and (out[2:, 2:] != 0).all()
    assert out[2, 2] == z[2, 2] and out[3, 3] == f32(65536.0 / 900.0)
    out2, _ = both(z, lab, 3, "empty and out of range, returns not kept", keep_returns=False)
    assert (out2[2:, :2] == 0).all() and out2[2, 2] == f32(65536.0 / 900.0)


def test_what_is_no_return():
    """NaN, +-inf, -0.0, negatives and depths outside [valid_thresh, max_depth] are no returns: a label that holds nothing else is of
    kind none, and beside real returns they change nothing."""
    bad = np.array(R.SPECIALS, f32)
    z = np.zeros((3, len(bad)), f32)
    z[0] = bad
    out, fits = both(z, np.zeros(z.shape, i32), 1, "specials alone")
    assert fits[0]["kind"] == R.NONE and not out.view(np.uint32).any()
    z[1, 0], z[1, 3], z[2, 1] = 0.1, 100.0, 7.0                  # the bounds themselves are returns
    clean = z.copy()
    clean[0] = 0
    a, b = both(z, np.zeros(z.shape, i32), 1, "specials among returns"), both(clean, np.zeros(z.shape, i32), 1, "without them")
    assert a[1].tobytes() == b[1].tobytes() and a[1][0]["seen"] == 3 and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert (a[0] != 0).all()                                     # the specials' pixels are painted like every other pixel of the label


def test_clamp_and_keep_returns():
    # a steep plane through three returns in a corner of a large label: beyond them it is held at wmin / wmax
    z, lab = frame(8, 40, {(0, 0): 1000, (2, 0): 1200, (0, 2): 1100})
    out, fits = both(z, lab, 1, "clamp")
    assert fits[0]["kind"] == R.PLANE and fits[0]["a"] == 100.0 and fits[0]["b"] == 50.0
    assert out[0, 39] == f32(65536.0 / 1200.0) and out[7, 39] == f32(65536.0 / 1200.0) and out[0, 1] == f32(65536.0 / 1100.0)
    assert out.min() >= f32(65536.0 / 1200.0) and out.max() <= f32(65536.0 / 1000.0)
    # keep_returns: on, a return keeps its bits; off, it gets the fit like its neighbours
    z, lab, n, _ = R.facet_scene(24, 70, 4, 0.2, 1)
    z[z > 0] *= f32(1.0001)                                      # off the planes by less than the code's step, yet other bits
    on, off = both(z, lab, n, "keep on"), both(z, lab, n, "keep off", keep_returns=False)
    ret = z > 0
    assert np.array_equal(on[0][ret].view(np.uint32), z[ret].view(np.uint32)) and (on[0][ret] != off[0][ret]).any()
    assert np.array_equal(on[0][~ret].view(np.uint32), off[0][~ret].view(np.uint32)) and on[1].tobytes() == off[1].tobytes()


def test_in_place_equals_out_of_place():
    """What the device's in-place call rests on, on the restatements: they read their input and never modify it, every output pixel
    is a function of the input alone (the moments are complete before the paint), and a kept return has its own bits -- so writing
    the output over the input pixel by pixel, each read before its write, gives the out-of-place bits.  The device's in-place call
    is in tests/test_gpu_planes.py."""
    z, lab, n, _ = R.facet_scene(24, 70, 4, 0.2, 2)
    before = z.copy()
    out, fits = both(z, lab, n, "facets")
    assert np.array_equal(z.view(np.uint32), before.view(np.uint32))
    assert np.array_equal(out[z > 0].view(np.uint32), z[z > 0].view(np.uint32))
    aliased = z.copy()
    aliased[...] = R.closed_planes(aliased, lab, n)[0]           # the call on a buffer that is then overwritten with its result
    assert np.array_equal(aliased.view(np.uint32), out.view(np.uint32))


def recovery(out, fits, z, lab, truth):
    """(largest relative depth error over the pixels of plane-kind labels inside the bounding box of their returns, share of the
    labelled pixels that are of plane kind)."""
    V, U = np.mgrid[0:z.shape[0], 0:z.shape[1]]
    worst = 0.0
    for k in np.flatnonzero(fits["kind"] == R.PLANE):
        vv, uu = np.nonzero((lab == k) & (z > 0))
        box = (lab == k) & (U >= uu.min()) & (U <= uu.max()) & (V >= vv.min()) & (V <= vv.max())
        worst = max(worst, float((np.abs(out[box].astype(f64) - truth[box]) / truth[box]).max()))
    return worst, float((fits["kind"][lab] == R.PLANE).mean())


def test_recovery_of_exact_facets():
    """facet_scene(48, 160, 12, 0.05, 0): every label is an exact plane of inverse depth.  Unclamped, the fit is within 1.5e-4 of it
    (the code's quantisation, 0.5 / 819 at 80 m, averaged); what the condition measures is dominated by the CLAMP: in the corners of a
    label's bounding box of returns a steep facet leaves the measured range [wmin, wmax] and is held there.  Measured on the restatement
    alone, seed 0: 0.3491 (seeds 1..3: 0.2819, 0.2907, 0.2339); asserted: twice that."""
    z, lab, n, truth = R.facet_scene(48, 160, 12, 0.05, 0)
    out, fits = R.closed_planes(z, lab, n)
    worst, share = recovery(out, fits, z, lab, truth)
    print(f"[planes] recovery on facet_scene(48, 160, 12, 0.05, 0): {worst:.4f}, plane share {share:.3f}")
    assert share >= 0.9
    assert worst <= 2 * 0.3491                                   # measured: 0.3491
    V, U = np.mgrid[0:48, 0:160]
    what = fits["a"][lab] * U + fits["b"][lab] * V + fits["c"][lab]
    assert (np.abs(65536.0 / what - truth) / truth).max() < 3e-4  # the planes themselves


def test_refit():
    """outlier_scene: 20 % of facet 0's returns at twice their depth.  The error of a fit on that facet is taken where the truth is
    measured and the clamp does not bind: at the facet's undisplaced returns, with keep_returns off.  Measured: 0.1883 untrimmed,
    0.0001 with refit_tol = 0.25 (all 28 undisplaced returns kept, all 7 displaced ones dropped)."""
    z, lab, n, truth, facet = R.outlier_scene(48, 160, 12, 0.05, 0, share=0.2, factor=2.0)
    clean = R.facet_scene(48, 160, 12, 0.05, 0)[0]
    inliers = (lab == facet) & (z > 0) & (z == clean)
    moved = (lab == facet) & (z != clean)
    assert moved.sum() == round(0.2 * ((lab == facet) & (z > 0)).sum()) and inliers.sum() >= 20

    def error(**kw):
        out, fits = both(z, lab, n, f"outliers {kw}", keep_returns=False, **kw)
        return float((np.abs(out[inliers].astype(f64) - truth[inliers]) / truth[inliers]).max()), fits

    plain, f0 = error()
    trimmed, f1 = error(refit_tol=0.25)
    print(f"[planes] outlier facet: {plain:.4f} untrimmed, {trimmed:.4f} trimmed, used {f0[facet]['used']} -> {f1[facet]['used']}")
    assert trimmed < plain and trimmed < 1e-3 and f1[facet]["seen"] == f0[facet]["seen"] == inliers.sum() + moved.sum()
    assert f1[facet]["used"] == inliers.sum()
    others = np.arange(n) != facet
    assert f0[others].tobytes() == f1[others].tobytes()          # exact facets lose nothing at this tolerance
    # on the clean scene both fits are bit-identical
    a, b = both(clean, lab, n, "clean"), both(clean, lab, n, "clean, refit", refit_tol=0.25)
    assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    # a trimmed set that is no plane leaves the first fit standing: a tolerance nothing but one return meets
    z2, lab2 = frame(4, 5, {(0, 0): 1000, (2, 0): 1006, (0, 2): 1010, (2, 2): 1400})
    first, again = both(z2, lab2, 1, "first"), both(z2, lab2, 1, "refit to nothing", refit_tol=1e-6)
    assert first[1].tobytes() == again[1].tobytes() and first[1][0]["kind"] == R.PLANE


def test_plans_and_the_fit_as_compiled(tmp_path):
    _build_and_run(tmp_path, "plan_planes_test")


def test_layouts_defaults_exports_and_refusals_without_a_device():
    from depth_completion_mt_amd import api
    import depth_completion_mt_amd as pkg
    lib = L.lib()
    for name in ("dcmt_default_planes_params", "dcmt_superpixel_planes_max_labels", "dcmt_superpixel_planes_dev", "dcmt_superpixel_planes"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert ctypes.sizeof(L.PlanesParams) == 24 and ctypes.sizeof(L.PlaneFit) == 48 == api.PLANE_FIT_DTYPE.itemsize == R.FIT_DTYPE.itemsize
    assert [(f[0], getattr(L.PlaneFit, f[0]).offset) for f in L.PlaneFit._fields_] == [(nm, api.PLANE_FIT_DTYPE.fields[nm][1]) for nm in api.PLANE_FIT_DTYPE.names]
    assert api.PLANE_FIT_DTYPE == R.FIT_DTYPE
    assert [getattr(L.PlanesParams, f[0]).offset for f in L.PlanesParams._fields_] == [0, 4, 8, 12, 16, 20]
    p = L.PlanesParams()
    lib.dcmt_default_planes_params(ctypes.byref(p))
    lib.dcmt_default_planes_params(None)
    assert (p.valid_thresh, p.max_depth, p.min_points, p.min_extent, p.refit_tol, p.keep_returns) == (float(f32(0.1)), 100.0, 3, 2, 0.0, 1)
    q = api.make_planes_params()
    assert bytes(p) == bytes(q)
    assert {k: (float(f32(v)) if isinstance(v, float) else int(v)) for k, v in R.DEFAULTS.items()} == {f[0]: getattr(q, f[0]) for f in L.PlanesParams._fields_}
    q = api.make_planes_params(valid_thresh=0.0625, max_depth=16384, min_points=9, min_extent=1, refit_tol=0.5, keep_returns=False)
    assert (q.valid_thresh, q.max_depth, q.min_points, q.min_extent, q.refit_tol, q.keep_returns) == (0.0625, 16384.0, 9, 1, 0.5, 0)
    for kw in (dict(valid_thresh=0.06), dict(valid_thresh=0.0), dict(valid_thresh=-1.0), dict(valid_thresh=float("nan")), dict(valid_thresh=float("inf")),
               dict(max_depth=0.05), dict(max_depth=16385.0), dict(max_depth=float("inf")), dict(max_depth=float("nan")), dict(valid_thresh=5.0, max_depth=4.0),
               dict(min_points=2), dict(min_points=0), dict(min_points=2.5), dict(min_points=2 ** 31), dict(min_extent=0), dict(min_extent=-1),
               dict(refit_tol=1.0), dict(refit_tol=-0.1), dict(refit_tol=float("nan")), dict(keep_returns=2), dict(keep_returns="yes")):
        with pytest.raises(ValueError):
            api.make_planes_params(**kw)
    with pytest.raises(TypeError):
        api.make_planes_params(blur=1)
    # the n_labels bound: 96 bytes a label and frame in one scratch plane of 4 * max_rows * max_cols * max_batch bytes
    assert lib.dcmt_superpixel_planes_max_labels(352, 1216, 8, 1) == 352 * 1216 * 8 // 24 == api.superpixel_planes_max_labels(352, 1216, 8)
    assert api.superpixel_planes_max_labels(352, 1216, 8, 8) == 352 * 1216 // 24 and api.superpixel_planes_max_labels(24, 96, 1) == 96
    assert api.superpixel_planes_max_labels(4, 5, 1) == 0 and api.superpixel_planes_max_labels(0, 5, 1) == 0 and api.superpixel_planes_max_labels(4, 5, 1, 2) == 0
    assert lib.dcmt_version() == 120
    # without a context every argument check is moot: refused before anything touches a device
    assert lib.dcmt_superpixel_planes_dev(None, None, None, 4, 4, 1, 1, ctypes.byref(p), None, None, None) == L.E_INVALID
    assert lib.dcmt_superpixel_planes(None, None, 16, None, 16, 4, 4, 1, ctypes.byref(p), None, 16, None) == L.E_INVALID
    assert pkg.fit_superpixel_planes is api.fit_superpixel_planes and pkg.make_planes_params is api.make_planes_params
    assert pkg.PLANE_FIT_DTYPE is api.PLANE_FIT_DTYPE and pkg.superpixel_planes_max_labels is api.superpixel_planes_max_labels
    for name in ("superpixel_planes_dev", "superpixel_planes"):
        assert hasattr(api.Context, name)
    for name in ("fit_superpixel_planes", "make_planes_params", "PLANE_FIT_DTYPE", "superpixel_planes_max_labels"):
        assert name in pkg.__all__
