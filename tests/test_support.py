"""The distance to the nearest LiDAR return and the trust mask without a GPU: the two restatements of tests/support_restatement.py
against each other (the literal minimum over the list of returns, and scipy's Euclidean distance transform), what is no return, the
cap and the marker, the select on the bits, what the map says about a KITTI-like frame, on the restatement alone; the launch plan
(tests/plan_support_test.cpp, built against the headers alone); the struct layout, the defaults, the exports and the refusals that
need no device."""
import ctypes

import numpy as np
import pytest

import support_restatement as R
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import synth
from test_plan import _build_and_run

f32, u16, u32 = np.float32, np.uint16, np.uint32
RADII = [1, 9, 40, 255]


def both(plane, what, **kw):
    """The two restatements agree bit for bit; returns (dist2, beyond)."""
    lit, edt = R.literal_dist2(plane, **kw), R.edt_dist2(plane, **kw)
    assert lit[0].dtype == u16 and lit[0].shape == np.asarray(plane).shape
    assert lit[0].tobytes() == edt[0].tobytes() and lit[1] == edt[1], f"{what}: {lit[1]} against {edt[1]} beyond"
    assert lit[1] == int((lit[0] == R.BEYOND).sum()), what
    return lit


@pytest.mark.parametrize("rows,cols", [(33, 130), (65, 129)])
def test_restatements_agree(rows, cols):
    for seed in range(2):
        z = synth.synth_frame(rows, cols, seed)
        assert R.returns_mask(z).sum() > 50
        for radius in RADII:
            d2, n = both(z, f"{rows}x{cols} seed {seed} R {radius}", max_radius=radius)
            assert (d2[R.returns_mask(z)] == 0).all() and ((d2 == 0) == R.returns_mask(z)).all()
    for radius in RADII:                                          # anything a plane may hold, and the payload
        both(R.sparse_plane(rows, cols, 0.05, 7), f"{rows}x{cols} sparse_plane R {radius}", max_radius=radius)
        both(R.payload_plane(rows, cols, 0.05, 7), f"{rows}x{cols} payload R {radius}", max_radius=radius)
    both(R.payload_plane(rows, cols, 0.05, 8), f"{rows}x{cols} payload, another scale", scale=0.01, max_radius=40)
    both(R.sparse_plane(rows, cols, 0.05, 9), f"{rows}x{cols} other bounds", valid_thresh=0.5, max_depth=20.0, max_radius=40)


def test_what_is_no_return():
    """NaN, +-inf, -0.0, negatives and depths outside [valid_thresh, max_depth] are no returns; both bounds themselves are."""
    bad = np.array(R.SPECIALS + (np.nextafter(f32(0.1), f32(0)), np.nextafter(f32(100), f32(1000))), f32)
    z = np.zeros((3, len(bad)), f32)
    z[1] = bad
    assert not R.returns_mask(z).any()
    d2, n = both(z, "specials alone")
    assert n == z.size and (d2 == R.BEYOND).all()
    good = np.array([[0.1, 100.0, np.nextafter(f32(0.1), f32(1)), np.nextafter(f32(100), f32(0)), 5.0]], f32)
    assert R.returns_mask(good).all() and not both(good, "bounds")[0].any()
    assert R.returns_mask(good, valid_thresh=0.5, max_depth=20.0).tolist() == [[False, False, False, False, True]]
    # the payload: 0 and what lies outside the bounds after the ingest
    v = np.array([[0, 25, 26, 25600, 25601, 65535, 512]], u16)
    assert R.returns_mask(v).tolist() == [[False, False, True, True, False, False, True]]
    assert both(v, "payload bounds", max_radius=1)[0].tolist() == [[R.BEYOND, 1, 0, 0, 1, 1, 0]]
    assert R.returns_mask(v, scale=0.01).tolist() == [[False, True, True, False, False, False, True]]        # 25 -> 0.25 m, 25600 -> 256 m


def test_a_frame_without_returns_is_all_beyond():
    for rows, cols in ((1, 1), (5, 3), (33, 130)):
        for radius in RADII:
            d2, n = both(np.zeros((rows, cols), f32), "empty", max_radius=radius)
            assert n == rows * cols and (d2 == R.BEYOND).all()
    d2, n = both(np.zeros((9, 9), u16), "empty payload")
    assert n == 81 and (d2 == R.BEYOND).all()


def test_the_cap_and_the_marker():
    """A lone return at (0, 0) of a 300 x 3 frame with R = 255: row 255 of column 0 is 255^2 = 65025, row 256 is the marker; and no
    value between R^2 + 1 and 65534 ever appears."""
    z = np.zeros((300, 3), f32)
    z[0, 0] = 5.0
    d2, n = both(z, "lone return", max_radius=255)
    assert d2[255, 0] == 65025 and d2[256, 0] == R.BEYOND and d2[255, 1] == R.BEYOND and d2[254, 1] == 254 * 254 + 1 and d2[0, 2] == 4
    assert n == int(((np.arange(300)[:, None] ** 2 + np.arange(3)[None, :] ** 2) > 65025).sum())
    for radius in RADII:
        for plane in (z, synth.synth_frame(65, 129, 0), R.sparse_plane(33, 130, 0.02, 3)):
            d2, _ = both(plane, f"cap at {radius}", max_radius=radius)
            assert not ((d2 > radius * radius) & (d2 < R.BEYOND)).any()
            full, _ = R.edt_dist2(plane, max_radius=255)
            assert np.array_equal(d2, np.where(full <= radius * radius, full, R.BEYOND))     # a smaller radius only hides values


def test_the_select_keeps_the_bits():
    z = R.sparse_plane(33, 130, 0.01, 4)
    dense, fallback = R.dense_planes(33, 130, 5)
    d2, n = both(z, "select")
    near = d2 != R.BEYOND
    assert 0 < n < z.size
    assert np.isnan(dense[near]).any() and np.isnan(fallback[~near]).any() and np.isnan(dense[~near]).any()
    out = R.select(d2, dense, fallback)
    assert np.array_equal(out.view(u32)[near], dense.view(u32)[near]) and np.array_equal(out.view(u32)[~near], fallback.view(u32)[~near])
    out = R.select(d2, dense)
    assert np.array_equal(out.view(u32)[near], dense.view(u32)[near]) and not out.view(u32)[~near].any()       # +0.0f, not -0.0f


def test_what_the_map_says_about_a_kitti_like_frame():
    """synth_frame(352, 1216, 0): 17898 returns, the first of them in row 111.  On the restatement at the default R = 9: every row above
    111 - 9 is wholly beyond, no return is beyond, and 289428 of the 428032 pixels lie within R of a return: a share of 0.6762
    (0.7514 at R = 32, all of them at R = 255)."""
    z = synth.synth_frame(352, 1216, 0)
    ret = R.returns_mask(z)
    first = int(np.argwhere(ret)[0][0])
    assert ret.sum() == 17898 and first == 111
    d2, n = R.edt_dist2(z)
    assert (d2[:first - 9] == R.BEYOND).all() and (d2[first - 9] != R.BEYOND).any()
    assert not d2[ret].any()
    share = 1.0 - n / z.size
    print(f"[support] synth_frame(352, 1216, 0): {z.size - n} of {z.size} pixels within R = 9, a share of {share:.4f}")
    assert z.size - n == 289428 and round(share, 4) == 0.6762
    assert round(1.0 - R.edt_dist2(z, max_radius=32)[1] / z.size, 4) == 0.7514 and R.edt_dist2(z, max_radius=255)[1] == 0


def test_the_plan_as_compiled(tmp_path):
    _build_and_run(tmp_path, "plan_support_test")


def test_layout_defaults_exports_and_refusals_without_a_device():
    from depth_completion_mt_amd import api
    import depth_completion_mt_amd as pkg
    lib = L.lib()
    for name in ("dcmt_default_support_params", "dcmt_support_distance_dev", "dcmt_support_distance_u16_dev", "dcmt_support_distance"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.dcmt_version() == 120
    assert ctypes.sizeof(L.SupportParams) == 12
    assert [(f[0], getattr(L.SupportParams, f[0]).offset) for f in L.SupportParams._fields_] == [("max_radius", 0), ("valid_thresh", 4), ("max_depth", 8)]
    p = L.SupportParams()
    lib.dcmt_default_support_params(ctypes.byref(p))
    lib.dcmt_default_support_params(None)
    assert (p.max_radius, p.valid_thresh, p.max_depth) == (9, float(f32(0.1)), 100.0)
    assert bytes(p) == bytes(api.make_support_params())
    assert {k: R.DEFAULTS[k] for k in ("max_radius", "max_depth")} == dict(max_radius=p.max_radius, max_depth=p.max_depth)
    occl = api.make_occlusion_params()                           # valid_thresh and max_depth are the occlusion filter's defaults
    assert (p.valid_thresh, p.max_depth) == (occl.valid_thresh, occl.max_depth)
    q = api.make_support_params(max_radius=255, valid_thresh=0.0625, max_depth=16384)
    assert (q.max_radius, q.valid_thresh, q.max_depth) == (255, 0.0625, 16384.0) and api.make_support_params(max_radius=1).max_radius == 1
    for kw in (dict(max_radius=0), dict(max_radius=-1), dict(max_radius=256), dict(max_radius=1.5), dict(max_radius=2 ** 31), dict(max_radius=True),
               dict(valid_thresh=0.06), dict(valid_thresh=0.0), dict(valid_thresh=-1.0), dict(valid_thresh=float("nan")), dict(valid_thresh=float("inf")),
               dict(max_depth=0.05), dict(max_depth=16385.0), dict(max_depth=float("inf")), dict(max_depth=float("nan")), dict(valid_thresh=5.0, max_depth=4.0)):
        with pytest.raises(ValueError):
            api.make_support_params(**kw)
    with pytest.raises(TypeError):
        api.make_support_params(rx=1)
    # without a context every argument check is moot: refused before anything touches a device
    assert lib.dcmt_support_distance_dev(None, None, None, None, None, None, 4, 4, 1, ctypes.byref(p), None, None) == L.E_INVALID
    assert lib.dcmt_support_distance_u16_dev(None, None, 1.0 / 256.0, None, None, None, None, 4, 4, 1, ctypes.byref(p), None, None) == L.E_INVALID
    assert lib.dcmt_support_distance(None, None, 16, None, 16, None, 16, None, 16, None, 8, 4, 4, ctypes.byref(p), None) == L.E_INVALID
    for name in ("distance_to_returns", "trust_mask", "make_support_params"):
        assert getattr(pkg, name) is getattr(api, name) and name in pkg.__all__
    for name in ("support_distance_dev", "support_distance"):
        assert hasattr(api.Context, name)
