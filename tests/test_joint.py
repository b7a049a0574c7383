"""The joint bilateral filter without a GPU: the two restatements of tests/joint_restatement.py against each other (the definition
pixel by pixel, and whole planes shifted tap by tap), the host's tables against numpy's, what the definition promises exactly (a
constant plane, the two-region scene, a frame without a valid pixel, entries above 255), on the restatements alone; the launch plan
(tests/plan_joint_test.cpp, built against the headers alone); the struct layouts, the defaults, the exports and the refusals that need
no device."""
import ctypes

import numpy as np
import pytest

import joint_restatement as J
from depth_completion_mt_amd import _lib as L
from test_plan import _build_and_run

f32, u8, u16, u32 = np.float32, np.uint8, np.uint16, np.uint32
FLAGS = [(True, False), (False, True), (True, True)]


def both(depth, guide, tab, what, **kw):
    """The two restatements agree bit for bit; returns (out, filled, left)."""
    lit, tap = J.literal(depth, guide, tab, **kw), J.tap_major(depth, guide, tab, **kw)
    assert lit[0].dtype == f32 and lit[0].shape == depth.shape
    assert lit[0].tobytes() == tap[0].tobytes() and lit[1:] == tap[1:], f"{what}: {lit[1:]} against {tap[1:]}"
    assert lit[1] + lit[2] == int((~J.valid_mask(depth)).sum()), what                      # filled + left = the holes of the frame
    return lit


@pytest.mark.parametrize("radius", [1, 3, 9])
@pytest.mark.parametrize("rows,cols", [(33, 130), (65, 129)])
def test_restatements_agree(rows, cols, radius):
    """Oracle-completed synth_frame planes with random holes, NaN, +-inf, -0.0, negatives and values one ulp inside and outside both
    bounds (holed_plane), 1 and 3 channels, every flag combination, min_weight 1 and 5000."""
    for channels in (1, 3):
        for fill, smooth in FLAGS:
            for mw in (1, 5000):
                z, g, tab, out, filled, left = J.case(rows, cols, 1, channels, radius, fill, smooth, mw)
                lit = J.literal(z, g, tab, radius=radius, fill=fill, smooth=smooth, min_weight=mw)
                what = f"{rows}x{cols} R {radius} ch {channels} fill {fill} smooth {smooth} min_weight {mw}"
                assert lit[0].tobytes() == out.tobytes() and lit[1:] == (filled, left), what
                ok = J.valid_mask(z)
                assert filled + left == int((~ok).sum()) and (filled > 0) == fill, what
                if not smooth:                                        # valid pixels keep their bytes
                    assert np.array_equal(out.view(u32)[ok], z.view(u32)[ok]), what
                if not fill:                                          # holes keep theirs, NaN payloads and -0.0 included
                    assert np.array_equal(out.view(u32)[~ok], z.view(u32)[~ok]) and left == int((~ok).sum()), what
    z = J.case(rows, cols, 1, 1, radius, True, False, 1)[0]
    assert np.isnan(z).any() and np.isinf(z).any() and (z.view(u32) == 0x80000000).any() and (z < 0).any()


def test_what_is_a_hole():
    """NaN, +-inf, -0.0, negatives and depths outside [valid_thresh, max_depth] are holes; both bounds themselves are valid."""
    bad = np.array(J.SPECIALS + (np.nextafter(f32(0.1), f32(0)), np.nextafter(f32(100), f32(1000)), 0.0), f32)
    assert not J.valid_mask(bad[None, :]).any()
    good = np.array([[0.1, 100.0, np.nextafter(f32(0.1), f32(1)), np.nextafter(f32(100), f32(0)), 5.0]], f32)
    assert J.valid_mask(good).all()
    assert J.valid_mask(good, valid_thresh=0.5, max_depth=20.0).tolist() == [[False, False, False, False, True]]
    # a row of holes between two valid pixels, R = 1: only the neighbours of a valid pixel are filled, with exactly its value
    z = np.concatenate([[5.0], bad, [7.0]]).astype(f32)[None, :]
    g = np.zeros(z.shape, u8)
    out, filled, left = both(z, g, J.tables(1), "specials", radius=1)
    assert filled == 2 and left == len(bad) - 2 and out[0, 1] == 5.0 and out[0, -2] == 7.0
    assert np.array_equal(out.view(u32)[0, 2:-2], z.view(u32)[0, 2:-2])


@pytest.mark.parametrize("radius,ss,sg", [(1, 0.5, 1.0), (6, 3.0, 10.0), (9, 4.5, 25.0), (9, 100.0, 1000.0), (3, 0.01, 0.01)])
def test_make_joint_tables_equals_numpy(radius, ss, sg):
    from depth_completion_mt_amd import api
    t = api.make_joint_tables(radius, ss, sg)
    ws, wg = J.tables(radius, ss, sg)
    assert t.dtype == api.JOINT_TABLES_DTYPE and t.shape == (1,) and t.dtype.itemsize == 1792
    assert np.array_equal(t["w_space"][0], ws) and np.array_equal(t["w_guide"][0], wg)
    assert ws[0] == 255 and wg[0] == 255 and not ws[radius * radius + 1:].any() and ws.max() <= 255 and wg.max() <= 255


def test_entries_above_255_behave_as_255():
    z, g = J.holed_plane(33, 130, 2), J.guide_plane(33, 130, 3, 2)
    g2 = np.random.Generator(np.random.PCG64(5))
    ws, wg = g2.integers(0, 65536, 128).astype(u16), g2.integers(0, 65536, 768).astype(u16)
    assert (ws > 255).sum() > 100 and (wg > 255).sum() > 700
    want = both(z, g, (ws, wg), "wide entries", radius=3, smooth=True)
    got = both(z, g, (np.minimum(ws, 255), np.minimum(wg, 255)), "clamped entries", radius=3, smooth=True)
    assert want[0].tobytes() == got[0].tobytes() and want[1:] == got[1:]


def test_a_constant_plane_comes_back_bit_for_bit():
    gen = np.random.Generator(np.random.PCG64(3))
    for value in (f32(0.1), f32(13.37), f32(100.0)):
        z = np.full((33, 70), value, f32)
        for channels in (1, 3):
            g = gen.integers(0, 256, (33, 70) if channels == 1 else (33, 70, 3)).astype(u8)
            tab = J.tables(9, 4.0, 300.0)
            out, filled, left = both(z, g, tab, "constant", radius=9, smooth=True)
            assert out.tobytes() == z.tobytes() and filled == left == 0
            holed = z.copy()
            holed[gen.random(z.shape) < 0.4] = 0.0
            out, filled, left = both(holed, g, tab, "constant with holes", radius=9, smooth=True)
            assert out.tobytes() == z.tobytes() and left == 0 and filled == int((holed == 0).sum())


def test_a_frame_without_a_valid_pixel_comes_back_unchanged():
    for rows, cols in ((1, 1), (5, 3), (33, 130)):
        z = np.resize(np.array(J.SPECIALS + (0.0,), f32), (rows, cols)).copy()
        g = J.guide_plane(rows, cols, 1, 0)
        for fill, smooth in FLAGS:
            out, filled, left = both(z, g, J.tables(9), "no valid pixel", radius=9, fill=fill, smooth=smooth)
            assert out.tobytes() == z.tobytes() and filled == 0 and left == rows * cols


def test_the_two_region_scene():
    """48 x 96, depth 10 | 30 and grey 60 | 180 with noise in -3..3, columns 43..52 zeroed; R = 6, sigma_space 3, sigma_guide 10, FILL.
    With the guide every tap across the edge has w_guide = 0: all 480 holes are filled and the plane equals the truth bit for bit.
    With w_guide == 255 (no guide) the band is blurred across the edge: measured 2.46 m at most, 96 pixels off by more than 1 m; only
    "more than 1 m somewhere" is asserted."""
    truth, holed, grey = J.two_regions()
    assert truth.shape == (48, 96) and int((holed == 0).sum()) == 480 and 57 <= grey[:, :48].min() and grey[:, :48].max() <= 63
    ws, wg = J.tables(6, 3.0, 10.0)
    assert not wg[120 - 6:].any()                                    # what lies across the edge weighs nothing
    out, filled, left = both(holed, grey, (ws, wg), "two regions", radius=6)
    assert (filled, left) == (480, 0) and out.tobytes() == truth.tobytes()
    blind, filled, left = both(holed, grey, (ws, np.full(768, 255, u16)), "two regions, no guide", radius=6)
    err = np.abs(blind - truth)
    print(f"[joint] two regions without the guide: largest error {err.max():.4f} m, {int((err > 1).sum())} pixels off by more than 1 m")
    assert (filled, left) == (480, 0) and err.max() > 1.0 and not err[:, :43].any() and not err[:, 53:].any()


def test_the_plan_as_compiled(tmp_path):
    _build_and_run(tmp_path, "plan_joint_test")


def test_layout_defaults_exports_and_refusals_without_a_device():
    from depth_completion_mt_amd import api
    import depth_completion_mt_amd as pkg
    lib = L.lib()
    for name in ("dcmt_default_joint_params", "dcmt_make_joint_tables", "dcmt_joint_bilateral_dev", "dcmt_joint_bilateral"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.dcmt_version() == 120
    assert ctypes.sizeof(L.JointParams) == 20 and ctypes.sizeof(L.JointTables) == 1792 == api.JOINT_TABLES_DTYPE.itemsize
    assert [(f[0], getattr(L.JointParams, f[0]).offset) for f in L.JointParams._fields_] == [("radius", 0), ("flags", 4), ("min_weight", 8),
                                                                                               ("valid_thresh", 12), ("max_depth", 16)]
    assert (L.JointTables.w_space.offset, L.JointTables.w_guide.offset) == (0, 256)
    assert [api.JOINT_TABLES_DTYPE.fields[n][1] for n in ("w_space", "w_guide")] == [0, 256]
    assert (L.JOINT_FILL, L.JOINT_SMOOTH) == (1, 2)
    p = L.JointParams()
    lib.dcmt_default_joint_params(ctypes.byref(p))
    lib.dcmt_default_joint_params(None)
    assert (p.radius, p.flags, p.min_weight, p.valid_thresh, p.max_depth) == (6, L.JOINT_FILL, 1, float(f32(0.1)), 100.0)
    assert bytes(p) == bytes(api.make_joint_params())
    sup = api.make_support_params()                                  # valid_thresh and max_depth are the support call's defaults
    assert (p.valid_thresh, p.max_depth) == (sup.valid_thresh, sup.max_depth)
    assert J.DEFAULTS == dict(radius=p.radius, fill=True, smooth=False, min_weight=p.min_weight, valid_thresh=0.1, max_depth=p.max_depth)
    assert api.make_joint_tables().tobytes() == api.make_joint_tables(p.radius, **J.SIGMAS).tobytes()
    q = api.make_joint_params(radius=9, smooth=True, min_weight=2 ** 32 - 1, valid_thresh=0.0625, max_depth=16384)
    assert (q.radius, q.flags, q.min_weight, q.valid_thresh, q.max_depth) == (9, 3, 2 ** 32 - 1, 0.0625, 16384.0)
    assert api.make_joint_params(fill=False, smooth=True).flags == 2 and api.make_joint_params(radius=1).radius == 1
    for kw in (dict(radius=0), dict(radius=-1), dict(radius=10), dict(radius=1.5), dict(radius=2 ** 31), dict(radius=True), dict(fill=False),
               dict(min_weight=0), dict(min_weight=-1), dict(min_weight=2 ** 32), dict(min_weight=1.5),
               dict(valid_thresh=0.06), dict(valid_thresh=0.0), dict(valid_thresh=-1.0), dict(valid_thresh=float("nan")), dict(valid_thresh=float("inf")),
               dict(max_depth=0.05), dict(max_depth=16385.0), dict(max_depth=float("inf")), dict(max_depth=float("nan")), dict(valid_thresh=5.0, max_depth=4.0)):
        with pytest.raises(ValueError):
            api.make_joint_params(**kw)
    with pytest.raises(TypeError):
        api.make_joint_params(max_radius=1)
    # the tables: refused radii and sigmas, by the C call and by the wrapper
    t = L.JointTables()
    for args in ((0, 3.0, 10.0), (10, 3.0, 10.0), (-1, 3.0, 10.0), (6, 0.0, 10.0), (6, -1.0, 10.0), (6, 3.0, 0.0), (6, float("nan"), 10.0),
                 (6, 3.0, float("inf")), (6, float("-inf"), 10.0)):
        ctypes.memset(ctypes.byref(t), 0xA5, ctypes.sizeof(t))
        assert lib.dcmt_make_joint_tables(args[0], args[1], args[2], ctypes.byref(t)) == L.E_INVALID and bytes(t) == b"\xa5" * 1792, args
        with pytest.raises(ValueError):
            api.make_joint_tables(*args)
    assert lib.dcmt_make_joint_tables(6, 3.0, 10.0, None) == L.E_INVALID
    # without a context every argument check is moot: refused before anything touches a device
    assert lib.dcmt_joint_bilateral_dev(None, None, None, 1, None, None, 4, 4, 1, ctypes.byref(p), None, None) == L.E_INVALID
    assert lib.dcmt_joint_bilateral(None, None, 16, None, 4, 1, None, None, 16, 4, 4, ctypes.byref(p), None) == L.E_INVALID
    for name in ("joint_bilateral_fill", "make_joint_params", "make_joint_tables", "JOINT_TABLES_DTYPE"):
        assert getattr(pkg, name) is getattr(api, name) and name in pkg.__all__
    for name in ("joint_bilateral_dev", "joint_bilateral"):
        assert hasattr(api.Context, name)
