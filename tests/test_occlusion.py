"""The occlusion filter of projected LiDAR returns without a GPU: the two restatements of tests/occlusion_restatement.py against each
other (the definition of include/dcmt.h pixel by pixel on Python ints, and as shifted maxima over a zero-padded code plane), on f32
planes and on the payload; what is no return, ties, radii of 0; that the filter does its job on the scene of boxes in front of a
wall, on the restatement alone; the launch plan (tests/plan_occlusion_test.cpp, built against the headers alone); the struct layout,
the defaults, the exports and the refusals that need no device."""
import ctypes

import numpy as np
import pytest

import occlusion_restatement as R
from depth_completion_mt_amd import _lib as L
from test_plan import _build_and_run

f32, u16, u32 = np.float32, np.uint16, np.uint32
SIZES = [(1, 1), (1, 65), (17, 1), (5, 3), (33, 130), (24, 70)]
GRID = [{}, dict(rx=0, ry=0), dict(rx=8, ry=16, tol_code=0), dict(rx=8, ry=0, tol_code=100), dict(rx=0, ry=16, tol_code=1 << 20),
        dict(rx=2, ry=1, valid_thresh=0.5, max_depth=20.0, tol_code=50)]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def both(plane, what, **kw):
    """The two restatements agree bit for bit; returns (out, removed)."""
    lit, vec = R.literal_occlusion(plane, **kw), R.shifted_occlusion(plane, **kw)
    assert same(lit[0], vec[0]) and lit[1] == vec[1], f"{what}: {lit[1]} against {vec[1]} removed"
    assert lit[0].dtype == plane.dtype and lit[1] == int((lit[0].view(u32 if plane.dtype == f32 else u16) != plane.view(u32 if plane.dtype == f32 else u16)).sum()), what
    return lit


@pytest.mark.parametrize("rows,cols", SIZES)
def test_restatements_agree(rows, cols):
    removed = 0
    for seed in range(2):
        for density in (0.1, 0.6):
            z, v = R.sparse_plane(rows, cols, density, seed), R.payload_plane(rows, cols, density, seed)
            for kw in GRID:
                removed += both(z, f"{rows}x{cols} seed {seed} density {density} {kw}", **kw)[1]
                removed += both(v, f"{rows}x{cols} payload seed {seed} density {density} {kw}", **kw)[1]
            both(v, f"{rows}x{cols} payload, another scale", scale=0.01)
    assert removed > 0 or rows * cols < 50


def test_what_is_no_return_and_keeps_its_bits():
    """NaN, +-inf, -0.0, negatives and depths outside [valid_thresh, max_depth] are no returns: they hide nothing, are never removed
    and keep their bits, beside a return at 2 m that would hide anything."""
    bad = np.array(R.SPECIALS + (np.nextafter(f32(0.1), f32(0)), np.nextafter(f32(100), f32(1000))), f32)
    z = np.zeros((3, len(bad)), f32)
    z[0] = bad
    out, n = both(z, "specials alone")
    assert n == 0 and same(out, z)
    z[1] = 2.0
    z[2] = 100.0                                                  # the bound itself is a return: hidden behind 2 m
    out, n = both(z, "specials beside returns")
    assert same(out[:2], z[:2]) and n == len(bad) and not out[2].view(u32).any()
    assert R.literal_codes(np.array([[0.1, 100.0]], f32))[0] == [655360, 655]    # both bounds are returns
    # a huge "depth" is no return: it hides nothing (its code would be 0 anyway) and a tiny one neither
    z = np.array([[1e30, 50.0, 0.05, 50.0, np.inf]], f32)
    assert both(z, "no occluders")[1] == 0
    # the payload: 0 and what lies outside the bounds after the ingest
    v = np.array([[0, 25, 26, 25600, 25601, 65535, 512]], u16)
    assert R.literal_codes(v)[0] == [0, 0, int(np.rint(f32(65536) / (f32(26) / f32(256)))), 655, 0, 0, 32768]
    out, n = both(v, "payload bounds")
    assert n == 1 and out.tolist() == [[0, 25, 26, 0, 25601, 65535, 512]]


def test_ties_are_kept():
    """m - w == tol_code keeps the return, tol_code + 1 removes it."""
    for tol in (0, 655, 5000):
        z, go, stay = R.with_ties(100, 200, tol)
        assert len(go) >= 5 and len(stay) >= 10
        out, n = both(z, f"ties at {tol}", tol_code=tol)
        assert n == len(go) and all(out[p] == 0 for p in go) and all(out[p] == z[p] for p in stay)
    # tol_code = 2^20: nothing is ever removed (the largest code is 2^20, the smallest 4)
    z = np.array([[0.0625, 16384.0]], f32)
    assert R.literal_codes(z, valid_thresh=0.0625, max_depth=16384.0)[0] == [1 << 20, 4]
    assert both(z, "extremes", valid_thresh=0.0625, max_depth=16384.0, tol_code=1 << 20)[1] == 0
    assert both(z, "extremes", valid_thresh=0.0625, max_depth=16384.0, tol_code=(1 << 20) - 5)[1] == 1


def test_radii_of_zero_and_empty_planes_remove_nothing():
    for rows, cols in SIZES:
        z = R.sparse_plane(rows, cols, 0.5, 3)
        out, n = both(z, "radii 0", rx=0, ry=0, tol_code=0)
        assert n == 0 and same(out, z)
        empty = np.zeros((rows, cols), f32)
        empty.reshape(-1)[::3] = np.resize(np.array(R.SPECIALS, f32), len(empty.reshape(-1)[::3]))
        out, n = both(empty, "no returns", tol_code=0)
        assert n == 0 and same(out, empty)
    out, n = both(np.zeros((9, 9), u16), "empty payload")
    assert n == 0 and not out.any()


def test_window_reach_and_the_clipped_border():
    """An occluder exactly rx / ry away removes the return, one further does not; the window is clipped, not wrapped or replicated."""
    for rx, ry in ((3, 6), (8, 16), (1, 0), (0, 2)):
        z = np.zeros((40, 40), f32)
        z[20, 20] = 50.0
        for dy, dx, hit in ((ry, rx, True), (-ry, -rx, True), (ry + 1, 0, False), (0, rx + 1, False), (ry, 0, True), (0, -rx, True)):
            if (dy, dx) == (0, 0):
                continue
            zz = z.copy()
            zz[20 + dy, 20 + dx] = 2.0
            out, n = both(zz, f"reach {rx} {ry} {dy} {dx}", rx=rx, ry=ry)
            assert n == int(hit) and (out[20, 20] == 0) == hit
    z = np.zeros((8, 30), f32)
    z[3, 29], z[4, 0], z[0, 5], z[7, 5] = 2.0, 50.0, 50.0, 2.0   # the end of one row and the start of the next; the first and the last row
    assert both(z, "no wrap", rx=3, ry=0)[1] == 0 and both(z, "no wrap", rx=8, ry=2)[1] == 0


def test_a_removed_return_still_hides_others():
    """A hides B, B hides C, A does not reach C: every decision is taken on the input, so C goes although B went."""
    z = np.zeros((1, 12), f32)
    z[0, 0], z[0, 3], z[0, 6] = 2.0, 10.0, 50.0
    out, n = both(z, "chain", rx=3, ry=0)
    assert n == 2 and out[0].tolist() == [2.0] + [0.0] * 11
    once = R.shifted_occlusion(z, rx=3, ry=0)[0]
    again = R.shifted_occlusion(once, rx=3, ry=0)
    assert again[1] == 0                                          # and what an order-dependent filter would give differs:
    seq = z.copy()
    seq[0, 3] = 0                                                 # B removed first, C decided on the result
    assert R.shifted_occlusion(seq, rx=3, ry=0)[1] == 0


def _rates(boxes=True, **kw):
    sparse, see_through = R.lidar_scene(boxes, **({"lidar": kw.pop("lidar")} if "lidar" in kw else {}))
    out, n = R.shifted_occlusion(sparse, **kw)
    gone = (out == 0) & (sparse > 0)
    assert n == gone.sum()
    return int((sparse > 0).sum()), int(see_through.sum()), int((gone & see_through).sum()), int((gone & ~see_through).sum())


def test_the_filter_does_its_job_on_the_scene():
    """Ground, wall and three boxes seen by a LiDAR beside the camera (occlusion_restatement.lidar_scene), at the defaults.  Measured on
    the restatement: 16198 returns, 412 of them see-through; removed 412 of 412 and 172 of the other 15786 (1.09 %: the band of true
    background within the window of a silhouette edge, the filter's known cost).  Without the boxes: 16206 returns, 0 removed at
    tol_code 655 and at 500; tol_code 328 removes 3602 ground returns, as the derivation of the default predicts.  With the LiDAR at
    (0.3, -0.3, -0.27): 1345 of 1345 see-through returns and 143 of the 16616 others."""
    returns, st, gone_st, gone_other = _rates()
    print(f"[occlusion] scene: {returns} returns, {st} see-through; removed {gone_st} of them and {gone_other} of the other {returns - st}")
    assert st >= 300
    assert gone_st >= 0.99 * st
    assert gone_other <= 0.02 * (returns - st)
    creturns, cst, cgone_st, cgone_other = _rates(boxes=False)
    print(f"[occlusion] control: {creturns} returns, {cst} see-through; removed {cgone_st + cgone_other}")
    assert cst == 0 and cgone_st + cgone_other == 0
    assert sum(_rates(boxes=False, tol_code=500)[2:]) == 0
    low = _rates(boxes=False, tol_code=328)
    far = _rates(lidar=(0.3, -0.3, -0.27))
    print(f"[occlusion] control at tol_code 328: {sum(low[2:])} removed; LiDAR at (0.3, -0.3, -0.27): {far}")
    assert sum(low[2:]) > 1000                                    # half the default eats the ground
    assert far[1] > st and far[2] >= 0.99 * far[1] and far[3] <= 0.02 * (far[0] - far[1])


def test_the_plan_as_compiled(tmp_path):
    _build_and_run(tmp_path, "plan_occlusion_test")


def test_layout_defaults_exports_and_refusals_without_a_device():
    from depth_completion_mt_amd import api
    import depth_completion_mt_amd as pkg
    lib = L.lib()
    for name in ("dcmt_default_occlusion_params", "dcmt_sparse_occlusion_dev", "dcmt_sparse_occlusion_u16_dev", "dcmt_sparse_occlusion"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert ctypes.sizeof(L.OcclusionParams) == 20
    assert [(f[0], getattr(L.OcclusionParams, f[0]).offset) for f in L.OcclusionParams._fields_] == [("rx", 0), ("ry", 4), ("tol_code", 8), ("valid_thresh", 12), ("max_depth", 16)]
    p = L.OcclusionParams()
    lib.dcmt_default_occlusion_params(ctypes.byref(p))
    lib.dcmt_default_occlusion_params(None)
    assert (p.rx, p.ry, p.tol_code, p.valid_thresh, p.max_depth) == (3, 6, 655, float(f32(0.1)), 100.0)
    assert bytes(p) == bytes(api.make_occlusion_params())
    assert {k: R.DEFAULTS[k] for k in ("rx", "ry", "tol_code")} == dict(rx=p.rx, ry=p.ry, tol_code=p.tol_code)
    planes = api.make_planes_params()                            # valid_thresh and max_depth are the planes' defaults
    assert (p.valid_thresh, p.max_depth) == (planes.valid_thresh, planes.max_depth)
    q = api.make_occlusion_params(rx=8, ry=16, inv_depth_tol=16.0, valid_thresh=0.0625, max_depth=16384)
    assert (q.rx, q.ry, q.tol_code, q.valid_thresh, q.max_depth) == (8, 16, 1 << 20, 0.0625, 16384.0)
    assert api.make_occlusion_params(inv_depth_tol=0.01).tol_code == 655 == round(65536 * 0.01) and api.make_occlusion_params(inv_depth_tol=0).tol_code == 0
    assert api.make_occlusion_params(rx=0, ry=0, tol_code=500).tol_code == 500
    for kw in (dict(rx=-1), dict(rx=9), dict(rx=1.5), dict(rx=2 ** 31), dict(ry=-1), dict(ry=17), dict(inv_depth_tol=-0.001), dict(inv_depth_tol=16.001),
               dict(inv_depth_tol=float("nan")), dict(inv_depth_tol=float("inf")), dict(tol_code=-1), dict(tol_code=(1 << 20) + 1), dict(tol_code=5, inv_depth_tol=0.01),
               dict(valid_thresh=0.06), dict(valid_thresh=0.0), dict(valid_thresh=-1.0), dict(valid_thresh=float("nan")), dict(valid_thresh=float("inf")),
               dict(max_depth=0.05), dict(max_depth=16385.0), dict(max_depth=float("inf")), dict(max_depth=float("nan")), dict(valid_thresh=5.0, max_depth=4.0)):
        with pytest.raises(ValueError):
            api.make_occlusion_params(**kw)
    with pytest.raises(TypeError):
        api.make_occlusion_params(blur=1)
    # without a context every argument check is moot: refused before anything touches a device
    assert lib.dcmt_sparse_occlusion_dev(None, None, None, 4, 4, 1, ctypes.byref(p), None, None) == L.E_INVALID
    assert lib.dcmt_sparse_occlusion_u16_dev(None, None, 1.0 / 256.0, None, 4, 4, 1, ctypes.byref(p), None, None) == L.E_INVALID
    assert lib.dcmt_sparse_occlusion(None, None, 16, None, 16, 4, 4, ctypes.byref(p), None) == L.E_INVALID
    assert pkg.filter_occluded_returns is api.filter_occluded_returns and pkg.make_occlusion_params is api.make_occlusion_params
    for name in ("sparse_occlusion_dev", "sparse_occlusion"):
        assert hasattr(api.Context, name)
    for name in ("filter_occluded_returns", "make_occlusion_params"):
        assert name in pkg.__all__
