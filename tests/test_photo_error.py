"""get_initial_error without a GPU: the two restatements of tests/photo_error_restatement.py against each other, the square root the
reference takes against the integer square root over every sum a window can give, the zero-error case, the truncation cases, the
launch plan (tests/plan_photo_error_test.cpp, built against the headers alone), the refusals that need no device and the ABI."""
import ctypes
import math

import numpy as np
import pytest

import photo_error_restatement as R
from depth_completion_mt_amd import _lib as L
from test_plan import _build_and_run

f32 = np.float32
SMALL = [(1, 1), (1, 9), (9, 1), (3, 5), (5, 7), (37, 131)]


def both(depth, left, right, what, **kw):
    """The two restatements agree; returns (err, stats)."""
    e1, s1 = R.literal(depth, left, right, **kw)
    e2, s2 = R.vectorised(depth, left, right, **kw)
    assert e1.dtype == e2.dtype == np.uint8 and s1.dtype == s2.dtype == np.uint64
    assert np.array_equal(e1, e2), f"{what}: {int((e1 != e2).sum())} pixels differ, first at {tuple(np.argwhere(e1 != e2)[0])}"
    assert np.array_equal(s1, s2), (what, s1, s2)
    valid, matches, nonzero, total = (int(v) for v in s1)
    assert nonzero <= valid <= depth.size and matches <= valid * (2 * kw.get("window", R.WINDOW)) ** 2 and nonzero <= total <= 255 * nonzero
    return e1, s1


@pytest.mark.parametrize("rows,cols", SMALL)
def test_restatements_agree(rows, cols):
    planes = {"random": R.random_depth(rows, cols, 5), "constant": R.constant_depth(rows, cols), "adversarial": R.adversarial_depth(rows, cols, 6)[0]}
    for n, (pname, depth) in enumerate(planes.items()):
        for window in (1, 2, 3, 4):
            iname = list(R.IMAGES)[(n + window) % 3] if rows * cols > 1000 else None
            for name in ([iname] if iname else list(R.IMAGES)):
                left, right = R.IMAGES[name](rows, cols)
                both(depth, left, right, f"{rows}x{cols} {pname} {name} window {window}", window=window)
    # other constants: a small disparity, so that most pixels of even the narrow frames are valid
    left, right = R.random_pair(rows, cols, 3)
    both(R.random_depth(rows, cols, 8), left, right, f"{rows}x{cols} small disparity", baseline=0.5, focal=1.0)


def test_the_square_root_is_the_integer_square_root():
    """Exhaustively, for every n in [0, 64 * 255^2] (a window of up to 8 x 8 taps): min(255, int(np.float32(math.sqrt(n)))) ==
    min(255, math.isqrt(n)) -- the reference's float e = sqrt(int), clamped and cast, against what the library computes."""
    n = np.arange(64 * 255 * 255 + 1, dtype=np.int64)
    root = np.sqrt(n.astype(np.float64))                    # math.sqrt: the correctly rounded f64 root
    assert root[12345] == math.sqrt(12345) and root[-1] == math.sqrt(int(n[-1]))
    as_reference = np.minimum(255, root.astype(f32).astype(np.int64))
    isqrt = np.floor(root).astype(np.int64)
    assert (isqrt * isqrt <= n).all() and ((isqrt + 1) * (isqrt + 1) > n).all()      # ... whose floor IS math.isqrt on this range
    for k in (0, 1, 2, 3, 4, 65024, 65025, 65026, 16 * 255 * 255, int(n[-1])):
        assert isqrt[k] == math.isqrt(k) and as_reference[k] == min(255, int(f32(math.sqrt(k))))
    assert np.array_equal(as_reference, np.minimum(255, isqrt))
    # the unclamped f32 root never crosses an integer either
    assert np.array_equal(root.astype(f32).astype(np.int64), isqrt)


@pytest.mark.parametrize("params,depth_value,shift", [(dict(baseline=0.5, focal=64.0), 4.0, 8), (dict(), None, 7)])
def test_zero_error_where_the_right_image_is_the_left_one_shifted(params, depth_value, shift):
    rows, cols, window = 12, 64, 2
    with np.errstate(all="ignore"):
        bf = f32(params.get("baseline", R.BASELINE)) * f32(params.get("focal", R.FOCAL))
    d = f32(depth_value) if depth_value is not None else R.depth_for_disparity(shift, bf)
    assert d is not None and f32(bf / d) == f32(shift)
    left, _ = R.random_pair(rows, cols, 21)
    right = np.roll(left, -shift, axis=1)                  # right[i][c - shift] = left[i][c]
    err, stats = both(np.full((rows, cols), d, f32), left, right, "shifted", window=window, **params)
    inner = err[:, shift + window:cols - window]
    assert inner.size > 0 and (inner == 0).all()
    assert int(stats[0]) == rows * (cols - shift - 1)      # valid: 0 < j - shift
    assert int(stats[1]) > 0
    # the counter-case: one more pixel of disparity, and the windows no longer match
    d1 = R.depth_for_disparity(shift + 1, bf)
    assert d1 is not None
    err1, stats1 = both(np.full((rows, cols), d1, f32), left, right, "shifted + 1", window=window, **params)
    assert (err1[1:, shift + 1 + window:cols - window] > 0).all() and int(stats1[2]) > 0 and int(stats1[3]) >= int(stats1[2])


def test_truncation_cases():
    cols = 9
    # the decision itself: toward zero, both bounds strict, nothing undefined converted
    assert R.target(f32(-0.5), cols) is None and R.target(f32(0.5), cols) is None          # (int) gives 0: pr > 0 fails
    assert R.target(f32(1.0), cols) == 1 and R.target(f32(1.999), cols) == 1
    assert R.target(f32(cols - 1), cols) == cols - 1 and R.target(f32(cols - 0.5), cols) == cols - 1
    assert R.target(f32(cols), cols) is None and R.target(f32(cols + 0.5), cols) is None
    for t in (np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 1e30, -1e30, -0.0, -3.0):
        assert R.target(f32(t), cols) is None
    assert R.target(f32(2.0 ** 31 - 128), 2 ** 31 - 1) == 2 ** 31 - 128
    # the same through a plane: baseline * focal = 0.5, so depth 1 is half a pixel of disparity and depth 0.5 a whole one
    kw = dict(baseline=0.5, focal=1.0, window=1)
    left, right = R.extremes_pair(2, cols)                  # every valid pixel with a kept tap reads 255
    for j, depth, t, valid in ((0, 1.0, -0.5, False), (1, 1.0, 0.5, False), (2, 0.5, 1.0, True), (1, 1e30, 1.0, True), (cols - 1, np.inf, cols - 1, True),
                               (cols - 1, 1e30, cols - 1, True), (0, np.inf, 0.0, False), (3, 0.25, 1.0, True), (3, 0.125, -1.0, False)):
        plane = np.zeros((2, cols), f32)
        plane[1, j] = depth
        with np.errstate(all="ignore"):
            assert f32(j) - f32(0.5) / f32(depth) == f32(t)
        err, stats = both(plane, left, right, f"t = {t} at column {j}", **kw)
        assert int(stats[0]) == (1 if valid else 0) and (err[1, j] == 255) == valid and int((err > 0).sum()) == (1 if valid else 0)
    # ... and the adversarial plane of the GPU test holds every case that a plane can hold, at the reference's constants
    plane, placed = R.adversarial_depth(37, 131, 6)
    assert set(placed) == set(R.T_TARGETS) | set(R.SPECIAL_VALUES)
    with np.errstate(all="ignore"):
        bf = f32(R.BASELINE) * f32(R.FOCAL)
        t_of = {k: f32(j) - bf / plane[i, j] for k, (i, j) in placed.items()}
    assert t_of["t=-0.5"] == -0.5 and t_of["t=0.5"] == 0.5 and t_of["t=1"] == 1.0 and t_of["t=cols-1"] == 130.0 and t_of["t<left"] == -3.0
    assert t_of["t=-inf"] == -np.inf and t_of["1e30"] == f32(placed["1e30"][1]) and np.isnan(t_of["nan"])
    left, right = R.extremes_pair(37, 131)
    err, _ = both(plane, left, right, "adversarial")
    for k, (i, j) in placed.items():
        inside = k in ("t=1", "t=cols-1", "+inf", "1e30") and R.target(t_of[k], 131) is not None
        assert (err[i, j] == 255) == inside, (k, i, j, err[i, j])
    assert err[placed["t=1"]] == 255 and err[placed["t=cols-1"]] == 255


def test_plans(tmp_path):
    _build_and_run(tmp_path, "plan_photo_error_test")


def test_refusals_without_a_device_and_the_abi():
    from depth_completion_mt_amd import api
    import depth_completion_mt_amd as pkg
    lib = L.lib()
    for name in ("dcmt_default_photo_error_params", "dcmt_photo_error_dev", "dcmt_photo_error_calib_dev", "dcmt_photo_error"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert ctypes.sizeof(L.PhotoErrorParams) == 12
    p = api.make_photo_error_params()
    assert (f32(p.baseline), f32(p.focal), p.window) == (f32(0.54), f32(9.597910e+02), 2)
    q = api.make_photo_error_params(baseline=0.5, window=4)
    assert (q.baseline, f32(q.focal), q.window) == (0.5, f32(9.597910e+02), 4)
    lib.dcmt_default_photo_error_params(None)               # no-op
    # without a context every argument check is moot: refused before anything touches a device
    assert lib.dcmt_photo_error_dev(None, None, None, None, 4, 4, 1, ctypes.byref(p), None, None, None) == L.E_INVALID
    assert lib.dcmt_photo_error_calib_dev(None, None, None, None, 4, 4, 1, ctypes.byref(p), None, None, None, None) == L.E_INVALID
    assert lib.dcmt_photo_error(None, None, 16, None, 4, None, 4, 4, 4, ctypes.byref(p), None, 4, None) == L.E_INVALID
    assert pkg.get_initial_error is api.get_initial_error and pkg.make_photo_error_params is api.make_photo_error_params
    for name in ("photo_error_dev", "photo_error_calib_dev", "photo_error"):
        assert hasattr(api.Context, name)
    assert api.PHOTO_STATS == R.STATS
