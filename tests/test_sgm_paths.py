"""Eight-path aggregation (dcmt_sgm_paths_dev) without a GPU: the two restatements of tests/sgm_paths_restatement.py against each other
over the parameter grid; S = 8 C without penalties; the bound 8 * (6375 + 1800) = 65400, which the comb attains; the wrapped walk of
k_sgm_diag, restated here from its definition, against the per-diagonal paths element for element -- the claim the kernel rests on; the
launch plan (tests/plan_sgm_paths_test.cpp); exports, the Python surface and its ValueErrors; and a condition of usefulness on the
restatement alone: on a flat patch inside texture, eight paths find the true disparity on more pixels than four."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import sgm_paths_restatement as P
import sgm_restatement as R
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd.api import SGM_MAX_P2_EIGHT_PATHS          # the library's limit: the penalty grid below runs up to it
from test_plan import _build_and_run

SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (5, 2), (6, 6), (7, 19), (23, 5), (12, 40)]
DISPARITIES = [16, 32, 64]
PENALTIES = [(0, 0), (200, 800), (1800, 1800), (0, 1800)]
assert SGM_MAX_P2_EIGHT_PATHS == P.MAX_P2 == max(p2 for _, p2 in PENALTIES)
UNIQUENESS = [0, 10, 100]
DISP12 = [-1, 0, 1]
# the shapes at which the wrapped walk was argued in the first place, and the ones above
WALK_SHAPES = sorted(set(SHAPES + [(6, 6), (8, 3), (3, 64), (17, 16)]))


@functools.lru_cache(maxsize=None)
def pair(rows, cols):
    out = R.shifted_pair(rows, cols, 700 + rows + cols, shift=min(3, cols - 1)) if cols >= 5 else R.random_pair(rows, cols, 700 + rows + cols)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cost(rows, cols, D):
    """C of pair(rows, cols), from both forms of tests/sgm_restatement.py (which tests/test_sgm.py holds against each other)."""
    C1 = R.literal_volumes(*pair(rows, cols), D, 0, 0)[0]
    C2 = R.vectorised_volumes(*pair(rows, cols), D, 0, 0)[0]
    assert np.array_equal(C1, C2)
    C1.setflags(write=False)
    return C1


@pytest.mark.parametrize("D", DISPARITIES)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_restatements_agree(rows, cols, D):
    left, right = pair(rows, cols)
    C = cost(rows, cols, D)
    for p1, p2 in PENALTIES:
        C1, S1 = P.literal_volumes(left, right, D, p1, p2, C=C)
        C2, S2 = P.vectorised_volumes(left, right, D, p1, p2)
        assert np.array_equal(C1, C2) and np.array_equal(S1, S2), (rows, cols, D, p1, p2)
        if (p1, p2) == (200, 800):      # the literal form's own four axis paths are those of tests/sgm_restatement.py
            assert np.array_equal(P.literal_volumes(left, right, D, p1, p2, paths=4, C=C)[1], R.vectorised_volumes(left, right, D, p1, p2)[1])
            assert np.array_equal(P.vectorised_volumes(left, right, D, p1, p2, paths=4)[1], R.vectorised_volumes(left, right, D, p1, p2)[1])
        for u, lr in itertools.product(UNIQUENESS, DISP12):
            a, b = R.literal_select(S1, u, lr), R.vectorised_select(S2, u, lr)
            assert a.dtype == b.dtype == np.int16
            assert np.array_equal(a, b), f"{D} {rows}x{cols} p1 {p1} p2 {p2} uniqueness {u} disp12 {lr}: first at {tuple(np.argwhere(a != b)[0])}"
            assert ((a == R.INVALID) | ((a >= 0) & (a <= 16 * (D - 1)))).all()


def test_chained_forms_agree_and_find_the_shift():
    left, right = pair(12, 40)
    d16, depth = P.literal(left, right, num_disparities=16)
    d16v, depthv = P.vectorised(left, right, num_disparities=16)
    assert np.array_equal(d16, d16v) and np.array_equal(depth.view(np.uint32), depthv.view(np.uint32))
    assert (np.abs(d16[:, 8:-4] - 48) <= 8).mean() > 0.8              # 3 px, to half a pixel
    four = P.vectorised(left, right, paths=4, num_disparities=16)[0]
    assert np.array_equal(four, R.vectorised(left, right, num_disparities=16)[0])
    with pytest.raises(AssertionError):
        P.params(8, p2=1801)
    assert P.params(4, p2=1801)["p2"] == 1801 and P.params(8, p1=1800, p2=1800)["p2"] == 1800


def test_without_penalties_the_sum_is_eight_times_the_cost():
    for rows, cols in SHAPES:
        C, S = P.vectorised_volumes(*pair(rows, cols), 16, 0, 0)
        assert np.array_equal(S, 8 * C), (rows, cols)
    C = cost(7, 19, 32)
    assert np.array_equal(P.literal_volumes(*pair(7, 19), 32, 0, 0, C=C)[1], 8 * C)


@pytest.mark.parametrize("D", [16, 64])
def test_the_comb_attains_the_bound(D):
    """All 255 against a comb with a tooth every D columns, p1 = p2 = 1800: every path of every direction saturates at C + p2 on some
    element, so S reaches 8 * (6375 + 1800) = 65400 and never passes it; with four paths the same pair reaches 4 * 8175 = 32700."""
    left, right = R.comb_pair(12, 3 * D, D)
    C, S = P.vectorised_volumes(left, right, D, 1800, 1800)
    assert C.max() == 6375 and int(S.max()) == P.S_BOUND == 65400
    assert int(P.vectorised_volumes(left, right, D, 1800, 1800, paths=4)[1].max()) == 32700
    assert int(R.vectorised_volumes(left, right, D, 1800, 1800)[1].max()) == 32700
    if D == 16:
        assert np.array_equal(P.literal_volumes(left, right, D, 1800, 1800)[1], S)


def test_the_stripes_never_pay_a_penalty():
    for p1, p2 in PENALTIES:
        for value in (0, 255):
            left, right = R.stripes_pair(12, 40, value)
            C, S = P.vectorised_volumes(left, right, 32, p1, p2)
            assert np.array_equal(S, 8 * C) and S.max() == 2 * 20400
    left, right = R.stripes_pair(6, 20)
    assert np.array_equal(P.literal_volumes(left, right, 16, 0, 1800)[1], P.vectorised_volumes(left, right, 16, 0, 1800)[1])


# ---- the wrapped walk -----------------------------------------------------------------------------------------------------------------
def wrapped_diagonals(C, p1, p2):
    """The diagonal part of S as k_sgm_diag computes it: for each orientation sx, wave w of cols visits pixel (y, (w + sx y) mod cols)
    for y = 0 .. rows - 1 going down, then the same pixels going up.  The path restarts on a walk's first pixel and wherever the
    previous pixel of the walk is not this pixel's diagonal predecessor inside the frame.  Returns (the sum, the lengths of the runs
    between restarts)."""
    rows, cols, D = C.shape
    c = C.tolist()
    S = [[[0] * D for _ in range(cols)] for _ in range(rows)]
    runs = []
    for sx in (1, -1):
        visits = np.zeros((rows, cols), np.int64)
        for w in range(cols):
            down = [(y, (w + sx * y) % cols) for y in range(rows)]
            for walk, dy in ((down, 1), (down[::-1], -1)):
                prev = last = None
                for y, x in walk:
                    visits[y, x] += 1
                    linked = last is not None and last == (y - dy, x - sx * dy) and 0 <= x - sx * dy < cols
                    if not linked:
                        cur = list(c[y][x])
                        runs.append(1)
                    else:
                        m = min(prev)
                        cur = [c[y][x][d] + min([prev[d], m + p2] + ([prev[d - 1] + p1] if d > 0 else []) + ([prev[d + 1] + p1] if d + 1 < D else [])) - m
                               for d in range(D)]
                        runs[-1] += 1
                    for d in range(D):
                        S[y][x][d] += cur[d]
                    prev, last = cur, (y, x)
        assert (visits == 2).all()                          # one orientation: every pixel once down and once up
    return np.array(S, dtype=np.int64), runs


@pytest.mark.parametrize("rows,cols", WALK_SHAPES)
def test_the_wrapped_walk_is_the_set_of_maximal_diagonals(rows, cols):
    D = 16
    C = cost(rows, cols, D).astype(np.int32)
    lengths = sorted(int(n) for n in P.diagonal_indices(rows, cols)[2].sum(axis=1))
    for p1, p2 in PENALTIES[1:]:
        got, runs = wrapped_diagonals(C, p1, p2)
        want = P.vectorised_diagonals(C, p1, p2)
        assert np.array_equal(got, want), (rows, cols, p1, p2, tuple(np.argwhere(got != want)[0]))
        assert sorted(runs) == sorted(4 * lengths)           # the runs are the frame's diagonals: each one in two orientations, both ways
    # ... and the penalties matter on this input: a walk that linked across a wrap, or restarted inside a diagonal, would be seen
    if rows > 1 and cols > 1:
        assert not np.array_equal(P.vectorised_diagonals(C, 200, 800), 4 * C)


# ---- the plan, the ABI, the Python surface --------------------------------------------------------------------------------------------
def test_plans(tmp_path):
    _build_and_run(tmp_path, "plan_sgm_paths_test")
    _build_and_run(tmp_path, "plan_sgm_test")                # the earlier program, as it is, against the changed header


def test_exports_surface_and_refusals_without_a_device():
    import inspect
    from depth_completion_mt_amd import api
    lib = L.lib()
    for name in ("dcmt_sgm_paths_dev", "dcmt_sgm_paths"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert ctypes.sizeof(L.SgmParams) == 32                  # the path count is an argument, not a field
    for fn in (api.Context.sgm_dev, api.Context.sgm, api.stereo_sgm):
        assert inspect.signature(fn).parameters["paths"].default == 4
    assert "paths" not in inspect.signature(api.make_sgm_params).parameters
    p = api.make_sgm_params()
    # without a context every argument check is moot: refused before anything touches a device
    for paths in (4, 8, 0, 5, 16):
        assert lib.dcmt_sgm_paths_dev(None, 16, 32, 48, 64, 4, 4, 1, ctypes.byref(p), paths, 4096, 1 << 20, None) == L.E_INVALID
        assert lib.dcmt_sgm_paths(None, None, 4, None, 4, 4, 4, ctypes.byref(p), None, 8, None, 16, paths) == L.E_INVALID
    grey = np.zeros((4, 8), np.uint8)
    for bad in (0, 5, 16, -8, 4.5, "8", True):               # before any call: no device is needed to be told
        with pytest.raises((ValueError, TypeError)):
            api.stereo_sgm(grey, grey, paths=bad)
    with pytest.raises(ValueError):
        api.stereo_sgm(grey, grey, paths=8, p2=1801)
    with pytest.raises(ValueError):
        api.stereo_sgm(grey, grey, paths=8, p1=200, p2=10000)
    with pytest.raises(ValueError):
        api.stereo_sgm(grey, grey, paths=4, p2=10001)
    assert api.SGM_MAX_P2_EIGHT_PATHS == P.MAX_P2 == 1800


# ---- what the diagonals are for -------------------------------------------------------------------------------------------------------
def test_eight_paths_find_more_of_a_flat_patch_than_four():
    """A condition on the restatement, not a measurement.  40 x 120 at true disparity 6, D = 16, default parameters: inside the flat
    patch the block cost says nothing, and the answer has to be carried in along the paths.  Over seeds 0..3, the pixels of
    disp16[13:27, 43:77] whose integer part is 6: eight paths must find strictly more than four (808 against 641 when this was
    written, eight ahead on every seed)."""
    found = {4: [], 8: []}
    for seed in range(4):
        left, right = P.flat_scene(seed)
        for paths in (4, 8):
            d16 = P.vectorised(left, right, paths=paths, num_disparities=16)[0]
            inner = d16[13:27, 43:77]
            found[paths].append(int(((inner >= 0) & ((inner >> 4) == 6)).sum()))
    print(f"pixels at the true disparity, seeds 0..3: four paths {found[4]}, eight paths {found[8]}")
    assert sum(found[8]) > sum(found[4]), found
