"""The stereo matcher (dcmt_sgm_dev) without a GPU: the two restatements of tests/sgm_restatement.py against each other over the
parameter grid, plain block matching at p1 = p2 = 0, the bound on S on adversarial pairs, a sanity condition on the restatement (it
finds a known scene; it finds every targeted disparity of the pairs and staircases the GPU tests use, and its two forms agree at
D = 128 with winners at 63, 64, 100 and 127), the launch plan (tests/plan_sgm_test.cpp, built against the headers alone), the refusals that need no device
and the ABI."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import sgm_restatement as R
from depth_completion_mt_amd import _lib as L
from test_plan import _build_and_run

f32 = np.float32
PENALTIES = [(0, 0), (200, 800), (10000, 10000), (0, 10000)]
UNIQUENESS = [0, 10, 100]
DISP12 = [-1, 0, 1]
# (D, rows, cols, maker): up to about 12 x 40; fewer rows than the block, fewer columns than D, one row, one pixel
TINY = [(16, 12, 40, "shifted"), (16, 3, 33, "random"), (32, 7, 33, "shifted"), (64, 5, 40, "random"), (16, 1, 1, "random"), (32, 1, 21, "shifted"),
        (16, 9, 2, "random")]


def pair(maker, rows, cols, D):
    if maker == "shifted":
        return R.shifted_pair(rows, cols, 10 + rows + cols)
    if maker == "stripes":
        return R.stripes_pair(rows, cols)
    if maker == "comb":
        return R.comb_pair(rows, cols, D)
    return R.random_pair(rows, cols, 20 + rows + cols)


@functools.lru_cache(maxsize=None)
def volumes(which, maker, rows, cols, D, p1, p2):
    left, right = pair(maker, rows, cols, D)
    return (R.literal_volumes if which == "literal" else R.vectorised_volumes)(left, right, D, p1, p2)


@pytest.mark.parametrize("D,rows,cols,maker", TINY)
def test_restatements_agree(D, rows, cols, maker):
    valid = 0
    for p1, p2 in PENALTIES:
        C1, S1 = volumes("literal", maker, rows, cols, D, p1, p2)
        C2, S2 = volumes("vectorised", maker, rows, cols, D, p1, p2)
        assert np.array_equal(C1, C2) and np.array_equal(S1, S2), (D, rows, cols, p1, p2)
        for u, lr in itertools.product(UNIQUENESS, DISP12):
            a, b = R.literal_select(S1, u, lr), R.vectorised_select(S2, u, lr)
            assert a.dtype == b.dtype == np.int16
            assert np.array_equal(a, b), f"{D} {rows}x{cols} p1 {p1} p2 {p2} uniqueness {u} disp12 {lr}: first at {tuple(np.argwhere(a != b)[0])}"
            assert ((a == R.INVALID) | ((a >= 0) & (a <= 16 * (D - 1)))).all()
            valid += int((a >= 0).sum())
    assert valid > 0
    if maker == "shifted" and rows >= 7:      # a pair with an answer: the default parameters find the shift on most pixels
        left, right = pair(maker, rows, cols, D)
        d16, depth = R.literal(left, right, num_disparities=D)
        d16v, depthv = R.vectorised(left, right, num_disparities=D)
        assert np.array_equal(d16, d16v) and np.array_equal(depth.view(np.uint32), depthv.view(np.uint32))
        assert (np.abs(d16[:, 8:-4] - 48) <= 8).mean() > 0.8          # 3 px, to half a pixel
        assert depth.dtype == f32 and ((depth > 0) == (d16 > 0)).all() and depth.max() <= 100.0


def test_without_penalties_it_is_block_matching():
    for D, rows, cols, maker in TINY[:4]:
        C, S = volumes("vectorised", maker, rows, cols, D, 0, 0)
        assert np.array_equal(S, 4 * C)
        C, S = volumes("literal", maker, rows, cols, D, 0, 0)
        assert np.array_equal(S, 4 * C)


def test_the_bound_on_S_on_adversarial_pairs():
    """The stripes against a constant image: every disparity costs the same, so no path pays a penalty and S = 4 C whatever p2 is
    (20400 at most: 20 of 25 taps on a 255 stripe).  The comb is the pair that separates uint16 from int16: one cheap band of
    disparities, every other one at 25 * 255 on every pixel of every path, so with p2 = 10000 the paths saturate and S reaches
    the bound 4 * (6375 + 10000) = 65500 and never passes it."""
    for p1, p2 in PENALTIES + [(10000, 10000), (200, 10000)]:
        for value in (0, 255):
            left, right = R.stripes_pair(12, 40, value)
            C, S = R.vectorised_volumes(left, right, 32, p1, p2)
            assert np.array_equal(S, 4 * C) and S.max() == 20400
    left, right = R.stripes_pair(6, 20)
    assert np.array_equal(R.literal_volumes(left, right, 16, 0, 10000)[1], R.vectorised_volumes(left, right, 16, 0, 10000)[1])
    reached = {}
    for D, rows, cols in ((16, 24, 96), (32, 24, 96), (64, 24, 140)):
        left, right = R.comb_pair(rows, cols, D)
        for p1, p2 in ((0, 10000), (200, 10000), (10000, 10000)):
            C, S = R.vectorised_volumes(left, right, D, p1, p2)
            assert C.max() == 6375 and S.max() <= R.S_BOUND
            reached[D, p1] = int(S.max())
    assert all(v > 50000 for v in reached.values()), reached            # well above 32767
    assert reached[32, 0] == R.S_BOUND and reached[64, 0] == R.S_BOUND    # the bound is attained
    left, right = R.comb_pair(6, 36, 16)
    C1, S1 = R.literal_volumes(left, right, 16, 0, 10000)
    C2, S2 = R.vectorised_volumes(left, right, 16, 0, 10000)
    assert np.array_equal(S1, S2) and S1.max() > 32767


@pytest.mark.parametrize("rows,cols,D,seed", [(16, 70, 16, 3), (24, 96, 32, 0), (24, 96, 32, 1), (37, 150, 64, 2)])
def test_the_restatement_finds_a_known_scene(rows, cols, D, seed):
    """A condition on the restatement, not a measurement: noise with a background at disparity 5 and a box at min(12, D - 3), default
    parameters: at least 0.85 of the pixels valid, at least 0.99 of the valid ones within a pixel of the truth."""
    left, right, truth = R.box_scene(rows, cols, D, seed)
    d16, depth = R.vectorised(left, right, num_disparities=D)
    valid = d16 >= 0
    within = np.abs(d16[valid] / 16.0 - truth[valid]) <= 1.0
    print(f"{rows}x{cols} D {D} seed {seed}: valid {valid.mean():.4f}, within a pixel {within.mean():.4f}")
    assert valid.mean() >= 0.85 and within.mean() >= 0.99
    want = R.depth_of(d16)
    assert np.array_equal(depth.view(np.uint32), want.view(np.uint32)) and (depth[d16 <= 0] == 0).all()


@pytest.mark.parametrize("D", list(R.TARGET_SHIFTS))
def test_the_restatement_finds_every_targeted_disparity(D):
    """Conditions on the inputs of the GPU tests, from the restatement alone, at the default parameters: the shifted pairs, exact
    and half, have their answer at the chosen disparity (the ends of the range, 63 | 64 at D = 128) on at least 500 / 200 pixels,
    the half pairs show at least 12 of the 16 fractions, and every band of the staircase is found."""
    found = {(shift, half): R.vectorised(*R.target_pair(D, shift, half), num_disparities=D)[0] for shift, half in R.target_pairs(D)}
    R.assert_targets_found(D, found)
    left, right, truth = R.staircase_scene(R.STAIR_ROWS, R.staircase_cols(D), D, 5)
    assert sorted(set(truth.ravel().tolist())) == R.staircase_disparities(D)
    assert {63, 64} <= set(R.staircase_disparities(128)) and R.staircase_disparities(16) == [0, 1, 14, 15]
    R.assert_staircase_found(D, R.vectorised(left, right, num_disparities=D)[0], truth)


HIGH = [("exact", lambda: R.shifted_pair(4, 140, 31, 127)), ("half", lambda: R.shifted_pair(4, 140, 32, 64, half=True)),
        ("staircase", lambda: R.staircase_scene(4, 140, 128, 33, disparities=(1, 63, 64, 100))[:2])]


@pytest.mark.parametrize("name", [h[0] for h in HIGH])
def test_restatements_agree_on_high_disparities(name):
    """literal against vectorised on 4 x (D + 12) at D = 128 with winners far above the 12 of the TINY frames: the second half of the
    disparity range, d* = 63 | 64, d* = D - 1."""
    left, right = dict(HIGH)[name]()
    C1, S1 = R.literal_volumes(left, right, 128, 200, 800)
    C2, S2 = R.vectorised_volumes(left, right, 128, 200, 800)
    assert np.array_equal(C1, C2) and np.array_equal(S1, S2)
    winners = set()
    for u, lr in ((10, 1), (0, -1), (100, 0)):
        a, b = R.literal_select(S1, u, lr), R.vectorised_select(S2, u, lr)
        assert np.array_equal(a, b), f"{name} uniqueness {u} disp12 {lr}: first at {tuple(np.argwhere(a != b)[0])}"
        winners |= set((a[a >= 0] >> 4).tolist())
    want = {"exact": {127}, "half": {64}, "staircase": {63, 64, 100}}[name]
    assert want <= winners, (name, sorted(winners))


def test_depth_formula():
    d16 = np.array([[-16, 0, 1, 16, 83, 84, 16 * 127 + 8]], np.int16)
    z = R.depth_of(d16)
    bf = f32(0.54) * f32(9.597910e+02)
    assert z.dtype == f32 and z[0, 0] == 0 and z[0, 1] == 0 and z[0, 2] == 100.0 and z[0, 3] == 100.0
    assert z[0, 4] == f32(bf / (f32(83) / f32(16))) < 100.0 and z[0, 5] == f32(bf / f32(5.25))
    assert R.depth_of(d16, max_depth=50.0)[0, 4] == 50.0 and R.depth_of(d16, baseline=0.1, focal=100.0)[0, 3] == f32(f32(0.1) * f32(100.0))


def test_plans(tmp_path):
    _build_and_run(tmp_path, "plan_sgm_test")


def test_abi_defaults_workspace_and_refusals_without_a_device():
    from depth_completion_mt_amd import api
    import depth_completion_mt_amd as pkg
    lib = L.lib()
    for name in ("dcmt_default_sgm_params", "dcmt_sgm_workspace_bytes", "dcmt_sgm_dev", "dcmt_sgm"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert ctypes.sizeof(L.SgmParams) == 32 and [f[0] for f in L.SgmParams._fields_] == list(R.DEFAULTS)
    assert L.SgmParams.baseline.offset == 20 and L.SgmParams.max_depth.offset == 28
    p = api.make_sgm_params()
    for k, v in R.DEFAULTS.items():
        assert f32(getattr(p, k)) == f32(v), k
    q = api.make_sgm_params(num_disparities=128, p1=0, p2=10000, uniqueness=100, disp12_max_diff=-1, focal=80.0)
    assert (q.num_disparities, q.p1, q.p2, q.uniqueness, q.disp12_max_diff, q.focal, f32(q.baseline)) == (128, 0, 10000, 100, -1, 80.0, f32(0.54))
    lib.dcmt_default_sgm_params(None)                        # no-op
    # what the C call refuses of its parameters, make_sgm_params raises on
    for bad in (dict(num_disparities=0), dict(num_disparities=8), dict(num_disparities=24), dict(num_disparities=144), dict(num_disparities=-16),
                dict(p1=-1), dict(p1=801), dict(p2=10001), dict(p1=300, p2=200), dict(uniqueness=-1), dict(uniqueness=101),
                dict(baseline=0.0), dict(baseline=-0.54), dict(focal=np.nan), dict(focal=np.inf), dict(max_depth=0.0), dict(max_depth=np.nan),
                dict(p1=1.5), dict(num_disparities=2 ** 40)):
        with pytest.raises(ValueError):
            api.make_sgm_params(**bad)
    # ... except that the three floats are tested only for a call that writes the depth plane, as in C
    loose = api.make_sgm_params(for_depth=False, baseline=np.nan, focal=0.0, max_depth=-1.0)
    assert np.isnan(loose.baseline) and loose.focal == 0.0 and loose.max_depth == -1.0
    with pytest.raises(ValueError):
        api.make_sgm_params(for_depth=False, p2=10001)
    # the workspace: two uint16 volumes a frame; monotone in frames and at least frames x one frame
    wb = lib.dcmt_sgm_workspace_bytes
    one = wb(352, 1216, 64, 1)
    assert one == 2 * 2 * 352 * 1216 * 64 and one % 16 == 0 and api.sgm_workspace_bytes(352, 1216) == one
    sizes = [wb(352, 1216, 64, n) for n in range(1, 40)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])) and all(s >= n * one - 4096 for n, s in enumerate(sizes, 1))
    assert wb(375, 1242, 128, 65535) >= 65535 * wb(375, 1242, 128, 1) > 2 ** 42       # computed in 64 bits
    assert wb(1, 1, 16, 1) == 64 and wb(3, 5, 48, 2) == 2 * 4 * 3 * 5 * 48
    for bad in ((0, 8, 16, 1), (8, 0, 16, 1), (8, 8, 16, 0), (8, 8, 15, 1), (8, 8, 0, 1), (8, 8, 144, 1), (-1, 8, 16, 1), (8, 8, 16, -1)):
        assert wb(*bad) == 0, bad
    # without a context every argument check is moot: refused before anything touches a device
    assert lib.dcmt_sgm_dev(None, None, None, None, None, 4, 4, 1, ctypes.byref(p), None, 0, None) == L.E_INVALID
    assert lib.dcmt_sgm_dev(None, 16, 32, 48, 64, 4, 4, 1, ctypes.byref(p), 4096, 1 << 20, None) == L.E_INVALID
    assert lib.dcmt_sgm(None, None, 4, None, 4, 4, 4, ctypes.byref(p), None, 8, None, 16) == L.E_INVALID
    assert pkg.stereo_sgm is api.stereo_sgm and pkg.make_sgm_params is api.make_sgm_params
    for name in ("sgm_dev", "sgm"):
        assert hasattr(api.Context, name)
