"""LiDAR-guided stereo matching (dcmt_sgm_guided_dev; include/dcmt.h, step 2b) without a GPU: the two restatements of
tests/sgm_guided_restatement.py against each other over shapes, disparity counts, both path counts, every guide kind and the weight /
cap grid; the hint rule on hostile bit patterns; the settings that must change nothing; the bound paths * (6375 + p2 + cap), which the
comb attains at 65500 and 65400; two conditions of usefulness on the restatement alone -- true hints find more of a flat patch, wrong
hints do not overrule texture; the launch plan (tests/plan_sgm_guided_test.cpp); exports, the Python surface and its ValueErrors."""
import ctypes
import functools
import struct

import numpy as np
import pytest

import sgm_guided_restatement as G
import sgm_paths_restatement as P
import sgm_restatement as R
from depth_completion_mt_amd import _lib as L
from test_plan import _build_and_run

SHAPES = [(1, 1), (1, 9), (9, 1), (6, 6), (7, 19)]
DISPARITIES = [16, 64, 128]
# (paths, p1, p2, weight, cap): nothing, the defaults, a cap that binds at once, and the largest sum the path count allows
GRID = {4: [(200, 800, 0, 0), (200, 800, 100, 1000), (200, 800, 1000, 100), (5000, 5000, 5000, 5000)],
        8: [(200, 800, 0, 0), (200, 800, 100, 1000), (200, 800, 1000, 100), (900, 900, 900, 900)]}


@functools.lru_cache(maxsize=None)
def pair(rows, cols):
    out = R.shifted_pair(rows, cols, 900 + rows + cols, shift=min(3, cols - 1)) if cols >= 5 else R.random_pair(rows, cols, 900 + rows + cols)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cost(rows, cols, D):
    C = R.literal_volumes(*pair(rows, cols), D, 0, 0)[0]
    assert np.array_equal(C, R.vectorised_volumes(*pair(rows, cols), D, 0, 0)[0])
    C.setflags(write=False)
    return C


@pytest.mark.parametrize("D", DISPARITIES)
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_restatements_agree(rows, cols, D):
    """Every guide kind at the default weight and cap; the whole weight / cap grid on the dense and the hostile guide (at D = 16 on
    every kind)."""
    left, right = pair(rows, cols)
    C = cost(rows, cols, D)
    for name, guide in G.guide_kinds(rows, cols, D).items():
        assert np.array_equal(np.array(G.literal_hints(guide, G.BF, D)), G.vectorised_hints(guide, G.BF, D)), name
        for paths in (4, 8):
            for p1, p2, weight, cap in GRID[paths]:
                if (weight, cap) != (100, 1000) and D > 16 and name not in ("dense", "hostile"):
                    continue
                C1, S1 = G.literal_volumes(left, right, guide, D, p1, p2, paths, weight, cap, C=C)
                C2, S2 = G.vectorised_volumes(left, right, guide, D, p1, p2, paths, weight, cap)
                assert np.array_equal(C1, C2) and np.array_equal(S1, S2), (name, paths, p1, p2, weight, cap)
                a, b = R.literal_select(S1, 10, 1), R.vectorised_select(S2, 10, 1)
                assert np.array_equal(a, b) and ((a == R.INVALID) | ((a >= 0) & (a <= 16 * (D - 1)))).all()


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def test_the_hint_rule_on_hostile_bits():
    for D in DISPARITIES:
        for bits in G.HOSTILE_BITS:
            z = np.array([bits], np.uint32).view(np.float32)
            want = G.vectorised_hints(z.reshape(1, 1), G.BF, D)[0, 0]
            assert G.literal_hint(bits, G.BF, D) == want
            # NaN, +-inf, negatives, both zeros: none.  The denormals and the least normal number are finite and > 0, but their
            # quotient overflows or lands beyond the range: none either.  The greatest finite number: the hint 0.
            assert want == (0 if bits == 0x7F7FFFFF else -1), hex(bits)
        inside, outside = G.boundary_depths(D)
        assert G.literal_hint(_bits(inside), G.BF, D) == D - 1 and G.literal_hint(_bits(outside), G.BF, D) == -1
        with np.errstate(over="ignore"):
            t = np.float32(np.float32(G.BF / outside) + np.float32(0.5))
        assert t == np.float32(D), (D, t)                     # exactly D, not beyond it: "<" is what refuses it
        assert G.literal_hint(_bits(1e30), G.BF, D) == 0 and G.literal_hint(_bits(1e-30), G.BF, D) == -1
        for d in (1, D // 2, D - 1):
            assert G.literal_hint(_bits(G.depth_for(d)), G.BF, D) == d
        assert G.literal_hint(_bits(G.depth_for(D)), G.BF, D) == -1 and G.literal_hint(_bits(G.depth_for(D + 40)), G.BF, D) == -1
        # rounding to nearest: q = h + 0.5 goes up, just under it stays
        assert G.literal_hint(_bits(np.float32(G.BF / np.float32(3.75))), G.BF, D) == 4 and G.literal_hint(_bits(np.float32(G.BF / np.float32(3.25))), G.BF, D) == 3
    # a product that overflowed: q is infinite for every depth, no pixel is hinted
    assert G.literal_hint(_bits(5.0), float("inf"), 64) == -1
    assert (G.vectorised_hints(np.full((2, 2), 5.0, np.float32), np.float32(np.inf), 64) == -1).all()


@pytest.mark.parametrize("paths", [4, 8])
def test_settings_that_change_nothing(paths):
    left, right = pair(7, 19)
    D = 16
    want = P.vectorised_volumes(left, right, D, 200, 800, paths)
    want16 = P.vectorised(left, right, paths=paths, num_disparities=D)
    kinds = G.guide_kinds(7, 19, D)
    for guide, weight, cap in ((kinds["dense"], 0, 1000), (kinds["dense"], 100, 0), (kinds["zero"], 100, 1000), (None, 100, 1000)):
        for volumes, run in ((G.vectorised_volumes, G.vectorised), (G.literal_volumes, G.literal)):
            got = volumes(left, right, guide, D, 200, 800, paths, weight, cap)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            d16, depth = run(left, right, guide, paths, weight, cap, num_disparities=D)
            assert np.array_equal(d16, want16[0]) and np.array_equal(depth.view(np.uint32), want16[1].view(np.uint32))
    # ... and the dense guide at the defaults does change something here
    assert not np.array_equal(G.vectorised_volumes(left, right, kinds["dense"], D, 200, 800, paths)[1], want[1])


@pytest.mark.parametrize("paths,penalty,bound", [(4, 5000, 65500), (8, 900, 65400)])
def test_the_comb_attains_the_bound(paths, penalty, bound):
    """comb_pair(12, 48, 16) with a hint of 0 on every pixel and weight = cap = p1 = p2: S reaches paths * (6375 + p2 + cap)."""
    left, right = R.comb_pair(12, 48, 16)
    guide = np.full((12, 48), G.FAR, np.float32)
    assert (G.vectorised_hints(guide, G.BF, 16) == 0).all()
    C, S = G.vectorised_volumes(left, right, guide, 16, penalty, penalty, paths, penalty, penalty)
    assert int(C.max()) == 6375 + penalty and int(S.max()) == bound == paths * (6375 + 2 * penalty)
    assert np.array_equal(G.literal_volumes(left, right, guide, 16, penalty, penalty, paths, penalty, penalty)[1], S)
    with pytest.raises(AssertionError):
        G.params(paths, penalty, penalty + 1, p2=penalty)
    with pytest.raises(AssertionError):
        G.params(paths, 10001, 0)
    assert G.params(paths, 100, 10 ** 6, guided=False)["p2"] == 800          # without a guide the two integers are not looked at


# ---- what the guide is for ------------------------------------------------------------------------------------------------------------
def _found(d16, truth):
    return int(((d16 >= 0) & ((d16 >> 4) == truth)).sum())


def test_true_hints_find_more_of_a_flat_patch():
    """A condition on the restatement, not a measurement.  flat_scene seeds 0..3, D = 16, default parameters, a return at the true
    disparity 6 on every 4th row and 8th column, weight 100, cap 1000: the pixels of disp16[13:27, 43:77] at disparity 6, in sum
    over the seeds, must be strictly more with the guide than without, for four paths and for eight (715 against 641 and 860 against
    808 when this was written; with four paths the guide is ahead on every seed)."""
    guide = G.flat_grid_guide(6)
    assert (G.vectorised_hints(guide, G.BF, 16)[2::4, 3::8] == 6).all() and (guide > 0).sum() == 10 * 15
    for paths in (4, 8):
        plain, guided = [], []
        for seed in range(4):
            left, right = P.flat_scene(seed)
            plain.append(_found(P.vectorised(left, right, paths=paths, num_disparities=16)[0][13:27, 43:77], 6))
            guided.append(_found(G.vectorised(left, right, guide, paths, 100, 1000, num_disparities=16)[0][13:27, 43:77], 6))
        print(f"{paths} paths, pixels of the flat patch at the true disparity, seeds 0..3: unguided {plain} = {sum(plain)}, guided {guided} = {sum(guided)}")
        assert sum(guided) > sum(plain), (paths, plain, guided)


def test_wrong_hints_do_not_overrule_texture():
    """The same grid with every return at disparity 12 where the truth is 6, four paths: on the textured pixels outside [8:32, 38:82]
    and right of column 8, over seeds 0..3, the guided matcher finds at least 99 in every 100 of what the unguided one finds (12076
    against 12035 when this was written)."""
    guide = G.flat_grid_guide(12)
    assert (G.vectorised_hints(guide, G.BF, 16)[2::4, 3::8] == 12).all()
    textured = np.ones((40, 120), bool)
    textured[8:32, 38:82] = False
    textured[:, :8] = False
    plain = guided = 0
    for seed in range(4):
        left, right = P.flat_scene(seed)
        a = R.vectorised(left, right, num_disparities=16)[0]
        b = G.vectorised(left, right, guide, 4, 100, 1000, num_disparities=16)[0]
        plain += int(((a >= 0) & ((a >> 4) == 6) & textured).sum())
        guided += int(((b >= 0) & ((b >> 4) == 6) & textured).sum())
    print(f"textured pixels at the true disparity under wrong hints, seeds 0..3: unguided {plain}, guided {guided}")
    assert 100 * guided >= 99 * plain, (plain, guided)


# ---- the plan, the ABI, the Python surface --------------------------------------------------------------------------------------------
def test_plans(tmp_path):
    _build_and_run(tmp_path, "plan_sgm_guided_test")
    _build_and_run(tmp_path, "plan_sgm_paths_test")          # the earlier programs, as they are, against the changed header
    _build_and_run(tmp_path, "plan_sgm_test")


def test_exports_surface_and_refusals_without_a_device():
    import inspect
    from depth_completion_mt_amd import api
    lib = L.lib()
    for name in ("dcmt_sgm_guided_dev", "dcmt_sgm_guided"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert ctypes.sizeof(L.SgmParams) == 32                  # the guide's integers are arguments, not fields
    assert api.SGM_GUIDE_WEIGHT == G.GUIDE_WEIGHT == 100 and api.SGM_GUIDE_CAP == G.GUIDE_CAP == 1000
    for fn, key in ((api.Context.sgm_dev, "d_guide"), (api.Context.sgm, "guide"), (api.stereo_sgm, "guide")):
        sig = inspect.signature(fn).parameters
        assert sig[key].default is None and sig["guide_weight"].default == 100 and sig["guide_cap"].default == 1000 and sig["paths"].default == 4
    made = inspect.signature(api.make_sgm_params).parameters
    assert "paths" not in made and not [k for k in made if "guide" in k]
    p = api.make_sgm_params()
    # without a context every argument check is moot: refused before anything touches a device
    assert lib.dcmt_sgm_guided_dev(None, 16, 32, 128, 48, 64, 4, 4, 1, ctypes.byref(p), 4, 100, 1000, 4096, 1 << 20, None) == L.E_INVALID
    assert lib.dcmt_sgm_guided_dev(None, 16, 32, None, 48, 64, 4, 4, 1, ctypes.byref(p), 8, 100, 1000, 4096, 1 << 20, None) == L.E_INVALID
    assert lib.dcmt_sgm_guided(None, None, 4, None, 4, None, 16, 4, 4, ctypes.byref(p), None, 8, None, 16, 4, 100, 1000) == L.E_INVALID
    grey, guide = np.zeros((4, 8), np.uint8), np.ones((4, 8), np.float32)
    bad = [dict(guide_weight=-1), dict(guide_weight=10001), dict(guide_weight=1.5), dict(guide_weight=True), dict(guide_cap=-1), dict(guide_cap=0.5),
           dict(guide_cap=9201), dict(paths=8, guide_cap=1001), dict(paths=8, p2=801), dict(p2=9001), dict(p2=10000, p1=0, guide_cap=1),
           dict(baseline=float("nan")), dict(focal=0.0), dict(baseline=-1.0), dict(focal=float("inf")), dict(paths=5), dict(paths=8, p2=1801, guide_cap=0)]
    for kw in bad:                                           # before any call: no device is needed to be told
        with pytest.raises(ValueError):
            api.stereo_sgm(grey, grey, guide=guide, **kw)
    # without a guide the two integers are not looked at: what is raised is the missing device, not a ValueError
    for kw in (dict(guide_weight=-1), dict(guide_cap=10 ** 6), dict(paths=8, guide_cap=1001)):
        try:
            api.stereo_sgm(grey, grey, **kw)
        except ValueError as e:                              # pragma: no cover
            pytest.fail(f"{kw}: {e}")
        except Exception:
            pass
