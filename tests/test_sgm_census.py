"""The census matching cost of the stereo matcher (dcmt_sgm_cost_dev with DCMT_SGM_COST_CENSUS; include/dcmt.h, steps 1c and 2c) without a
GPU: the two restatements of tests/sgm_census_restatement.py against each other over frames narrower than the census window and the
box, both path counts, with and without a guide, on six kinds of pair; two answers known by hand; three conditions of usefulness on
the restatement alone -- under a halved exposure census finds what absolute differences lose; the launch plan
(tests/plan_sgm_census_test.cpp); exports, the Python surface, its ValueErrors and the calls it makes."""
import ctypes
import functools
import inspect
import os
import subprocess

import numpy as np
import pytest

import sgm_census_restatement as CR
import sgm_guided_restatement as G
import sgm_restatement as R
from conftest import ROOT
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api
from test_plan import _build_and_run

FRAMES = [(1, 1), (1, 7), (7, 1), (3, 3), (6, 11)]      # in 3 x 3 the census window and the box are both wider than the frame
KINDS = ("random", "shifted", "stripes", "comb", "constant", "quantised")
D = 16


def pair_of(kind, rows, cols):
    seed = 700 + 13 * rows + cols
    if kind == "random":
        return R.random_pair(rows, cols, seed)
    if kind == "shifted":
        return R.shifted_pair(rows, cols, seed, shift=min(3, cols - 1))
    if kind == "stripes":
        return R.stripes_pair(rows, cols)
    if kind == "comb":
        return R.comb_pair(rows, cols, D)
    if kind == "constant":
        return CR.constant_pair(rows, cols)
    if kind == "quantised":
        return CR.quantised_pair(rows, cols, seed)
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cols", FRAMES)
def test_restatements_agree(rows, cols, kind):
    """C, S and disp16, element for element, with 4 and 8 paths, with and without a dense guide."""
    left, right = pair_of(kind, rows, cols)
    KL, KR = np.array(CR.literal_codes(left), dtype=np.int64), CR.vectorised_codes(left)
    # the two forms order the bits differently; the number of darker neighbours is the same
    assert np.array_equal(CR.popcount24(KL), CR.popcount24(KR)) and KL.max() < 1 << 24 and KR.max() < 1 << 24
    C = CR.literal_cost(left, right, D)
    assert np.array_equal(C, CR.vectorised_cost(left, right, D)) and (C % 10 == 0).all() and C.max() <= 6000
    for guide in (None, G.guide_kinds(rows, cols, D)["dense"]):
        for paths in (4, 8):
            C1, S1 = CR.literal_volumes(left, right, guide, D, 200, 800, paths, C=C)
            C2, S2 = CR.vectorised_volumes(left, right, guide, D, 200, 800, paths)
            assert np.array_equal(C1, C2) and np.array_equal(S1, S2), (kind, paths, guide is not None)
            a, b = R.literal_select(S1, 10, 1), R.vectorised_select(S2, 10, 1)
            assert np.array_equal(a, b) and ((a == R.INVALID) | ((a >= 0) & (a <= 16 * (D - 1)))).all()
            if guide is None:
                assert np.array_equal(C1, C)
    if kind == "constant":                                      # every code is 0, C is 0, and the lowest d wins where x - d >= 0
        assert not KL.any() and not C.any()
        d16 = CR.vectorised(left, right, num_disparities=D)[0]
        assert (d16[:, 0] == 0).all() and ((d16 == 0) | (d16 == R.INVALID)).all()
    if kind == "quantised" and rows * cols > 9:                 # a non-strict comparison would set most of these bits
        pad = np.pad(left.astype(int), 2, mode="edge")
        equal = sum(int((pad[i:i + rows, j:j + cols] == left).sum()) for i in range(5) for j in range(5)) - rows * cols
        assert equal > 0.2 * 24 * rows * cols
        assert int(CR.popcount24(KL).sum()) + equal + int(CR.popcount24(CR.vectorised_codes(255 - left)).sum()) == 24 * rows * cols


def test_the_strict_maximum_has_every_bit_set():
    image = np.full((5, 5), 100, np.uint8)
    image[2, 2] = 101
    for codes in (np.array(CR.literal_codes(image), dtype=np.int64), CR.vectorised_codes(image)):
        assert codes[2, 2] == 0xFFFFFF
        assert np.count_nonzero(codes) == 1                     # equal neighbours set nothing: the comparison is strict
    image[2, 2] = 99                                            # the strict minimum: its own code is 0, all 24 neighbours see it
    codes = CR.vectorised_codes(image)
    assert codes[2, 2] == 0 and np.count_nonzero(codes) == 24 and (CR.popcount24(codes).sum() >= 24)


@pytest.mark.parametrize("paths", [4, 8])
def test_a_constant_offset_changes_nothing(paths):
    """Two images that differ by a constant offset without clipping have the same codes, and with them C, S and disp16."""
    rng = np.random.default_rng(11)
    wide = rng.integers(40, 200, (7, 19 + 3), dtype=np.uint8)
    left, right = np.ascontiguousarray(wide[:, :19]), np.ascontiguousarray(wide[:, 3:])
    brighter = (right + 55).astype(np.uint8)
    assert int(brighter.max()) == int(right.max()) + 55
    for codes in (lambda a: np.array(CR.literal_codes(a), dtype=np.int64), CR.vectorised_codes):
        assert np.array_equal(codes(right), codes(brighter))
    for volumes in (CR.literal_volumes, CR.vectorised_volumes):
        a, b = volumes(left, right, None, D, 200, 800, paths), volumes(left, brighter, None, D, 200, 800, paths)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(CR.vectorised(left, right, paths=paths, num_disparities=D)[0], CR.vectorised(left, brighter, paths=paths, num_disparities=D)[0])
    assert not np.array_equal(R.vectorised_volumes(left, right, D, 200, 800)[0], R.vectorised_volumes(left, brighter, D, 200, 800)[0])


# ---- what the census cost is for --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exposure_table():
    """{exposure: (absolute differences, census)}: the pixels of box_scene(48, 160, 32, 7) found at the default parameters."""
    left, right, truth = R.box_scene(48, 160, 32, 7)
    table = {}
    for name, expose in CR.EXPOSURES.items():
        r = np.ascontiguousarray(expose(right)).astype(np.uint8)
        table[name] = (CR.found(R.vectorised(left, r, num_disparities=32)[0], truth), CR.found(CR.vectorised(left, r, num_disparities=32)[0], truth))
    return table


def test_census_finds_what_a_halved_exposure_loses():
    """Conditions on the restatement, not measurements.  Of 7680 pixels, when this was written (absolute differences, census):
    as generated 6664, 7120; 0.6 v + 40: 6347, 7119; v // 2: 4805, 7122; max(v - 60, 0): 5091, 7004; gamma 1.8: 5562, 7113."""
    table = exposure_table()
    for name, (absdiff, census) in table.items():
        print(f"{name}: absolute differences {absdiff}, census {census}")
    plain, halved = table["as generated"], table["v // 2"]
    assert 10 * halved[1] >= 13 * halved[0], halved              # with right // 2, census finds at least 1.3 times the pixels
    assert halved[1] >= plain[0], (halved, plain)               # ... and at least what absolute differences find on the untouched pair
    assert plain[1] >= plain[0], plain                          # on the untouched pair census finds no fewer


# ---- the plan, the ABI, the Python surface ----------------------------------------------------------------------------------------------
def test_plans(tmp_path):
    _build_and_run(tmp_path, "plan_sgm_census_test")
    _build_and_run(tmp_path, "plan_sgm_guided_test")         # the earlier programs, as they are, against the changed header
    _build_and_run(tmp_path, "plan_sgm_paths_test")
    _build_and_run(tmp_path, "plan_sgm_test")


def test_shim_driver_compiles_against_the_cv_mat_stand_in(tmp_path):
    """tests/mock_opencv/shim_sgm_census_test.cpp, which tests/test_gpu_sgm_census.py links and runs, against the stand-in with 16-bit
    elements; stereo_sgm_cost stands inside the guard of its siblings."""
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "mock_opencv", "with_16s"),
                    "-c", os.path.join(ROOT, "tests", "mock_opencv", "shim_sgm_census_test.cpp"), "-o", str(tmp_path / "shim_sgm_census_test.o")],
                   check=True, capture_output=True)
    hdr = open(os.path.join(ROOT, "include", "img_completion.h")).read()
    at = hdr.index("inline void stereo_sgm_cost(")
    assert hdr.index("#ifdef CV_16SC1") < hdr.index("inline void stereo_sgm_guided(") < at < hdr.index("#endif", at)
    assert "#endif" not in hdr[hdr.index("inline void stereo_sgm_guided("):at]


def test_exports_surface_and_refusals_without_a_device():
    lib = L.lib()
    for name in ("dcmt_sgm_cost_dev", "dcmt_sgm_cost"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert len(lib.dcmt_sgm_cost_dev.argtypes) == len(lib.dcmt_sgm_guided_dev.argtypes) + 1 == 17
    assert len(lib.dcmt_sgm_cost.argtypes) == len(lib.dcmt_sgm_guided.argtypes) + 1 == 18
    assert lib.dcmt_sgm_cost_dev.argtypes[13] is ctypes.c_int and lib.dcmt_sgm_cost.argtypes[17] is ctypes.c_int
    assert ctypes.sizeof(L.SgmParams) == 32                  # the cost is an argument, not a field
    assert api.SGM_COSTS == {"absdiff": 0, "census": 1}
    for fn in (api.Context.sgm_dev, api.Context.sgm, api.stereo_sgm):
        sig = inspect.signature(fn).parameters
        assert sig["cost"].default == "absdiff" and sig["paths"].default == 4 and sig["guide_weight"].default == 100
    assert "cost" not in inspect.signature(api.make_sgm_params).parameters
    hdr = open(os.path.join(ROOT, "include", "dcmt.h")).read()
    assert "#define DCMT_SGM_COST_ABSDIFF 0" in hdr and "#define DCMT_SGM_COST_CENSUS 1" in hdr
    p = api.make_sgm_params()
    # without a context every argument check is moot: refused before anything touches a device
    for cost in (0, 1, 2, -1):
        assert lib.dcmt_sgm_cost_dev(None, 16, 32, None, 48, 64, 4, 4, 1, ctypes.byref(p), 4, 0, 0, cost, 4096, 1 << 20, None) == L.E_INVALID
        assert lib.dcmt_sgm_cost(None, None, 4, None, 4, None, 16, 4, 4, ctypes.byref(p), None, 8, None, 16, 4, 100, 1000, cost) == L.E_INVALID
    grey, guide = np.zeros((4, 8), np.uint8), np.ones((4, 8), np.float32)
    for bad in ("Census", "sad", "", None, 0, 1, True, b"census", ("census",)):        # before any call: no device is needed to be told
        with pytest.raises(ValueError):
            api.stereo_sgm(grey, grey, cost=bad)
        with pytest.raises(ValueError):
            api.stereo_sgm(grey, grey, guide=guide, paths=8, cost=bad)
    # it combines with the other keywords as they combine today: their ValueErrors are still raised with census
    for kw in (dict(paths=5), dict(paths=8, p2=1801), dict(guide=guide, guide_cap=9201), dict(guide=guide, paths=8, guide_cap=1001),
               dict(guide=guide, guide_weight=-1), dict(guide=guide, baseline=float("nan"))):
        with pytest.raises(ValueError):
            api.stereo_sgm(grey, grey, cost="census", **kw)


class _Recorder:
    """Stands in for the library: every call is recorded and answers DCMT_OK; the dcmt_default_* fillers are the library's own."""

    def __init__(self, real):
        self.calls, self.real = [], real

    def __getattr__(self, name):
        if name.startswith("dcmt_default_"):
            return getattr(self.real, name)

        def call(*args):
            self.calls.append((name, args))
            return L.OK
        return call


def test_absdiff_makes_the_calls_of_today_and_census_the_new_one(monkeypatch):
    fake = _Recorder(L.lib())
    monkeypatch.setattr(L, "lib", lambda: fake)
    ctx = object.__new__(api.Context)
    ctx._h = None
    left, right = R.shifted_pair(6, 11, 3)
    guide = np.ones((6, 11), np.float32)
    for kw in (dict(), dict(cost="absdiff")):
        fake.calls.clear()
        ctx.sgm(left, right, **kw)
        ctx.sgm(left, right, paths=8, **kw)
        ctx.sgm(left, right, guide=guide, **kw)
        ctx.sgm(left, right, guide=guide, paths=8, guide_weight=7, guide_cap=9, **kw)
        assert [name for name, _ in fake.calls] == ["dcmt_sgm", "dcmt_sgm_paths", "dcmt_sgm_guided", "dcmt_sgm_guided"]
        assert len(fake.calls[0][1]) == 12 and fake.calls[1][1][-1] == 8 and fake.calls[2][1][-3:] == (4, 100, 1000) and fake.calls[3][1][-3:] == (8, 7, 9)
    fake.calls.clear()
    ctx.sgm(left, right, cost="census")
    ctx.sgm(left, right, cost="census", paths=8, guide_weight=-3, guide_cap=-3)          # without a guide the integers are not looked at
    ctx.sgm(left, right, cost="census", guide=guide, paths=8, guide_weight=7, guide_cap=9)
    ctx.sgm(left, right, cost="census", speckle_window=200, speckle_range=2)
    names = [name for name, _ in fake.calls]
    assert names == ["dcmt_sgm_cost", "dcmt_sgm_cost", "dcmt_sgm_cost", "dcmt_sgm_cost", "dcmt_filter_speckles"]
    assert all(len(args) == 18 for name, args in fake.calls if name == "dcmt_sgm_cost")
    assert fake.calls[0][1][5:7] == (None, 0) and fake.calls[0][1][-4:] == (4, 0, 0, 1)
    assert fake.calls[1][1][5:7] == (None, 0) and fake.calls[1][1][-4:] == (8, 0, 0, 1)
    assert fake.calls[2][1][5] is not None and fake.calls[2][1][6] == 44 and fake.calls[2][1][-4:] == (8, 7, 9, 1)
