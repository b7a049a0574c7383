"""The Gaussian that ignores holes (DCMT_BLUR_GAUSSIAN_VALID) without a GPU: the two restatements of its definition
(tests/gauss_valid_restatement.py) agree bit for bit, the definition's stated consequences hold, the finish repairs the border of
the region the cascade without extrapolation completes, the dispatch plans it (tests/plan_gauss_valid_test.cpp), and the string
reaches dcmt_params."""
import numpy as np
import pytest

import gauss_valid_restatement as GV
import no_extrapolate_restatement as NE
import occlusion_restatement as OR
from conftest import assert_bit_equal, bits
from oracle import np_restatement as N
from test_plan import _build_and_run

f32 = np.float32
SHAPES = [(1, 1), (1, 2), (2, 1), (1, 65), (17, 1), (5, 3), (33, 70)]


def _planes():
    """(name, plane): random planes with 40 % holes of every shape, with NaN among them at some, and the adversarial planes"""
    out = [(f"holes {r}x{c}", GV.holes_plane(r, c, 31 * r + c)) for r, c in SHAPES]
    out += [(f"nan {r}x{c}", GV.nan_plane(r, c, 7 * r + c)) for r, c in ((5, 3), (33, 70))]
    out += list(NE.adversarial_planes().items())
    inf = GV.holes_plane(9, 11, 5)
    inf[4, 5] = np.inf
    out.append(("inf", inf))
    return out


PLANES = _planes()


@pytest.mark.parametrize("name,x", PLANES, ids=[n for n, _ in PLANES])
def test_restatements_agree(name, x):
    assert_bit_equal(GV.gv_arrays(x), GV.gv_loop(x), name)


def test_restatements_agree_at_another_threshold():
    x = GV.holes_plane(17, 23, 3, lo=0.05, hi=2.0)
    assert_bit_equal(GV.gv_arrays(x, 0.7), GV.gv_loop(x, 0.7), "thr 0.7")
    assert (bits(GV.gv_arrays(x, 0.7)) != bits(GV.gv_arrays(x))).any()


@pytest.mark.parametrize("name,x", PLANES, ids=[n for n, _ in PLANES])
def test_consequences_of_the_definition(name, x):
    y = GV.gv_arrays(x)
    v = GV.valid(x)
    num, den = GV.num_den(x)
    # at a valid pixel the centre tap alone gives 0.375^2; den is a multiple of 1/256
    assert (den[v] >= f32(0.140625)).all()
    assert np.array_equal(den * 256, np.round(den * 256)) and den.max(initial=0) <= 1
    # where all 25 taps are valid the Gaussian's bits
    one = v & (den == f32(1.0))
    with np.errstate(invalid="ignore"):
        g = N.gaussian5(x)
    assert np.array_equal(bits(y)[one], bits(g)[one])
    # an invalid pixel comes back bit for bit
    assert np.array_equal(bits(y)[~v], bits(x)[~v])
    # no NaN out of a NaN-free input (the invalid pixels that ARE NaN come back as they are, and only they)
    assert np.array_equal(np.isnan(y), np.isnan(x))
    # a valid result within [min, max] of its valid taps, up to the rounding of the 16 f32 operations that make it: each adds at
    # most 2^-24 relative to a sum of non-negative terms that never exceeds the largest tap
    R, C = x.shape
    if R >= 3 and C >= 3 and np.isfinite(x[v]).all():
        idx = lambda n: np.array([GV._reflect101(i, n) for i in range(-2, n + 2)])      # noqa: E731
        xv = np.where(v, x, np.nan)[np.ix_(idx(R), idx(C))]
        win = np.stack([xv[r:r + R, c:c + C] for r in range(5) for c in range(5)])
        with np.errstate(all="ignore"), np.testing.suppress_warnings() as sup:
            sup.filter(RuntimeWarning)
            lo, hi = np.nanmin(win, 0), np.nanmax(win, 0)
        margin = (16 * 2.0 ** -24) * hi.astype(np.float64)
        yy = y.astype(np.float64)
        assert (yy[v] >= lo[v] - margin[v]).all() and (yy[v] <= hi[v] + margin[v]).all(), name


def test_hole_free_plane_is_the_gaussian():
    x = NE.adversarial_planes()["fully valid"]
    assert_bit_equal(GV.gv_arrays(x), N.gaussian5(x), "hole-free")


def test_constant_region_with_holes_stays_within_the_rounding():
    """Not bit for bit: num and den round differently.  The bound is the [min, max] one with min = max."""
    c = f32(90.3)
    x = np.full((33, 70), c)
    x[GV.holes_plane(33, 70, 9) == 0] = 0
    y = GV.gv_arrays(x)
    v = GV.valid(x)
    assert (np.abs(y[v].astype(np.float64) - float(c)) <= 16 * 2.0 ** -24 * float(c)).all()
    assert (bits(y)[v] != bits(x)[v]).any()


# ---- the scene of the issue: what each finish does to the border of the region that extrapolate=False completes -----------------
@pytest.fixture(scope="module")
def scene():
    sparse, _ = OR.lidar_scene(boxes=False)
    V, U = np.mgrid[0:OR.ROWS, 0:OR.COLS]
    rays = np.stack([(U - OR.CX) / OR.F, (V - OR.CY) / OR.F, np.ones(U.shape)], -1).reshape(-1, 3)
    truth = OR._cast(np.zeros(3), rays, False).reshape(OR.ROWS, OR.COLS)
    x9 = NE.restatement_numpy(sparse, "as_compiled", "none", 9)
    region = x9 >= NE.THR
    out = {"none": NE.restatement_numpy(sparse, "as_compiled", "none", 11), "gaussian": NE.restatement_numpy(sparse, "as_compiled", "gaussian", 11),
           "gaussian_valid": GV.no_extrapolate(sparse)}
    err = {k: np.abs(v.astype(np.float64) - truth)[region] for k, v in out.items()}
    return sparse, x9, region, err


def test_scene_border_pixels(scene):
    _, x9, region, err = scene
    assert int(region.sum()) == 250139
    _, den = GV.num_den(x9)
    assert int((region & (den < 1)).sum()) == 2930               # valid pixels with at least one invalid tap
    assert int((err["gaussian"] > 5.0).sum()) == 1504
    assert int((err["gaussian_valid"] > 5.0).sum()) == 0
    assert int((err["none"] > 5.0).sum()) == 0


def test_scene_rmse(scene):
    _, _, _, err = scene
    rmse = {k: float(np.sqrt(np.mean(e * e))) for k, e in err.items()}
    assert rmse["gaussian_valid"] < rmse["none"] < rmse["gaussian"], rmse
    assert abs(rmse["gaussian_valid"] - 0.2832) < 5e-4 and abs(rmse["gaussian"] - 1.4693) < 5e-4 and abs(rmse["none"] - 0.4926) < 5e-4, rmse


def test_cascade_finishes():
    x = NE.random_plane(33, 70, 4)
    for k0 in ("as_compiled", "diamond"):
        x9 = NE.restatement_numpy(x, k0, "none", 9)
        assert (x9 < NE.THR).any() and (x9 >= NE.THR).any()
        assert_bit_equal(GV.no_extrapolate(x, k0, 9), x9, "stop_after = MEDIAN5 ignores the blur")
        assert_bit_equal(GV.no_extrapolate(x, k0, 10), GV.gv_loop(x9), "X10")
        assert_bit_equal(GV.no_extrapolate(x, k0, 11), N.invert(GV.gv_loop(x9)), "X11")
    # the extrapolating cascade: the Gaussian's bits where the loop converges
    y, info = GV.extrapolating(x)
    assert_bit_equal(y, N.img_completion(x), "converged")
    assert (N.img_completion(x, stop_after=9) >= NE.THR).all()


def test_plans(tmp_path):
    """tests/plan_gauss_valid_test.cpp against the headers alone"""
    _build_and_run(tmp_path, "plan_gauss_valid_test")


def test_params_and_abi():
    from depth_completion_mt_amd import _lib as L
    from depth_completion_mt_amd import api
    assert L.BLUR_GAUSSIAN_VALID == 5
    assert api.make_params(blur_type="gaussian_valid").blur == L.BLUR_GAUSSIAN_VALID
    assert api.make_params(blur_type="gaussian_valid", extrapolate=False).flags & L.FLAG_NO_EXTRAPOLATE
    assert api.make_params().blur == L.BLUR_GAUSSIAN                                    # the default stays the reference's
    assert api.make_params(blur_type="gaussian-valid").blur == L.BLUR_NONE              # any other string: no blur, as before
    lib = L.lib()
    for name in ("dcmt_gaussian5_valid_dev", "dcmt_gaussian5_valid"):
        assert name in L.EXPORTS and hasattr(lib, name)
