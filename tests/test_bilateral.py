"""The bilateral finish without a GPU: the numpy restatement of its statement (tests/bilateral_restatement.py), the launch plan of
k_bilateral5 and the cascade's plan with it (tests/plan_bilateral_test.cpp, built against the headers alone), the parameter mapping."""
import numpy as np
import pytest

import bilateral_restatement as B
from conftest import assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import synth
from oracle import oracle as O
from test_plan import _build_and_run

f32 = np.float32


def median_plane(rows, cols, seed=3, k0="as_compiled"):
    """The oracle's plane behind the 5x5 median: what the cascade hands to the filter."""
    return O.img_completion(synth.synth_frame(rows, cols, seed), O.default_params(k0=k0, blur="none", stop_after=9))


def noise_plane(rows=48, cols=64, seed=11):
    g = np.random.Generator(np.random.PCG64(seed))
    return g.uniform(-20.0, 100.0, (rows, cols)).astype(f32)


@pytest.mark.parametrize("name,plane", [("median 48x64", lambda: median_plane(48, 64)), ("median 33x70", lambda: median_plane(33, 70)),
                                        ("noise 48x64", noise_plane)])
def test_f32_restatement_stays_within_1e5_of_f64(name, plane):
    x = plane()
    want = B.restatement_f64(x)
    err = np.abs(B.restatement_f32(x).astype(np.float64) - want).max()
    naive = np.abs(B.naive_f32(x).astype(np.float64) - want).max()
    print(f"[bilateral] {name}: f32 difference form {err:.3g} m, naive form {naive:.3g} m from f64")
    assert err <= 1e-5
    assert B.restatement_f32(x).dtype == f32


def test_taps_weights_and_border():
    assert B.TAPS == [(-2, 0), (-1, -1), (-1, 0), (-1, 1), (0, -2), (0, -1), (0, 0), (0, 1), (0, 2), (1, -1), (1, 0), (1, 1), (2, 0)]
    gc, ws = B.constants()
    assert gc == f32(-0.5) / f32(2.25) and ws[0] == 1.0 and ws[1] == f32(np.exp(-1 / 8.0)) and ws[4] == f32(np.exp(-0.5))
    assert list(B.reflect101(np.arange(-2, 7), 5)) == [2, 1, 0, 1, 2, 3, 4, 3, 2]
    assert list(B.reflect101(np.arange(-2, 4), 2)) == [0, 1, 0, 1, 0, 1] and list(B.reflect101(np.arange(-2, 3), 1)) == [0] * 5


def test_constant_plane_comes_back_bit_for_bit():
    for v in (0.0, 7.25, 0.1, 99.999, -20.0):
        c = np.full((9, 13), v, f32)
        assert_bit_equal(B.restatement_f32(c), c, f"constant {v}")
    for shape in ((1, 1), (2, 2), (1, 70)):
        assert_bit_equal(B.restatement_f32(np.full(shape, 42.5, f32)), np.full(shape, 42.5, f32), f"constant {shape}")


def test_an_edge_survives_where_the_gaussian_smears_it():
    x = np.full((16, 32), 20.0, f32)
    x[:, 16:] = 60.0
    assert np.abs(B.restatement_f32(x) - x).max() <= 1e-6
    assert np.abs(O.gaussian5(x) - x).max() > 1.0


def test_invert_is_the_threshold_rule():
    x = np.array([[0.0, 0.05, 0.1, 50.0, 100.0, -3.0]], f32)
    assert_bit_equal(B.invert(x), np.array([[0.0, 0.05, f32(100.0) - f32(0.1), 50.0, 0.0, -3.0]], f32), "invert")


def test_plans(tmp_path):
    _build_and_run(tmp_path, "plan_bilateral_test")


def test_params_and_abi():
    from depth_completion_mt_amd import api
    assert L.BLUR_BILATERAL == 2 and L.BLUR_BILATERAL_CLONE == 3
    assert api.make_params(blur_type="bilateral_clone").blur == L.BLUR_BILATERAL_CLONE
    assert api.make_params(blur_type="bilateral").blur == L.BLUR_BILATERAL
    assert api.make_params(blur_type="gaussian").blur == L.BLUR_GAUSSIAN and api.make_params(blur_type="clone").blur == L.BLUR_NONE
    assert api.make_params().blur == L.BLUR_GAUSSIAN                                        # the default stays the reference's
    lib = L.lib()
    for name in ("dcmt_bilateral5_dev", "dcmt_bilateral5"):
        assert name in L.EXPORTS and hasattr(lib, name)
    # without a context every argument check is moot: refused before anything touches a device
    assert lib.dcmt_bilateral5_dev(None, None, None, 4, 4, 1, 1.5, 2.0, None) == L.E_INVALID
    assert lib.dcmt_bilateral5(None, None, 16, None, 16, 4, 4, 1.5, 2.0) == L.E_INVALID
    import depth_completion_mt_amd as pkg
    assert pkg.bilateral_filter5 is api.bilateral_filter5
