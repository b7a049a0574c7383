"""max_depth and valid_thresh on the CPU: the two oracles (oracle/dcmt_oracle.c, oracle/np_restatement.py) and the test restatements
take both parameters and agree bit for bit under the whole parameter grid of tests/param_cases.py; the inputs of the device tests
(tests/test_gpu_params.py) are shown to depend on each parameter; and the cascade's scaling relation holds on the oracle.

Nothing here runs a kernel.  Shapes 24x40 and 45x131 (the second tall enough for the "gap" variant)."""
import numpy as np
import pytest

import bilateral_restatement as B
import no_extrapolate_restatement as R
import param_cases as P
from conftest import assert_bit_equal
from oracle import np_restatement as N
from oracle import oracle as O

f32 = np.float32
SHAPES = ((24, 40), (45, 131))
SEED = P.SEEDS[0]
NK0 = {"as_compiled": N.K0_AS_COMPILED, "diamond": N.K0_DIAMOND, "custom": P.K0_CUSTOM}
K0S = ("as_compiled", "diamond", "custom")
grid = pytest.mark.parametrize("mt", P.GRID, ids=P.pid)


def ok0(name):
    return P.K0_CUSTOM if name == "custom" else name


def test_double_literal_compares_are_the_f32_compares():
    """The reference writes `x > 0.1` / `x < 0.1` with x promoted to double; the oracles now write x >= 0.1f / x < 0.1f so that the
    threshold can be a parameter.  The two forms agree on the 2^16 f32 values on either side of 0.1f (and so everywhere: both are
    monotonic in x)."""
    t = f32(0.1)
    b = int(np.array(t).view(np.uint32))
    x = np.arange(b - 65536, b + 65537, dtype=np.uint32).view(f32)
    assert x[65536] == t and x.size == 2 * 65536 + 1
    d = x.astype(np.float64)
    assert np.array_equal(d > 0.1, x >= t) and np.array_equal(d < 0.1, x < t)
    assert (d > 0.1).sum() == 65537 and (d < 0.1).sum() == 65536         # 0.1f itself is valid, its lower neighbour a hole


def test_defaults_are_the_references_constants():
    p = O.default_params()
    assert p.max_depth == 100.0 and f32(p.valid_thresh) == f32(0.1)
    q = O.default_params(max_depth=30.0, valid_thresh=1.0)
    assert (q.max_depth, q.valid_thresh) == (30.0, 1.0)
    assert f32(N.DEFAULT_VALID_THRESH) == f32(0.1) and N.DEFAULT_MAX_DEPTH == 100.0


@grid
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_c_oracle_equals_numpy_restatement_plain(mt, rows, cols):
    """every variant, with every k0 (two presets and a custom one) and both blurs between them, whole chain; primitives too"""
    M, t = mt
    i = P.GRID.index(mt)
    for v, variant in enumerate(P.VARIANTS):
        x = P.edge_frame(rows, cols, SEED, M, t, variant)
        for j in range(2):
            k0, blur = K0S[(i + v + j) % 3], ("gaussian", "none")[(i + v + j) % 2]
            ci, ni = {}, {}
            c, ci = O.img_completion(x, P.oparams(M, t, k0=ok0(k0), blur=blur, max_fill_iters=6), return_info=True)
            n = N.img_completion(x, k0=NK0[k0], blur=blur, max_fill_iters=6, info=ni, max_depth=f32(M), valid_thresh=f32(t))
            assert_bit_equal(c, n, f"{rows}x{cols} {variant} {P.pid(mt)} {k0} {blur}")
            assert ci["fill_iters"] == ni["fill_iters"] and ci["holes_after_extend"] == ni["holes_after_extend"]
        x6 = O.img_completion(x, P.oparams(M, t, stop_after=5))
        assert_bit_equal(O.extend_columns(x6, t), N.extend_columns(x6, f32(t)), f"extend_columns {variant} {P.pid(mt)}")


@grid
def test_c_oracle_equals_numpy_restatement_at_every_stage(mt):
    """stop_after 2..11 of the plain chain (the variant, k0 and blur change with the grid point)"""
    M, t = mt
    i = P.GRID.index(mt)
    rows, cols = SHAPES[i % 2]
    variant, k0, blur = P.VARIANTS[i % 3], K0S[i % 3], ("gaussian", "none")[(i // 2) % 2]
    x = P.edge_frame(rows, cols, SEED, M, t, variant)
    for stop in range(2, 12):
        c = O.img_completion(x, P.oparams(M, t, k0=ok0(k0), blur=blur, stop_after=stop))
        n = N.img_completion(x, k0=NK0[k0], blur=blur, stop_after=stop, max_depth=f32(M), valid_thresh=f32(t))
        assert_bit_equal(c, n, f"{rows}x{cols} {variant} {P.pid(mt)} {k0} {blur} stop {stop}")


@grid
def test_c_oracle_equals_numpy_restatement_labeled(mt):
    """the labeled chain at stop_after 4 and 11, with and without the label-masked stage, ROI and brute-force forms of the C oracle"""
    from test_gpu_fuzz import _labels
    M, t = mt
    i = P.GRID.index(mt)
    rows, cols = SHAPES[i % 2]
    g = np.random.Generator(np.random.PCG64(50 + i))
    lab, n = _labels(g, rows, cols)
    for v, variant in enumerate(P.VARIANTS):
        x = P.edge_frame(rows, cols, SEED, M, t, variant)
        k0 = ("as_compiled", "diamond")[(i + v) % 2]
        for stop in (4, 11):
            for sp in (1, 0):
                c = O.interpolate_with_superpixels(x, lab, n, P.oparams(M, t, k0=k0, stop_after=stop), use_superpixel=sp)
                w = N.interpolate_with_superpixels(x, lab, n, k0=NK0[k0], use_superpixel=sp, stop_after=stop, max_depth=f32(M), valid_thresh=f32(t))
                assert_bit_equal(c, w, f"labeled {rows}x{cols} {variant} {P.pid(mt)} {k0} stop {stop} use_superpixel {sp}")
            b = O.interpolate_with_superpixels(x, lab, n, P.oparams(M, t, k0=k0, stop_after=stop), bruteforce=True)
            assert_bit_equal(b, O.interpolate_with_superpixels(x, lab, n, P.oparams(M, t, k0=k0, stop_after=stop)), "brute force")


@grid
def test_no_extrapolate_and_bilateral_restatements_follow_the_parameters(mt):
    """Restatements (a) and (b) of the cascade without its extrapolation agree under (M, t) and start from the C oracle's X5; their X9
    is its median; the bilateral restatement's invert of the C oracle's X9 is the C oracle's blur-less stage 11."""
    M, t = mt
    i = P.GRID.index(mt)
    rows, cols = SHAPES[i % 2]
    planes = dict(R.adversarial_planes(rows, cols, M, t))
    for variant in P.VARIANTS:
        planes[variant] = P.edge_frame(rows, cols, SEED, M, t, variant)
    uninverted = 0
    for name, x in planes.items():
        k0 = ("as_compiled", "diamond")[(i + len(name)) % 2]
        x5 = O.img_completion(x, P.oparams(M, t, k0=k0, stop_after=5))
        assert_bit_equal(R.x5_oracle(x, k0, max_depth=M, valid_thresh=t), x5, f"X5 {name}")
        assert_bit_equal(R.restatement_oracle(x, k0, "none", 9, max_depth=M, valid_thresh=t), O.median5(x5), f"X9 {name}")
        for stop in (9, 10, 11):
            for blur in ("gaussian", "none"):
                a = R.restatement_oracle(x, k0, blur, stop, max_depth=M, valid_thresh=t)
                b = R.restatement_numpy(x, k0, blur, stop, max_depth=f32(M), valid_thresh=f32(t))
                assert_bit_equal(a, b, f"no extrapolation {name} {P.pid(mt)} {k0} {blur} stop {stop}")
        uninverted += int(R.uninverted_pixels(x, k0, M, t).sum())
        x9 = O.img_completion(x, P.oparams(M, t, k0=k0, blur="none", stop_after=9))
        assert_bit_equal(B.invert(x9, M, t), O.img_completion(x, P.oparams(M, t, k0=k0, blur="none")), f"bilateral invert {name}")
    assert uninverted > 0, "no pixel whose median is valid and whose blurred value is below thr: the planes do not reach that statement"


# ---- the inputs depend on the parameters ---------------------------------------------------------------------------------------
GPU_SHAPES = ((33, 70), (70, 333), (70, 332))      # (70x332: the 16-bit route needs an even width)


@grid
@pytest.mark.parametrize("rows,cols", SHAPES + GPU_SHAPES)
def test_inputs_are_sensitive_to_each_parameter(mt, rows, cols):
    """The condition on the inputs: for every frame the tests run the whole chain on, the oracle's result under (M, t) differs in
    at least 5 % of the pixels from its result with either field put back to its default.  (All frames of every batch: seeds x variants,
    plain and on the 1/256 m grid.)  A frame that misses it is replaced, the bound stays."""
    M, t = mt
    for seed in P.SEEDS:
        for variant in P.VARIANTS:
            for on_grid in (False, True):
                x = P.edge_frame(rows, cols, seed, M, t, variant, on_grid, on_grid)
                P.assert_sensitive(x, M, t, f"{rows}x{cols} seed {seed} {variant} on_grid {on_grid} {P.pid(mt)}")


@grid
def test_every_probed_stage_is_sensitive(mt):
    """stop_after probes: at every stage 2..10 at least one pixel moves with each non-default field"""
    M, t = mt
    for rows, cols in GPU_SHAPES:
        for variant in P.VARIANTS:
            x = P.edge_frame(rows, cols, SEED, M, t, variant)
            for stop in range(2, 11):
                P.assert_sensitive(x, M, t, f"{rows}x{cols} {variant} {P.pid(mt)}", stop=stop, bound=0)


def test_dispatch_toggle_frames_are_sensitive():
    M, t = 50.0, 0.5
    for seed in P.SEEDS[:2]:
        for variant in P.VARIANTS:
            P.assert_sensitive(P.edge_frame(352, 1216, seed, M, t, variant), M, t, f"352x1216 seed {seed} {variant}")


# ---- the scaling relation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(37, 131), (120, 333), (352, 1216)])
def test_scaling_relation_on_the_oracle(rows, cols):
    """img_completion(s x; s M, s t) == s img_completion(x; M, t) bit for bit for s a power of two, (M, t) = (100, 0.1f): every
    operation of the cascade (compare, subtract from M, max, min, median, the Gaussian's dyadic weights) commutes with an exact
    scaling.  The one thing that does not scale is the column extension's literal 100, so only frames whose X5 has no empty column
    qualify (asserted).  The bilateral finish and the normalisation have constants of their own and are excluded."""
    M, t = f32(100.0), f32(0.1)
    assert f32(f32(0.05) * f32(2.0)) == t
    frames = P.scaling_frames(rows, cols)[:3]
    assert len(frames) >= 2 and any("gap" in what for what, _ in frames), "too few frames without an empty column at X5"
    for what, x in frames:
        for k0 in ("as_compiled", "diamond"):
            x5 = O.img_completion(x, P.oparams(M, t, k0=k0, stop_after=5))
            assert (x5 >= t).any(axis=0).all(), "a column of X5 is empty: the literal 100 would show"
            for blur in ("gaussian", "none"):
                base = O.img_completion(x, P.oparams(M, t, k0=k0, blur=blur))
                for s in (0.5, 2.0, 0.25):
                    s = f32(s)
                    got = O.img_completion(x * s, P.oparams(M * s, t * s, k0=k0, blur=blur))
                    assert_bit_equal(got, base * s, f"{what} {k0} {blur} s = {s}")
