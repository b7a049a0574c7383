"""The oracle (oracle/dcmt_oracle.c), its numpy twin and the recorded fixtures against the reference's own sources,
compiled unmodified by oracle/refbuild/build_ref.py into oracle/_ref/libdcmt_ref.so (oracle/ref.py binds it).

What that build executes is the reference's own statements: thresholds, the `int d[5][5]` handed to a byte kernel, the
column extension, the hole-fill loop, the per-label mask / copy / close / copy-back, all of Slic::generate_superpixels,
the stereo functions and the three evaluate loops.  What it does not pin is OpenCV itself: the five primitives come from a
stand-in header written from OpenCV's documentation, a third implementation that is compared with the oracle's
primitives one by one below so that a mismatch of a whole chain can be attributed.

Every comparison is bit equality; there is no tolerance in this file.  The reference's fill loop has no cap, so no frame
reaches it before the oracle has reported that the frame converges.

Where there is a reference checkout and no library, these tests fail (run `python __graft_entry__.py`); they skip only
where there is neither.  The tests on the recorded fixtures (tests/golden/reference_cases.npz) need neither."""
import math
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT, assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth
from oracle import np_restatement as N
from oracle import oracle as O

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_reference_cases as MRC  # noqa: E402

F32 = np.float32
EDGE_VALUES = MRC.EDGE_VALUES


@pytest.fixture(scope="module")
def R():
    from oracle import ref
    from oracle.refbuild import build_ref
    if ref.available():
        ref.lib()                    # a library that does not load is an error, not a skip
        return ref
    if build_ref.reference_dir() is not None:
        pytest.fail("a reference checkout exists but oracle/_ref/libdcmt_ref.so does not: run python __graft_entry__.py")
    pytest.skip("neither oracle/_ref/libdcmt_ref.so nor a reference checkout")


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(GOLDEN_DIR, "reference_cases.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def converges(x, blur="gaussian"):
    """(oracle output, True) if the oracle's fill loop ends on its own; the reference may only see such frames."""
    want, info = O.img_completion(x, O.default_params(blur=blur), return_info=True)
    return want, info["rc"] == 0, info


def check_lo(R, x, what, blurs=("gaussian", "none")):
    for blur in blurs:
        want, ok, _ = converges(x, blur)
        assert ok, f"{what}: the oracle does not converge, the reference must not be called"
        assert_bit_equal(R.img_completion(x, blur), want, f"{what}, blur_type {blur!r}")


def assert_centers(got, want, what):
    assert got.shape == want.shape, what
    dead = np.isnan(want)
    assert np.array_equal(np.isnan(got), dead), f"{what}: dead centres differ"
    assert np.array_equal(got[~dead].view(np.uint64), want[~dead].view(np.uint64)), f"{what}: live centres differ"


def check_slic(R, img, step, nc, what):
    img = np.ascontiguousarray(img)
    wl, wn, wc = O.slic(img, step, nc, return_centers=True)
    gl, gn, gc = R.slic(img, step, nc, return_centers=True)
    assert gn == wn == L.lib().dcmt_slic_num_centers(img.shape[0], img.shape[1], step), (what, gn, wn)
    assert np.array_equal(gl, wl), f"{what}: {int((gl != wl).sum())} labels differ"
    assert_centers(wc, gc, what)
    return gl, gn, gc


# ------------------------------------------------------------------ the stand-in's primitives, one by one
@pytest.mark.parametrize("shape", ((1, 9), (9, 1), (3, 4), (5, 5), (7, 31), (33, 70), (48, 64), (64, 33)))
def test_standin_primitives_equal_the_oracle_primitives(R, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    frames = [rng.uniform(-5, 105, shape).astype(F32),
              np.where(rng.random(shape) < 0.1, rng.uniform(0.2, 99, shape), 0).astype(F32),
              rng.choice(EDGE_VALUES, shape).astype(F32)]
    for i, x in enumerate(frames):
        for k in (5, 7, 31):
            ones = np.ones((k, k), np.uint8)
            assert_bit_equal(R.standin_dilate(x, ones), O.dilate_rect(x, k), f"dilate {k}x{k} of frame {i} {shape}")
            assert_bit_equal(R.standin_erode(x, ones), O.erode_rect(x, k), f"erode {k}x{k} of frame {i} {shape}")
        for el in (O.k0_as_compiled(), O.k0_diamond(), (rng.random((5, 5)) < 0.3).astype(np.uint8) * 7):
            if el.any():
                assert_bit_equal(R.standin_dilate(x, el), O.dilate_mask5(x, el), f"dilate with element {el.ravel().tolist()} of frame {i} {shape}")
        assert_bit_equal(R.standin_median5(x), O.median5(x), f"median of frame {i} {shape}")
        assert_bit_equal(R.standin_median5(x), O.median5(x, simple=True), f"median (definition) of frame {i} {shape}")
        assert_bit_equal(R.standin_gaussian5(x), O.gaussian5(x), f"gaussian of frame {i} {shape}")


# ------------------------------------------------------------------ img_completion
def test_img_completion_on_the_goldens_inputs(R, golden, golden_meta):
    """Every input of small_cases.npz, against its committed output and the oracle.  All of them converge under the oracle's
    default cap (the fill-loop cap's test lowers the cap on tall_gap, which needs 7 passes); one that did not would be held
    back from the reference."""
    assert_bit_equal(R.img_completion(golden["crop48x64_in"]), golden["crop48x64_stage11"], "crop48x64")
    assert_bit_equal(R.img_completion(golden["crop48x64_in"], "none"), golden["crop48x64_noblur"], "crop48x64 without blur")
    assert_bit_equal(R.img_completion(golden["odd33x70_in"]), golden["odd33x70_out"], "odd33x70")
    ran, held_back = [], []
    for name in sorted(golden_meta["adversarial"]):
        x = golden[f"adv_{name}_in"]
        want, ok, info = converges(x)
        if not ok:
            held_back.append(name)
            continue
        assert info["fill_iters"] == golden_meta["adversarial"][name]["fill_iters"]
        assert_bit_equal(want, golden[f"adv_{name}_out"], f"oracle on adv_{name}")
        assert_bit_equal(R.img_completion(x), golden[f"adv_{name}_out"], f"adv_{name}")
        check_lo(R, x, f"adv_{name}")
        ran.append(name)
    assert held_back == [], held_back
    assert {"tall_gap", "negative_region", "threshold", "one_row", "one_col", "tiny_3x4"} <= set(ran)


@pytest.mark.parametrize("rows,cols", ((352, 1216), (375, 1242)))
def test_img_completion_full_size(R, rows, cols):
    check_lo(R, synth.synth_frame(rows, cols, 5), f"{rows}x{cols}")


def test_img_completion_odd_sizes(R):
    rng = np.random.default_rng(5)
    shapes = [(1, 1), (1, 40), (40, 1), (2, 2), (5, 5), (7, 31), (31, 7)]
    shapes += [(r, c) for r in (30, 31, 32, 61, 62, 63) for c in (30, 31, 32, 61, 62, 63) if (r + c) % 3 != 1]
    for rows, cols in shapes:
        x = np.where(rng.random((rows, cols)) < 0.12, rng.uniform(0.5, 95.0, (rows, cols)), 0).astype(F32)
        x[rng.integers(rows), rng.integers(cols)] = 33.25        # at least one valid pixel
        check_lo(R, x, f"{rows}x{cols}")


def test_img_completion_on_frames_that_need_several_passes_of_the_loop(R):
    """The constructions of tests/test_tail.py and tests/test_tail_phases.py: the reference's uncapped while loop runs 2 to 8
    times on these."""
    seen = set()
    for rows, h0, cols in ((240, 30, 48), (240, 60, 48), (240, 80, 48), (200, 198, 48), (240, 232, 48), (240, 80, 256), (120, 70, 33)):
        x = MRC.gap_frame(rows, h0, cols)
        _, ok, info = converges(x)
        assert ok
        seen.add(info["fill_iters"])
        check_lo(R, x, f"gap {rows}x{cols} from row {h0} ({info['fill_iters']} passes)")
    assert max(seen) >= 7 and len([n for n in seen if n >= 2]) >= 3, seen


def fuzz_frame(rng, i):
    rows, cols = int(rng.integers(1, 80)), int(rng.integers(1, 140))
    density = (0.01, 0.05, 0.30)[i % 3]
    x = np.where(rng.random((rows, cols)) < density, rng.uniform(0.2, 99.0, (rows, cols)), 0).astype(F32)
    m = rng.random((rows, cols)) < 0.02
    x[m] = rng.choice(EDGE_VALUES, int(m.sum()))
    kind = i % 9
    if kind == 0:
        x[:, rng.integers(cols)] = 0                          # an emptied column
    elif kind == 1:
        x[:] = 0
        x[(0, -1)[i % 2], (0, -1)[(i // 2) % 2]] = 17.5       # a single valid pixel in a corner
    elif kind == 2:
        x[1:] = 0                                            # valid pixels only in the first row
        x[0, rng.integers(cols)] = 8.0
    elif kind == 3:
        x[:-1] = 0                                           # ... only in the last row
        x[-1, rng.integers(cols)] = 8.0
    return x


def test_img_completion_fuzz_biased_to_the_edges(R):
    """Seeded small frames with the values where a reading goes wrong: 0.1f and its neighbours, 100 - 0.1f, 100, above 100
    (negative once inverted), negatives, -0.0f; empty columns, lone pixels in corners, a single valid row.  Frames the oracle
    reports as not converging are dropped before the reference sees them; their share stays under 2 %."""
    rng = np.random.default_rng(20240)
    n, dropped = 270, 0
    for i in range(n):
        x = fuzz_frame(rng, i)
        blur = "gaussian" if i % 4 else "none"
        want, ok, _ = converges(x, blur)
        if not ok:
            dropped += 1
            continue
        assert_bit_equal(R.img_completion(x, blur), want, f"fuzz frame {i} {x.shape}, blur_type {blur!r}")
    print(f"fuzz: {dropped} of {n} frames dropped for not converging")
    assert dropped / n < 0.02, (dropped, n)


def test_first_kernel_is_what_the_int_array_compiles_to(R):
    """The reference hands `int d[5][5]` to a CV_8UC1 header: the build that executes it agrees with the two-tap element
    dcmt_oracle_k0_as_compiled states, and not with the 13-tap diamond the source's comment intends."""
    k = O.k0_as_compiled()
    assert k.sum() == 2 and k[1, 3] == 1 and k[4, 4] == 1
    differ = 0
    for seed in range(4):
        x = synth.synth_frame(48, 64, 20 + seed)
        got = R.img_completion(x)
        assert_bit_equal(got, O.img_completion(x, O.default_params(k0="as_compiled")), f"seed {seed}")
        differ += int((got.view(np.uint32) != O.img_completion(x, O.default_params(k0="diamond")).view(np.uint32)).any())
    assert differ == 4


# ------------------------------------------------------------------ SLIC
@pytest.mark.parametrize("rows,cols,step,nc", ((352, 1216, 18, 50), (375, 1242, 68, 40)))
def test_slic_at_both_callers_settings(R, rows, cols, step, nc):
    assert step == int(math.sqrt(rows * cols / (1200 if rows == 352 else 100)))       # the callers' double step, truncated at the call
    check_slic(R, synth.synth_lab(rows, cols, 21), step, nc, f"{rows}x{cols} step {step} nc {nc}")


def test_slic_small_steps_ties_dead_centres_and_grid_edges(R):
    dead = 0
    for step in (6, 7, 8, 9, 10, 11, 16):
        for rows, cols, seed in ((75, 131, 40 + step), (96, 160, 1)):
            _, _, c = check_slic(R, synth.synth_lab(rows, cols, seed), step, 40 if step != 7 else 10, f"{rows}x{cols} step {step}")
            dead += int(np.isnan(c[:, 3]).sum())
    assert dead > 0, "no case with a centre that dies"
    # exact ties: the lower centre index keeps the pixel (strict < in index order)
    flat = np.full((100, 170, 3), 128, np.uint8)
    halves = flat.copy()
    halves[:, 85:] = (30, 200, 90)
    for img, step, nc in ((flat, 16, 40), (flat, 9, 40), (halves, 18, 50), (halves, 7, 1)):
        check_slic(R, img, step, nc, f"flat / two-tone step {step} nc {nc}")
    lab = synth.synth_lab(100, 170, 3)
    for nc in (1, 100000):
        check_slic(R, lab, 16, nc, f"nc {nc}")
    # `i < cols - step / 2` and `j < rows - step / 2` on either side of a grid point; the count against dcmt_slic_num_centers
    counts = set()
    for step in (6, 9, 12):
        for d in (-1, 0, 1):
            rows, cols = 3 * step + step // 2 + d, 4 * step + step // 2 + d
            _, n, _ = check_slic(R, synth.synth_lab(rows, cols, 9), step, 30, f"grid edge {rows}x{cols} step {step}")
            counts.add((step, d, n))
    assert len({n for _, _, n in counts}) > 1, counts
    # too small for a single centre: every label stays -1
    gl, gn, _ = check_slic(R, synth.synth_lab(10, 40, 2), 12, 40, "no centre")
    assert gn == 0 and (gl == -1).all()


def test_slic_fuzz(R):
    rng = np.random.default_rng(31)
    for i in range(30):
        step = int(rng.integers(6, 20))
        rows, cols = int(rng.integers(8, 90)), int(rng.integers(8, 140))
        img = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)
        if i % 3 == 0:
            img = (img // 64 * 64).astype(np.uint8)          # few distinct colours: ties
        if i % 5 == 0:
            img[:, :, 0] = 77
        check_slic(R, img, step, int(rng.choice((1, 10, 40, 50, 1000))), f"fuzz {i}: {rows}x{cols} step {step}")


# ------------------------------------------------------------------ interpolate_with_superpixels
def check_lc(R, x, labels, n, what, modes=(0, 1)):
    for us in modes:
        want, info = O.interpolate_with_superpixels(x, labels, n, use_superpixel=us, return_info=True)
        assert info["rc"] == 0, f"{what}: the oracle does not converge, the reference must not be called"
        assert_bit_equal(R.interpolate_with_superpixels(x, labels, n, us), want, f"{what}, use_superpixel {us}")


def test_interpolate_with_superpixels(R, golden, golden_meta):
    x = synth.synth_frame(96, 160, 5)
    lab, n, _ = R.slic(golden["slic_lab96x160"], 12, 40, return_centers=True)          # labels from the reference's own SLIC
    assert n == 84
    check_lc(R, x, lab, n, "96x160, reference SLIC labels")
    assert_bit_equal(R.interpolate_with_superpixels(x, lab, n, 1), golden["slic_chain96x160"], "SLIC -> interpolate golden")
    assert_bit_equal(R.interpolate_with_superpixels(golden["lc40x56_in"], golden["lc40x56_labels"], golden_meta["lc40x56_n_labels"], 1), golden["lc40x56_out"], "lc40x56")
    assert_bit_equal(R.interpolate_with_superpixels(golden["lc40x56_in"], golden["lc40x56_labels"], golden_meta["lc40x56_n_labels"], 0), golden["lc40x56_out_nosp"], "lc40x56 nosp")
    x = synth.synth_frame(40, 56, 3)
    lab, n = synth.synth_labels(40, 56, 30, 1)
    assert (lab == -1).any()
    check_lc(R, x, lab, n, "40x56 synth_labels with unreached pixels")
    check_lc(R, x, lab, n + 9, "n_labels above the highest label", modes=(1,))
    gone = lab.copy()
    gone[gone == 3] = 4                                                    # label 3 owns no pixel
    check_lc(R, x, gone, n, "a label without pixels", modes=(1,))
    ones = lab.copy()
    for k, (r, c) in enumerate(((0, 0), (39, 55), (20, 28), (7, 0))):      # one-pixel superpixels, three of them on the border
        ones[r, c] = n + k
    xx = x.copy()
    xx[20, 28], xx[0, 0] = 12.5, 40.0
    check_lc(R, xx, ones, n + 4, "one-pixel superpixels", modes=(1,))
    ring = lab.copy()
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = 2                # one superpixel touches all four borders
    ring[1, 1:-1] = 2
    check_lc(R, x, ring, n, "a superpixel along all four borders", modes=(1,))
    lost = lab.copy()
    lost[::3, ::2] = -1                                                    # a third of a half of the pixels unreached
    check_lc(R, x, lost, n, "many unreached pixels", modes=(1,))
    rng = np.random.default_rng(77)
    edge = x.copy()
    m = rng.random(x.shape) < 0.05
    edge[m] = rng.choice(EDGE_VALUES, int(m.sum()))
    check_lc(R, edge, lab, n, "edge values")


# ------------------------------------------------------------------ stereo
def check_stereo(R, O_, depth, left, right, what):
    """Every pixel is compared, those at the right edge of the patch included."""
    pre, post = R.stereo(depth, left, right)
    assert_bit_equal(pre, O_.stereo_refine(depth, left, right, iterations=0), f"{what}: before the sweeps")
    want = O_.stereo_refine(depth, left, right)
    assert_bit_equal(post, want, f"{what}: after the sweeps")
    return post, want


def test_stereo_refinement(R, golden):
    l, r, g = golden["stereo_left48x64"], golden["stereo_right48x64"], golden["stereo_guess48x64"]
    check_stereo(R, O, g, l, r, "golden triple")
    for rows, cols, seed in ((48, 64, 1), (97, 131, 2), (33, 50, 3), (375, 1242, 30)):
        l, r, g = synth.synth_stereo(rows, cols, seed)
        check_stereo(R, O, g, l, r, f"synth_stereo {rows}x{cols}")      # realistic depths never reach the edge case
    # black / white noise: the patch extrapolates (dc in [-0.5, 0.5]) up to 382.5, so errors beyond +-255 reach the clamp
    l, r, g = synth.synth_stereo(48, 64, 5)
    noise = np.random.default_rng(3)
    l2, r2 = (noise.choice(np.array([0, 255], np.uint8), g.shape) for _ in range(2))
    check_stereo(R, O, g, np.ascontiguousarray(l2), np.ascontiguousarray(r2), "black and white noise")
    l, r, g = synth.synth_stereo(48, 64, 4)
    post, _ = check_stereo(R, O, np.zeros_like(g), l, r, "no depth anywhere")
    assert not post.any()
    # disparities below 1 (depth beyond 518 m) and above the image width (depth of millimetres), negative depths
    rng = np.random.default_rng(8)
    wild = g.copy()
    m = rng.random(g.shape) < 0.2
    wild[m] = rng.choice(np.array([600.0, 1100.0, 5000.0, 1e6, 0.004, 0.05, 1.0, -4.0, 518.28, 1036.6], F32), int(m.sum()))
    wild[:, -1] = rng.choice(np.array([7.0, 30.0, 90.0], F32), g.shape[0])                # ... none of them in the last column
    check_stereo(R, O, wild, l, r, "wild depths away from the last column")
    assert not MRC.right_edge_pixels(wild).any()
    # the last column with disparities below 0.5 (the patch reaches column `cols`), and the last row (patch row `rows`)
    wild[::2, -1] = rng.choice(np.array([1100.0, 5000.0, 1e6, 2000.0], F32), len(wild[::2, -1]))
    wild[-1, :] = rng.choice(np.array([600.0, 9.0, 44.0, 2000.0], F32), g.shape[1])
    assert MRC.right_edge_pixels(wild).sum() >= g.shape[0] // 2
    check_stereo(R, O, wild, l, r, "last column and last row")


def test_the_stereo_edge_is_what_design_md_says(R):
    """At a pixel of the last column whose patch reaches column `cols`, the oracle (and k_stereo_refine with it) takes the
    next pixel of a dense run, the first pixel of the next row; the reference's images have 48-byte elements addressed in
    12-byte steps, so its entry lies inside the same row, in bytes nothing writes.  The grey values read differ, the
    results do not: both derivative entries of such a patch are border entries (0), so dx = 0 and the disparity keeps its
    value -- as long as the reference's unwritten bytes hold a zero derivative, which the stand-in's zero-filled cv::Mat
    guarantees and a real one does not."""
    l, r, g = synth.synth_stereo(24, 40, 6)
    g[:, -1] = 2000.0                               # disparity 0.259: c0 = cols - 1 in every sweep
    l[:, :], r[:, :] = 90, 90
    r[:, -1], r[:, 0] = 200, 0
    r[10, 0] = 255                                  # what row 9's last pixel reads in the oracle; the stand-in reads 0
    assert MRC.right_edge_pixels(g).all()
    for right in (r, np.where(np.arange(40)[None, :] == 38, 10, r).astype(np.uint8)):      # (a step next to the last column too)
        pre, post = R.stereo(g, l, np.ascontiguousarray(right))
        want = O.stereo_refine(g, l, np.ascontiguousarray(right))
        assert_bit_equal(post, want, "with zeroed bytes the pixels at the right edge agree too")
        assert_bit_equal(post[:, -1], pre[:, -1], "the last column keeps its disparity")


# ------------------------------------------------------------------ evaluate_performance(s)
def np_sums(gt, pred, thresh, mode):
    """dcmt_evaluate's seven sums of one frame from numpy (per-pixel terms in f32, summed exactly)."""
    g, p = gt.ravel(), pred.ravel()
    m = g > F32(thresh)
    if mode == "both":
        m &= p > F32(thresh)
    e = g[m] - p[m]
    d = np.abs(e)
    inv = m & (p > 0)
    di = np.abs(1.0 / g[inv].astype(np.float64) - 1.0 / p[inv].astype(np.float64))
    fs = lambda a: math.fsum(np.asarray(a, np.float64).tolist())
    return np.array([m.sum(), fs(e), fs(d), fs(d * d), inv.sum(), fs(di), fs(di * di)], np.float64)


def test_evaluate_functions(R):
    """api.reference_performance turns the sums into what the three reference functions return; on inputs in multiples of
    1/256 m the reference's f32 running sums are exact, so the results are equal bit for bit."""
    pairs = [MRC.eval_pair(40, 56, 7), MRC.eval_pair(17, 93, 8)]
    for gt, pred in pairs:
        for preset, (mode, thresh) in api.EVAL_PRESETS.items():
            want = np.atleast_1d(np.asarray(api.reference_performance(np_sums(gt, pred, thresh, mode), preset), F32))
            got = np.atleast_1d(np.asarray(R.EVALUATE[preset](gt, pred), F32))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (preset, got, want)
    gt, pred = pairs[0]
    for preset, (mode, thresh) in api.EVAL_PRESETS.items():                 # an empty selection: 0 / 0 on both sides
        got = np.atleast_1d(np.asarray(R.EVALUATE[preset](np.zeros_like(gt), pred), F32))
        want = np.atleast_1d(np.asarray(api.reference_performance(np_sums(np.zeros_like(gt), pred, thresh, mode), preset), F32))
        assert np.isnan(got).all() and np.isnan(want).all(), (preset, got, want)
    # the lidar-camera tolerance is `int tolerance = 0.1`, i.e. 0: a prediction of 0.05 m counts there, not in the stereo preset
    gt = np.full((4, 4), 3.0, F32)
    pred = np.full((4, 4), 0.05 + 0 * 3.0, F32)
    pred[0, 0] = 3.5
    rmse, mae = R.evaluate_lc(gt, pred)
    assert mae > 2.0
    mae2, _ = R.evaluate_sl(gt, pred)
    assert mae2 == F32(0.5)


# ------------------------------------------------------------------ the numpy twin
def test_numpy_twin_against_the_reference_build(R, golden):
    for x in (synth.synth_frame(48, 64, 3), golden["adv_threshold_in"], golden["adv_negative_region_in"], MRC.gap_frame(120, 70, 33)):
        for blur in ("gaussian", "none"):
            assert converges(x, blur)[1]
            assert_bit_equal(N.img_completion(x, blur=blur), R.img_completion(x, blur), f"numpy twin img_completion {x.shape} {blur}")
    for img, step, nc in ((synth.synth_lab(60, 90, 5), 8, 40), (synth.synth_lab(96, 160, 1), 7, 40)):
        nl, nn, ncent = N.slic(img, step, nc)
        gl, gn, gc = R.slic(img, step, nc, return_centers=True)
        assert nn == gn and np.array_equal(nl, gl)
        assert_centers(np.asarray(ncent, np.float64), gc, f"numpy twin slic step {step}")
    x = synth.synth_frame(40, 56, 3)
    lab, n = synth.synth_labels(40, 56, 30, 1)
    assert O.interpolate_with_superpixels(x, lab, n, return_info=True)[1]["rc"] == 0
    for us in (0, 1):
        assert_bit_equal(N.interpolate_with_superpixels(x, lab, n, use_superpixel=us), R.interpolate_with_superpixels(x, lab, n, us), f"numpy twin lc {us}")
    l, r, g = synth.synth_stereo(48, 64, 1)
    pre, post = R.stereo(g, l, r)
    assert_bit_equal(N.stereo_refine(g, l, r, iterations=0), pre, "numpy twin stereo, before the sweeps")
    assert_bit_equal(N.stereo_refine(g, l, r), post, "numpy twin stereo, after the sweeps")


# ------------------------------------------------------------------ recorded fixtures
def oracle_on_recorded(z):
    """The oracle's answers to the recorded inputs, under the names of the reference's recorded answers."""
    out = {}
    for k in ("lo48x64", "lo_edge33x70", "lo_gap240x48"):
        for suffix, blur in (("_out", "gaussian"), ("_out_noblur", "none")):
            want, ok, _ = converges(z[k + "_in"], blur)
            assert ok
            out[k + suffix] = want
    for k in ("slic60x90", "slic96x160"):
        step, nc = (int(v) for v in z[k + "_step_nc"])
        out[k + "_labels"], _, out[k + "_centers"] = O.slic(z[k + "_img"], step, nc, return_centers=True)
    chain, info = O.interpolate_with_superpixels(z["chain96x160_in"], out["slic96x160_labels"], out["slic96x160_centers"].shape[0], return_info=True)
    assert info["rc"] == 0
    out["chain96x160_out"] = chain
    n = int(z["lc40x56_n"][0])
    out["lc40x56_out"] = O.interpolate_with_superpixels(z["lc40x56_in"], z["lc40x56_labels"], n, use_superpixel=1)
    out["lc40x56_out_nosp"] = O.interpolate_with_superpixels(z["lc40x56_in"], z["lc40x56_labels"], n, use_superpixel=0)
    d, l, r = z["stereo48x64_depth"], z["stereo48x64_left"], z["stereo48x64_right"]
    out["stereo48x64_pre"] = O.stereo_refine(d, l, r, iterations=0)
    out["stereo48x64_post"] = O.stereo_refine(d, l, r)
    for preset, (mode, thresh) in api.EVAL_PRESETS.items():
        out["eval40x56_" + preset] = np.atleast_1d(np.asarray(api.reference_performance(np_sums(z["eval40x56_gt"], z["eval40x56_pred"], thresh, mode), preset), F32))
    return out


def test_oracle_against_the_recorded_reference_outputs(recorded):
    """Needs no reference build: what the reference's code returned is in tests/golden/reference_cases.npz."""
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "reference_cases.npz")) < os.path.getsize(os.path.join(GOLDEN_DIR, "small_cases.npz"))
    mine = oracle_on_recorded(recorded)
    assert set(mine) | set(MRC.inputs()) == set(recorded)
    assert MRC.right_edge_pixels(recorded["stereo48x64_depth"]).sum() == 2      # the two pixels make_reference_cases.py puts there
    assert np.isnan(recorded["slic96x160_centers"]).any()   # a case with dead centres
    for k, want in mine.items():
        got = recorded[k]
        assert MRC.same(np.asarray(want, got.dtype), got), f"{k}: the oracle differs from what the reference returned"


def test_recorded_fixtures_are_what_the_reference_build_produces_today(R, recorded):
    fresh = MRC.record(R)
    assert set(fresh) == set(recorded)
    for k in sorted(fresh):
        assert MRC.same(np.asarray(fresh[k]), recorded[k]), f"{k}: tests/golden/reference_cases.npz is stale (python tests/golden/make_reference_cases.py)"


# ------------------------------------------------------------------ the build recipe's cutter (no reference needed)
def test_cut_by_signature_and_braces_fails_loudly():
    from oracle.refbuild import build_ref
    text = ('// void f(int){ }\n/* void f(){ */\nvoid f(int a);\nstruct S {\n  float v; // }\n};\n'
            'void f(int a)\n{ if (a) { char c = \'}\'; const char* s = "}{"; } }\nint g;\nvoid h() {}\nvoid h() {}\n')
    assert build_ref.cut_definition(text, "void", "f") == 'void f(int a)\n{ if (a) { char c = \'}\'; const char* s = "}{"; } }\n'
    assert build_ref.cut_definition(text, "struct", "S") == "struct S {\n  float v; // }\n};\n"
    for kind, name in (("void", "h"), ("void", "missing"), ("bool", "f")):
        with pytest.raises(build_ref.CutError):
            build_ref.cut_definition(text, kind, name)
    with pytest.raises(build_ref.CutError):
        build_ref.cut_definition("void k() { {", "void", "k")
