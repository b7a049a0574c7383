"""Writes tests/golden/reference_cases.npz: a small, named set of inputs and what the reference's own code returned
for them, run through oracle/_ref/libdcmt_ref.so (oracle/refbuild/build_ref.py builds it from a reference checkout).
The file pins the oracle and the kernels to the reference where no reference build exists.

    python tests/golden/make_reference_cases.py        # needs oracle/_ref/libdcmt_ref.so

record() is also what tests/test_reference_parity.py calls to check that the committed file is what the reference
build produces today."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from depth_completion_mt_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_cases.npz")
F32 = np.float32
EDGE_VALUES = np.array([F32(0.1), np.nextafter(F32(0.1), F32(0)), np.nextafter(F32(0.1), F32(1)), F32(100) - F32(0.1), 100.0, 100.5,
                        250.0, -3.0, -0.0, 0.05, 99.95], dtype=np.float32)


def gap_frame(rows, h0, cols=48):
    """Valid rows at the top and from h0 down: the taller the gap, the more passes of the 31x31 loop it takes."""
    x = np.zeros((rows, cols), np.float32)
    x[0:2] = 40.0
    x[h0:] = 12.0
    return x


def right_edge_pixels(depth, baseline=0.54, focal=9.597910e+02):
    """Rows whose last-column pixel starts with a disparity that puts the right column of its stereo patch at column `cols`
    (c0 = (int)(c + 0.5) = cols - 1, disparity != 0): the entry the reference never writes."""
    d = np.asarray(depth, np.float32)[:, -1]
    cols = np.asarray(depth).shape[1]
    disp = np.zeros_like(d)
    with np.errstate(divide="ignore"):
        disp[d > 0] = (F32(baseline) * F32(focal)) / d[d > 0]
    c = F32(cols - 1) - disp
    return (np.trunc(c.astype(np.float64) + 0.5) == cols - 1) & (disp != 0)


def eval_pair(rows=40, cols=56, seed=7):
    """Ground truth and prediction in multiples of 1/256 m, small enough that the reference's f32 running sums are exact."""
    rng = np.random.default_rng(seed)
    gt = (rng.integers(64, 256 * 40, size=(rows, cols)) / 256.0).astype(np.float32)
    gt[rng.random((rows, cols)) < 0.85] = 0
    gt[0, :8] = np.array([1.0, 1.5, 2.0, 2.00390625, 3, 0.5, 1.99609375, 2.5], np.float32)
    pred = (gt + rng.integers(-4, 5, size=(rows, cols)) / 256.0).astype(np.float32)
    pred[rng.random((rows, cols)) < 0.1] = 0
    pred[0, :8] = np.array([2.5, 1.0, 3.0, 2.0, 1.5, 0.0, 2.00390625, 2.5], np.float32)
    return gt, pred


def inputs() -> dict:
    rng = np.random.default_rng(2024)
    edge = np.where(rng.random((33, 70)) < 0.2, rng.uniform(0.5, 90.0, (33, 70)), 0.0).astype(np.float32)
    m = rng.random((33, 70)) < 0.04
    edge[m] = rng.choice(EDGE_VALUES[~np.signbit(EDGE_VALUES) | (EDGE_VALUES != 0)], int(m.sum()))      # no -0.0: outside the kernels' contract
    edge[:, 17] = 0
    lab, n_lab = synth.synth_labels(40, 56, 30, 1)
    left, right, guess = synth.synth_stereo(48, 64, 2)
    guess[5, -1], guess[9, -1], guess[20, 30] = 3000.0, 1500.0, 0.002      # disparities below 0.5 in the last column, beyond the width
    gt, pred = eval_pair()
    return {
        "lo48x64_in": synth.synth_frame(48, 64, 11),
        "lo_edge33x70_in": edge,
        "lo_gap240x48_in": gap_frame(240, 80),
        "slic60x90_img": synth.synth_lab(60, 90, 5), "slic60x90_step_nc": np.array([8, 40], np.int32),
        "slic96x160_img": synth.synth_lab(96, 160, 1), "slic96x160_step_nc": np.array([7, 40], np.int32),
        "chain96x160_in": synth.synth_frame(96, 160, 6),           # completed under the labels of slic96x160 (SLIC -> interpolate_with_superpixels)
        "lc40x56_in": synth.synth_frame(40, 56, 3), "lc40x56_labels": lab, "lc40x56_n": np.array([n_lab], np.int32),
        "stereo48x64_left": left, "stereo48x64_right": right, "stereo48x64_depth": guess,
        "eval40x56_gt": gt, "eval40x56_pred": pred,
    }


def record(R) -> dict:
    """inputs() plus the reference build's outputs."""
    z = inputs()
    for k in ("lo48x64", "lo_edge33x70", "lo_gap240x48"):
        z[k + "_out"] = R.img_completion(z[k + "_in"], "gaussian")
        z[k + "_out_noblur"] = R.img_completion(z[k + "_in"], "none")
    for k in ("slic60x90", "slic96x160"):
        step, nc = (int(v) for v in z[k + "_step_nc"])
        z[k + "_labels"], _, z[k + "_centers"] = R.slic(z[k + "_img"], step, nc, return_centers=True)
    z["chain96x160_out"] = R.interpolate_with_superpixels(z["chain96x160_in"], z["slic96x160_labels"], z["slic96x160_centers"].shape[0], 1)
    n = int(z["lc40x56_n"][0])
    z["lc40x56_out"] = R.interpolate_with_superpixels(z["lc40x56_in"], z["lc40x56_labels"], n, 1)
    z["lc40x56_out_nosp"] = R.interpolate_with_superpixels(z["lc40x56_in"], z["lc40x56_labels"], n, 0)
    z["stereo48x64_pre"], z["stereo48x64_post"] = R.stereo(z["stereo48x64_depth"], z["stereo48x64_left"], z["stereo48x64_right"])
    g, p = z["eval40x56_gt"], z["eval40x56_pred"]
    z["eval40x56_lidar_only"] = np.array([R.evaluate_lo(g, p)], np.float32)
    z["eval40x56_lidar_camera"] = np.array(R.evaluate_lc(g, p), np.float32)
    z["eval40x56_stereo_lidar"] = np.array(R.evaluate_sl(g, p), np.float32)
    return z


def same(a, b) -> bool:
    """Bit equality, NaN payloads and signs aside (a dead SLIC centre is 0 / 0, whose sign is the platform's)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(np.ascontiguousarray(a)[~na].view(u), np.ascontiguousarray(b)[~nb].view(u)))


if __name__ == "__main__":
    from oracle import ref as R
    if not R.available():
        sys.exit("oracle/_ref/libdcmt_ref.so is missing: python oracle/refbuild/build_ref.py (needs a reference checkout)")
    np.savez_compressed(OUT, **record(R))
    print(OUT, os.path.getsize(OUT), "bytes")
