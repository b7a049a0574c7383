"""The HIP kernels against the reference's own code directly, not through the oracle: oracle/_ref/libdcmt_ref.so (the
reference's unmodified sources compiled by oracle/refbuild/build_ref.py; it travels with the tree to a machine without a
reference checkout) where it exists, and always against tests/golden/reference_cases.npz, which records what that build
returned.  Each test runs its recorded cases first and its live cases -- the full-size ones -- when the library is
there; without it the run carries a warning that says so.  Bit equality throughout.

The reference's fill loop has no cap: a frame goes to it only after the oracle has reported that it converges (rc == 0)."""
import os
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN_DIR, assert_bit_equal
from depth_completion_mt_amd import api, synth
from oracle import oracle as O

sys.path.insert(0, GOLDEN_DIR)
import make_reference_cases as MRC  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def R():
    """oracle/ref.py if the library is there, else None (recorded cases only)."""
    from oracle import ref
    if not ref.available():
        warnings.warn("oracle/_ref/libdcmt_ref.so is absent: the GPU tests against the reference ran on the recorded cases of "
                      "tests/golden/reference_cases.npz only; the full-size and other live cases did not run")
        return None
    ref.lib()
    return ref


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(GOLDEN_DIR, "reference_cases.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sync():
    import torch
    torch.cuda.synchronize()


def ref_completion(R, x, blur="gaussian"):
    assert O.img_completion(x, O.default_params(blur=blur), return_info=True)[1]["rc"] == 0, "the reference would not return"
    return R.img_completion(x, blur)


def assert_centers(got, want, what):
    assert MRC.same(np.ascontiguousarray(got), np.ascontiguousarray(want)), f"{what}: centres differ (live ones bit for bit, dead ones as NaN)"


def test_the_reference_library_loads_where_it_exists(R):
    """Where oracle/_ref/libdcmt_ref.so is absent this passes with the fixture's warning in the run's output."""
    assert R is None or R.lib().ref_abi_version() == 1


# ------------------------------------------------------------------ img_completion: every family of kernels
def test_completion_recorded_cases(recorded):
    for k in ("lo48x64", "lo_edge33x70", "lo_gap240x48"):
        x = recorded[k + "_in"]
        with api.Context(0, x.shape[0], x.shape[1], 16) as c:
            for blur, key in (("gaussian", "_out"), ("none", "_out_noblur")):
                want = recorded[k + key]
                assert_bit_equal(c.complete(x, api.make_params(blur_type=blur)), want, f"{k} host entry, {blur}")
                for n in (3, 16):                        # the gap frame needs three passes of the loop: let the device entry run them
                    out = c.complete_dev(cu(np.stack([x] * n)), params=api.make_params(blur_type=blur, spec_fill_iters=8))
                    sync()
                    got = out.cpu().numpy()
                    for i in (0, n - 1):
                        assert_bit_equal(got[i], want, f"{k} device entry, {n} frames, frame {i}, {blur}")


def test_completion_paths_at_full_size(R, recorded):
    """Host entry (staged LDS-tile kernels), 3 and 16 frames per call (f32 streaming kernels, with and without row bands),
    256 on-grid frames per call (16-bit k_fp_q / k_tail), 256 with an off-grid frame (attempt + f32 rerun, then no attempt),
    the uint16 entry point fed what the reference's main converts.  Full-size
    frames exist only live; without the library the three families run on the recorded 48x64 frame (forced where needed)."""
    x, want = recorded["lo48x64_in"], recorded["lo48x64_out"]
    with api.Context(0, 48, 64, 16) as c:
        for kw in ({"force_staged": True}, {"force_fused": True}):
            out = c.complete_dev(cu(np.stack([x] * 16)), params=api.make_params(**kw))
            sync()
            assert_bit_equal(out[15].cpu().numpy(), want, f"recorded 48x64, {kw}: {c.last_path()}")
    if R is None:
        return
    for rows, cols in ((352, 1216), (375, 1242)):
        full_size_paths(R, rows, cols)


def full_size_paths(R, rows, cols):
    frames = synth.synth_batch(16, rows, cols, 700)
    frames[7, 100:140, 500:520] = 0
    grid = frames.copy()                                 # every frame a multiple of 1/256 m: what the 16-bit form of X6 can hold
    assert np.array_equal(np.round(grid * 256) / 256, grid)
    frames[7, 10, 10], frames[7, 300, 1000], frames[7, 200, 200] = F32(0.1), 100.5, 99.9          # frame 7 is no multiple of 1/256 m
    pick = (0, 7, 15)
    want = {i: ref_completion(R, frames[i]) for i in pick}
    want_grid = dict(want)
    want_grid[7] = ref_completion(R, grid[7])
    want_nb = {i: ref_completion(R, frames[i], "none") for i in (0, 7)}
    with api.Context(0, rows, cols, 256) as c:
        assert_bit_equal(c.complete(frames[7]), want[7], "host entry")
        assert "staged tile kernels" in c.last_path(), c.last_path()
        out = c.complete_dev(cu(frames[list(pick)]))
        sync()
        assert "k_pre_p" in c.last_path() and "k_fp_s" in c.last_path() and "k_fp_q" not in c.last_path(), c.last_path()
        for k, i in enumerate(pick):
            assert_bit_equal(out[k].cpu().numpy(), want[i], f"3 frames per call, frame {i}")
        out = c.complete_dev(cu(frames))
        sync()
        assert "k_fp_s" in c.last_path() and "k_fp_q" not in c.last_path(), c.last_path()
        for i in pick:
            assert_bit_equal(out[i].cpu().numpy(), want[i], f"16 frames per call, frame {i}")
        out = c.complete_dev(cu(frames), params=api.make_params(blur_type="none"))
        sync()
        for i in (0, 7):
            assert_bit_equal(out[i].cpu().numpy(), want_nb[i], f"16 frames per call without blur, frame {i}")
        # 256 on-grid frames: the first 16-bit attempt of this context (the calls above are too small for one).  No frame raises
        # the attempt's flag, so dst holds what k_fp_q / the 16-bit k_tail wrote -- shown by the next call, which attempts
        # again (a raised flag would have been seen there and switched the attempts off for 63 calls)
        big = cu(grid).repeat(16, 1, 1).contiguous()
        for call in (1, 2):
            out = c.complete_dev(big)
            sync()
            assert "k_fp_q" in c.last_path(), (call, c.last_path())
            for j in (0, 16 * 5 + 7, 16 * 9 + 15, 255):
                assert_bit_equal(out[j].cpu().numpy(), want_grid[j % 16], f"256 on-grid frames per call (16-bit path), call {call}, frame {j}")
        # attempt + rerun: frame 7 off the grid raises the flag, the f32 kernels redo the batch behind the attempt ...
        big = cu(frames).repeat(16, 1, 1).contiguous()
        out = c.complete_dev(big)
        sync()
        assert "k_fp_q" in c.last_path(), c.last_path()
        for j in (0, 16 * 5 + 7, 255):
            assert_bit_equal(out[j].cpu().numpy(), want[j % 16], f"256 frames per call, attempt + f32 rerun, frame {j}")
        # ... and the flag is seen by the next call: no attempt, f32 streaming kernels at 256 frames per call
        out = c.complete_dev(big)
        sync()
        assert "k_fp_s" in c.last_path() and "k_fp_q" not in c.last_path(), c.last_path()
        for j in (16 + 7, 255):
            assert_bit_equal(out[j].cpu().numpy(), want[j % 16], f"256 frames per call, no attempt, frame {j}")
        del big, out
        # DC_lidar_only/main.cpp: uint16 PNG payload, convertTo(CV_32F, 1 / 256), img_completion
        u16 = np.round(frames * 256.0).astype(np.uint16)
        u16[0, 200, 300] = 65535                         # 255.996 m
        fed = (u16.astype(np.float32) / np.float32(256.0)).astype(np.float32)
        out = c.complete_u16_dev(cu(u16.view(np.int16)), 1.0 / 256.0)
        sync()
        for i in pick:
            assert_bit_equal(out[i].cpu().numpy(), ref_completion(R, fed[i]), f"uint16 entry point, frame {i}")


# ------------------------------------------------------------------ interpolate_with_superpixels
def label_cases():
    x = synth.synth_frame(40, 56, 3)
    lab, n = synth.synth_labels(40, 56, 30, 1)
    ring = lab.copy()
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = 2
    ones = lab.copy()
    for k, (r, c) in enumerate(((0, 0), (39, 55), (20, 28), (7, 0))):
        ones[r, c] = n + k
    gone = lab.copy()
    gone[gone == 3] = 4
    lost = lab.copy()
    lost[::3, ::2] = -1
    return x, ((lab, n, "synth_labels"), (lab, n + 9, "n_labels above the highest label"), (ring, n, "a superpixel along all four borders"),
               (ones, n + 4, "one-pixel superpixels"), (gone, n, "a label without pixels"), (lost, n, "many unreached pixels"))


def test_labeled_completion(R, recorded):
    x, lab, n = recorded["lc40x56_in"], recorded["lc40x56_labels"], int(recorded["lc40x56_n"][0])
    with api.Context(0, 40, 56, 4) as c:
        for us, key in ((1, "lc40x56_out"), (0, "lc40x56_out_nosp")):
            assert_bit_equal(c.complete(x, labels=lab, n_labels=n, use_superpixel=us), recorded[key], f"recorded, host entry, use_superpixel {us}")
            out = c.complete_dev(cu(np.stack([x] * 4)), d_labels=cu(np.stack([lab] * 4)), n_labels=n, use_superpixel=us)
            sync()
            assert_bit_equal(out[3].cpu().numpy(), recorded[key], f"recorded, device entry, use_superpixel {us}")
        if R is None:
            return
        x, cases = label_cases()
        for lab, n, what in cases:
            assert O.interpolate_with_superpixels(x, lab, n, return_info=True)[1]["rc"] == 0
            want = R.interpolate_with_superpixels(x, lab, n, 1)
            assert_bit_equal(c.complete(x, labels=lab, n_labels=n), want, f"{what}, host entry")
            out = c.complete_dev(cu(np.stack([x] * 4)), d_labels=cu(np.stack([lab] * 4)), n_labels=n)
            sync()
            assert_bit_equal(out[0].cpu().numpy(), want, f"{what}, device entry")


# ------------------------------------------------------------------ SLIC, and SLIC -> labeled completion
def test_slic_labels(R, recorded):
    for k in ("slic60x90", "slic96x160"):
        img, (step, nc) = recorded[k + "_img"], (int(v) for v in recorded[k + "_step_nc"])
        with api.Context(0, img.shape[0], img.shape[1], 1) as c:
            lab, n, cent = c.slic_labels_dev(cu(img), step, nc, return_centers=True)
            sync()
            assert n == recorded[k + "_centers"].shape[0]
            assert np.array_equal(lab.cpu().numpy()[0], recorded[k + "_labels"]), k
            assert_centers(cent.cpu().numpy()[0], recorded[k + "_centers"], k)
    if R is None:
        return
    for rows, cols, step, nc in ((352, 1216, 18, 50), (375, 1242, 68, 40)):         # both callers' settings, two images per call
        imgs = np.ascontiguousarray(np.stack([synth.synth_lab(rows, cols, 60 + i) for i in range(2)]))
        with api.Context(0, rows, cols, 2) as c:
            lab, n, cent = c.slic_labels_dev(cu(imgs), step, nc, return_centers=True)
            sync()
            gl, gc = lab.cpu().numpy(), cent.cpu().numpy()
        for f in range(2):
            wl, wn, wc = R.slic(imgs[f], step, nc, return_centers=True)
            assert wn == n and np.array_equal(gl[f], wl), (rows, cols, f, int((gl[f] != wl).sum()))
            assert_centers(gc[f], wc, f"{rows}x{cols} image {f}")
    flat = np.full((75, 131, 3), 128, np.uint8)
    for step, nc, img in [(s, 40 if s != 7 else 10, synth.synth_lab(75, 131, 40 + s)) for s in (6, 7, 8, 9, 10, 11, 16)] + [(9, 40, flat), (16, 1, flat)]:
        img = np.ascontiguousarray(img)
        with api.Context(0, 75, 131, 1) as c:
            lab, n, cent = c.slic_labels_dev(cu(img), step, nc, return_centers=True)
            sync()
        wl, wn, wc = R.slic(img, step, nc, return_centers=True)
        assert wn == n and np.array_equal(lab.cpu().numpy()[0], wl), (step, nc)
        assert_centers(cent.cpu().numpy()[0], wc, f"step {step} nc {nc}")


def test_slic_then_labeled_completion_chained_on_the_device(R, recorded):
    """main_lc.cpp: generate_superpixels, then interpolate_with_superpixels with that object -- on the device without a copy
    in between, against the reference chained on the CPU (small sizes: the reference makes a full-frame pass per label)."""
    img, (step, nc) = recorded["slic96x160_img"], (int(v) for v in recorded["slic96x160_step_nc"])
    with api.Context(0, 96, 160, 1) as c:
        lab, n = c.slic_labels_dev(cu(img), step, nc)
        dense = c.complete_dev(cu(recorded["chain96x160_in"])[None], d_labels=lab, n_labels=n, params=api.make_params(force_fused=True))
        sync()
        assert_bit_equal(dense.cpu().numpy()[0], recorded["chain96x160_out"], "recorded SLIC -> interpolate_with_superpixels")
    if R is None:
        return
    for rows, cols, step, nc, seed in ((96, 160, 12, 40, 1), (75, 131, 9, 30, 2)):
        img = np.ascontiguousarray(synth.synth_lab(rows, cols, seed))
        x = synth.synth_frame(rows, cols, 5 + seed)
        wl, wn = R.slic(img, step, nc)
        assert O.interpolate_with_superpixels(x, wl, wn, return_info=True)[1]["rc"] == 0
        want = R.interpolate_with_superpixels(x, wl, wn, 1)
        with api.Context(0, rows, cols, 1) as c:
            lab, n = c.slic_labels_dev(cu(img), step, nc)
            dense = c.complete_dev(cu(x)[None], d_labels=lab, n_labels=n, params=api.make_params(force_fused=True))
            sync()
            assert n == wn
            assert_bit_equal(dense.cpu().numpy()[0], want, f"SLIC -> interpolate_with_superpixels {rows}x{cols}")


# ------------------------------------------------------------------ stereo refinement
def test_stereo_refinement(R, recorded):
    d, l, r = recorded["stereo48x64_depth"], recorded["stereo48x64_left"], recorded["stereo48x64_right"]
    assert MRC.right_edge_pixels(d).sum() == 2              # two pixels whose patch reaches column `cols`: compared too
    with api.Context(0, 48, 64, 1) as c:
        post = c.stereo_refine_dev(cu(d), cu(l), cu(r))
        pre = c.stereo_refine_dev(cu(d), cu(l), cu(r), iterations=0)
        sync()
        assert_bit_equal(pre.cpu().numpy(), recorded["stereo48x64_pre"], "recorded, before the sweeps")
        assert_bit_equal(post.cpu().numpy(), recorded["stereo48x64_post"], "recorded, after the sweeps")
    if R is None:
        return
    rows, cols, n = 375, 1242, 3
    trip = [synth.synth_stereo(rows, cols, 80 + i) for i in range(n)]
    L_, R_, G_ = (np.ascontiguousarray(np.stack([t[k] for t in trip])) for k in range(3))
    G_[1, 100:120] = 0
    G_[0, ::5, -1], G_[0, -1, ::7] = 2000.0, 1500.0         # the right edge of the patch in the last column; far depths in the last row
    assert MRC.right_edge_pixels(G_[0]).sum() >= rows // 5
    sparse = np.where(np.random.default_rng(1).random(G_.shape) < 0.04, G_, 0).astype(np.float32)
    with api.Context(0, rows, cols, n) as c:
        post = c.stereo_refine_dev(cu(G_), cu(L_), cu(R_))
        pre = c.stereo_refine_dev(cu(G_), cu(L_), cu(R_), iterations=0)
        dense = c.complete_dev(cu(sparse))                      # complete -> refine, all on the device
        both = c.stereo_refine_dev(dense, cu(L_), cu(R_))
        sync()
        post, pre, both = post.cpu().numpy(), pre.cpu().numpy(), both.cpu().numpy()
    for f in range(n):
        wpre, wpost = R.stereo(G_[f], L_[f], R_[f])
        assert_bit_equal(pre[f], wpre, f"frame {f}, iterations = 0")
        assert_bit_equal(post[f], wpost, f"frame {f}, default parameters")
    f = 2
    wdense = ref_completion(R, sparse[f])
    assert_bit_equal(both[f], R.stereo(wdense, L_[f], R_[f])[1], "img_completion -> stereo refinement")


# ------------------------------------------------------------------ evaluate_performance(s)
def test_evaluate_presets(R, recorded):
    gt, pred = recorded["eval40x56_gt"], recorded["eval40x56_pred"]
    bits = lambda v: np.atleast_1d(np.asarray(v, F32)).view(np.uint32)
    for preset in api.EVAL_PRESETS:
        for got in (api.evaluate_performance(gt, pred, preset), api.evaluate_performance(cu(gt), cu(pred), preset)):
            assert np.array_equal(bits(got), bits(recorded["eval40x56_" + preset])), (preset, got, recorded["eval40x56_" + preset])
    if R is None:
        return
    gt, pred = MRC.eval_pair(17, 93, 8)
    batch_gt, batch_pred = np.stack([gt, np.zeros_like(gt), gt]), np.stack([pred, pred, gt])
    with api.Context(0, 17, 93, 3) as c:
        for preset, (mode, thresh) in api.EVAL_PRESETS.items():
            sums = c.evaluate_dev(cu(batch_gt), cu(batch_pred), thresh, mode).cpu().numpy()
            for f in (0, 2):
                got = api.reference_performance(sums[f], preset)
                assert np.array_equal(bits(got), bits(R.EVALUATE[preset](batch_gt[f], batch_pred[f]))), (preset, f, got)
            empty = np.atleast_1d(np.asarray(api.reference_performance(sums[1], preset), F32))
            want = np.atleast_1d(np.asarray(R.EVALUATE[preset](batch_gt[1], batch_pred[1]), F32))
            assert np.isnan(empty).all() and np.isnan(want).all()            # an empty selection: 0 / 0 on both sides
