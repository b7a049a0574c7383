"""The context's buffers over its lifetime (csrc/dcmt_ctx.h: every allocation is a member that frees itself).  Scratch that grows on
demand -- the label stage's box tables, the winner plane, SLIC's cells and centres -- and scratch a first user allocates -- the
evaluation slab, the 16-bit plane, the staged kernels' column statistics -- give the bits a fresh context gives, before and after
they grow; create / destroy cycles give their memory back; a dcmt_create that fails leaves nothing behind."""
import ctypes

import numpy as np
import pytest

from depth_completion_mt_amd import Context, make_params, make_reproject_params, synth
from depth_completion_mt_amd import _lib as L

pytestmark = pytest.mark.gpu

ROWS, COLS, MAXB = 96, 160, 8
T = synth.KITTI_T_VELO_TO_CAM


def _grid_labels(rows, cols, ny, nx):
    """ny x nx rectangular labels"""
    return ((np.arange(rows)[:, None] * ny // rows) * nx + np.arange(cols)[None, :] * nx // cols).astype(np.int32)


def _done(*tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def labeled(rows, cols, batch, ny, nx):
    """dcmt_complete_labeled_f32_dev with ny * nx labels: batch * ny * nx * 2 ints in each box table"""
    import torch
    frames, lab = synth.synth_batch(batch, rows, cols, 5), np.stack([_grid_labels(rows, cols, ny, nx)] * batch)

    def call(c):
        out = c.complete_dev(torch.from_numpy(frames).cuda(), d_labels=torch.from_numpy(lab).cuda(), n_labels=ny * nx)
        assert "k_label_bbox" in c.last_path(), c.last_path()
        return _done(out)
    return call


def project(rows, cols, batch):
    """dcmt_project_points_dev: batch * rows * cols entries of the winner plane"""
    import torch
    pts = synth.synth_points(400 * batch, 3)
    offsets = np.arange(batch + 1, dtype=np.int32) * 400
    P = np.array([[20.0, 0, cols / 2, 3.0], [0, 20.0, rows / 2, 0.01], [0, 0, 1, 0.002]], np.float32)

    def call(c):
        return _done(c.project_points_dev(torch.from_numpy(pts).cuda(), torch.from_numpy(offsets).cuda(), T, P, rows, cols))
    return call


def reproject(rows, cols, batch):
    """dcmt_reproject_depth_dev on the same winner plane, a camera that sees the small frame moved a little"""
    import torch
    depth = (5.0 + 40.0 * np.random.Generator(np.random.PCG64(9)).random((batch, rows, cols))).astype(np.float32)      # dense
    M = np.eye(4, dtype=np.float32)
    M[0, 3], M[2, 3] = 0.25, -0.5
    rp = make_reproject_params(M=M, K=[[100.0, 0, cols / 2], [0, 100.0, rows / 2], [0, 0, 1]], fx=100.0, fy=100.0, cx=cols / 2, cy=rows / 2)

    def call(c):
        out, = _done(c.reproject_depth_dev(torch.from_numpy(depth).cuda(), rows, cols, rp))
        assert (out > 0).any(), "the test's camera must see some of its pixels"
        return [out]
    return call


def slic(step, batch=2):
    """dcmt_slic_labels_dev at 96 x 160: the smaller the step, the more cells and centres"""
    import torch
    img = np.stack([synth.synth_lab(ROWS, COLS, 5 + f) for f in range(batch)])

    def call(c):
        labels, n, centers = c.slic_labels_dev(torch.from_numpy(img).cuda(), step, 50, return_centers=True)
        assert n == L.lib().dcmt_slic_num_centers(ROWS, COLS, step) > 0
        return _done(labels, centers)
    return call


def evaluate(rows, cols, batch):
    import torch
    gt, pred = synth.synth_batch(batch, rows, cols, 21), synth.synth_batch(batch, rows, cols, 22)

    def call(c):
        return _done(c.evaluate_dev(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()))
    return call


def complete(rows, cols, batch, kernel, **params):
    """dcmt_complete_f32_dev down the path that launches `kernel`"""
    import torch
    frames = synth.synth_batch(batch, rows, cols, 31)              # multiples of 1/256 m: the 16-bit path takes them

    def call(c):
        out = c.complete_dev(torch.from_numpy(frames).cuda(), params=make_params(**params))
        assert kernel in c.last_path(), c.last_path()
        return _done(out)
    return call


def _q16(rows=ROWS, cols=COLS, batch=MAXB):
    return complete(rows, cols, batch, "k_fp_q")                   # (with DCMT_Q16_MIN_WAVES=0): x6q on first use


def _staged(rows=ROWS, cols=COLS, batch=MAXB):
    return complete(rows, cols, batch, "k_pre_v1", force_staged=True)      # colstat on first use


def _same_bits(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}: differs from the fresh context's result"


def test_regrowth_gives_the_bits_of_a_fresh_context(monkeypatch):
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")                  # read by dcmt_create: the 16-bit form at these batch sizes too
    slic_small = slic(40)
    steps = [("labeled, 4 labels", labeled(16, 24, 3, 2, 2)), ("labeled, 64 labels", labeled(ROWS, COLS, MAXB, 8, 8)),      # 24 -> 1024 ints
             ("project into 8 x 8", project(8, 8, 1)), ("project into 96 x 160", project(ROWS, COLS, MAXB)),                # 64 -> 122880 entries
             ("reproject", reproject(ROWS, COLS, MAXB)),                                                                    # the same plane
             ("slic, step 40", slic_small), ("slic, step 6", slic(6)), ("slic, step 40 again", slic_small),                # 3 -> 390 centres, and back
             ("evaluate", evaluate(ROWS, COLS, MAXB)), ("16-bit", _q16()), ("staged", _staged())]
    with Context(0, ROWS, COLS, MAXB) as shared:
        for what, call in steps:
            got = call(shared)
            with Context(0, ROWS, COLS, MAXB) as fresh:
                _same_bits(got, call(fresh), what)


def _free():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_create_destroy_cycles_return_their_memory(monkeypatch):
    """Free device memory after cycle 8 against free device memory after cycle 1.  The figure is device-wide: another process's
    allocations move it too."""
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")
    rows, cols, batch = 352, 1216, 16
    plane = 4 * rows * cols * batch                                # 27 MB; a cycle allocates pp[0], pp[1], x6q (half a plane), d_in, d_out, ...
    assert 2 * plane + plane // 2 >= 64 << 20
    frame = synth.synth_frame(ROWS, COLS, 1)
    calls = [labeled(16, 24, 3, 2, 2), project(8, 8, 1), reproject(ROWS, COLS, 2), slic(40), evaluate(ROWS, COLS, 2), _q16(), _staged(),
             lambda c: c.complete(frame)]                          # (the host entry point: d_in and d_out)

    def cycle():
        c = Context(0, rows, cols, batch)
        for call in calls:
            call(c)
        c.close()
        return _free()

    cycle()                                                        # warm-up: the code object loads once, torch's allocator fills its cache
    after = [cycle() for _ in range(8)]
    print("free bytes after cycles 1..8:", after)
    assert after[7] >= after[0] - plane, f"{(after[0] - after[7]) / 2**20:.1f} MiB lost over seven cycles (one plane: {plane / 2**20:.1f} MiB)"


def test_a_failed_create_leaves_nothing_behind():
    import torch
    total = torch.cuda.mem_get_info()[1]
    rows = cols = 23170
    assert rows * cols <= 0x1ffffff0
    batch = total // (4 * rows * cols) + 1
    assert batch <= 65535 and 4 * rows * cols * batch > total, "one plane must exceed the device's memory"
    small_plane = 4 * ROWS * COLS * MAXB
    call = _staged()
    with Context(0, ROWS, COLS, MAXB) as c:                        # (the code object is loaded, torch's allocator warm)
        want = call(c)
    before = _free()
    h = ctypes.c_void_p(1)
    assert L.lib().dcmt_create(0, rows, cols, int(batch), ctypes.byref(h)) == L.E_NOMEM
    assert not h.value, "a failed dcmt_create returns a null handle"
    after = _free()
    print("free bytes before / after the failed create:", before, after)
    assert abs(after - before) <= small_plane
    with Context(0, ROWS, COLS, MAXB) as c:
        _same_bits(call(c), want, "a context created after the failure")
