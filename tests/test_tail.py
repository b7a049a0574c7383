"""k_tail: everything behind k_fp_s / k_fp_q of a device-entry-point call is one launch with one workgroup per frame, which
returns for the frames k_fp_* finished and runs the hole-closure loop (and, behind a 16-bit attempt that raised its flag, k_fp_s's
body first) for the others.  Bit-exact against the oracle: batches in which a few frames need 1, 2, 6 and 7 loop applications,
on the 16-bit and the f32 path, with spec_fill_iters below, at and above what they need; off-grid batches (attempt + rerun in
one call); the flag ring wrapping with such frames in the batch."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api, synth

pytestmark = pytest.mark.gpu

ROWS, COLS = 240, 256          # 8 fill strips, 5 post strips: every wave of a frame's workgroup walks more than one strip
K_MAX_ITERS = 64               # kMaxIters


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _gap(h0, cols=COLS):
    """The tall_gap construction: valid rows at the top and from h0 down, nothing in between; the taller the gap, the more
    applications of the 31x31 fill it takes to close."""
    a = np.zeros((ROWS, cols), np.float32)
    a[0:2] = 40.0
    a[h0:] = 12.0
    return a


GAPS = (60, 80, 198, 232)      # -> 1, 2, 6 and 7 loop applications (fill_iters 2, 3, 7 = tall_gap's, 8); checked against the oracle below


class Cases:
    """A batch of n frames: eight ordinary frames repeated, four gap frames at scattered places; expectations per distinct frame."""

    def __init__(self, O, cols=COLS, seed=77):
        self.O = O
        self.base = synth.synth_batch(8, ROWS, cols, seed)
        assert np.array_equal(np.round(self.base * 256) / 256, self.base)          # multiples of 1/256 m: the 16-bit path takes them
        self.gaps = [_gap(h, cols) for h in GAPS]
        self.kinds = list(self.base) + self.gaps                                    # kind 0..7 ordinary, 8..11 gaps
        self.info = [O.img_completion(x, return_info=True)[1] for x in self.kinds]
        assert all(i["fill_iters"] == 1 for i in self.info[:8])                    # no loop application
        assert [i["fill_iters"] - 1 for i in self.info[8:]] == [1, 2, 6, 7], self.info[8:]
        self._want = {}

    def batch(self, n):
        kind = np.arange(n) % 8
        for k, pos in enumerate((1, n // 2, n - 3, n - 1)):
            kind[pos] = 8 + k
        return np.stack([self.kinds[k] for k in kind]), kind

    def want(self, k, spec):
        """(output, fill_iters as the device reports them) of kind k with `spec` speculative applications."""
        need = self.info[k]["fill_iters"] - 1
        key = (k, spec if need > spec else None)
        if key not in self._want:
            p = self.O.default_params(max_fill_iters=spec) if need > spec else self.O.default_params()
            self._want[key] = self.O.img_completion(self.kinds[k], p)
        return self._want[key], (self.info[k]["fill_iters"] if need <= spec else -1)

    def check(self, ctx, d, kind, spec, tag, alone=None):
        import torch
        out = ctx.complete_dev(d, params=api.make_params(spec_fill_iters=spec))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        iters, st = ctx.last_fill_iters(len(kind))
        all_converge = True
        for k in np.unique(kind):
            want, it = self.want(int(k), spec)
            all_converge &= it >= 0
            idx = np.flatnonzero(kind == k)
            assert [iters[i] for i in idx] == [it] * len(idx), (tag, spec, int(k))
            assert_bit_equal(got[idx], np.broadcast_to(want, (len(idx),) + want.shape), f"{tag}, spec_fill_iters={spec}, frame kind {int(k)}")
            if alone is not None and k < 8:
                assert_bit_equal(got[idx], np.broadcast_to(alone[k], (len(idx),) + want.shape), f"{tag}: untouched frames against the same frames run alone")
        assert st == (L.OK if all_converge else L.E_NOT_CONVERGED), (tag, spec, st)
        return ctx.last_path()


def _alone(cases):
    """The eight ordinary frames as a batch of their own."""
    import torch
    with api.Context(0, ROWS, cases.base.shape[2], 8) as c:
        out = c.complete_dev(torch.from_numpy(cases.base).cuda())
        torch.cuda.synchronize()
        return out.cpu().numpy()


def test_16_bit_batch_with_a_few_frames_that_need_the_loop(O, monkeypatch):
    import torch
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")      # read by dcmt_create: the 16-bit form at this frame size too
    cases = Cases(O)
    alone = _alone(cases)
    frames, kind = cases.batch(256)
    d = torch.from_numpy(frames).cuda()
    with api.Context(0, ROWS, COLS, 256) as ctx:
        for spec in (1, 3, K_MAX_ITERS, 3, 1):
            path = cases.check(ctx, d, kind, spec, "16-bit, 256 frames", alone)
            assert "k_fp_q" in path, path


@pytest.mark.parametrize("n", (8, 128, 1024))
def test_f32_batch_with_a_few_frames_that_need_the_loop(O, monkeypatch, n):
    import torch
    monkeypatch.setenv("DCMT_FP_Q16", "0")
    cases = Cases(O)
    alone = _alone(cases)
    frames, kind = cases.batch(n)
    d = torch.from_numpy(frames).cuda()
    with api.Context(0, ROWS, COLS, n) as ctx:
        for spec in (1, 3, K_MAX_ITERS):
            path = cases.check(ctx, d, kind, spec, f"f32, {n} frames", alone)
            assert "k_fp_s" in path, path


def test_off_grid_batch_first_and_later(O, monkeypatch):
    """A batch with frames that are no multiples of 1/256 m raises the attempt's flag: k_pre_p (f32) reruns behind it and k_tail runs
    k_fp_s's body before its own phases.  As the first call of a fresh context, and behind on-grid calls; then on-grid calls again
    (the first 63 of them without an attempt)."""
    import torch
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")
    cases = Cases(O)
    off = Cases(O)
    for k in (2, 5):
        x = off.kinds[k]
        x[x > 0] += np.float32(0.003)
    off.kinds[9] = off.kinds[9] + np.float32(0.0007) * (off.kinds[9] > 0)           # a gap frame off the grid too
    off.info = [O.img_completion(x, return_info=True)[1] for x in off.kinds]
    n = 64
    g_frames, kind = cases.batch(n)
    o_frames, okind = off.batch(n)
    assert np.array_equal(kind, okind)
    d_grid, d_off = torch.from_numpy(g_frames).cuda(), torch.from_numpy(o_frames).cuda()
    with api.Context(0, ROWS, COLS, n) as ctx:
        assert "k_fp_q" in off.check(ctx, d_off, kind, 8, "off-grid, first call (attempt + rerun)")
        assert "k_fp_s" in cases.check(ctx, d_grid, kind, 8, "on-grid behind a raised flag (no attempt)")
        assert "k_fp_s" in off.check(ctx, d_off, kind, 2, "off-grid, no attempt")
    with api.Context(0, ROWS, COLS, n) as ctx:
        for spec in (8, 1):
            assert "k_fp_q" in cases.check(ctx, d_grid, kind, spec, "on-grid")
        assert "k_fp_q" in off.check(ctx, d_off, kind, 8, "off-grid behind on-grid calls (attempt + rerun)")
        assert "k_fp_s" in off.check(ctx, d_off, kind, 1, "off-grid again (the flag was seen: no attempt)")
        assert "k_fp_s" in cases.check(ctx, d_grid, kind, 8, "on-grid again (no attempt)")
        assert "k_fp_s" in cases.check(ctx, d_grid, kind, 3, "on-grid again (no attempt)")


def test_flag_ring_wraps_with_frames_that_need_the_loop(O, monkeypatch):
    """tests/test_gpu_parity.py::test_16_bit_flag_ring_over_many_calls with frames in the batch that need 1 and 7 applications:
    more attempts than the ring of flags is long on one context, three times, an off-grid batch (raised flag, rerun, 63 calls without
    an attempt) in between."""
    import torch
    monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")
    cols = 96
    grid = synth.synth_batch(8, ROWS, cols, 21)
    grid[2] = _gap(60, cols)
    grid[6] = _gap(232, cols)
    off = grid.copy()
    off[5][off[5] > 0] += np.float32(0.003)
    info = [O.img_completion(f, return_info=True)[1]["fill_iters"] for f in grid]
    assert info[2] == 2 and info[6] == 8, info
    want_grid = np.stack([O.img_completion(f) for f in grid])
    want_off = np.stack([O.img_completion(f) for f in off])
    d_grid, d_off = torch.from_numpy(grid).cuda(), torch.from_numpy(off).cuda()
    with api.Context(0, ROWS, cols, 8) as ctx:
        paths = set()

        def call(d, want, tag):
            got = ctx.complete_dev(d, params=api.make_params(spec_fill_iters=8))
            torch.cuda.synchronize()
            paths.add(ctx.last_path())
            assert_bit_equal(got.cpu().numpy(), want, tag)
            iters, st = ctx.last_fill_iters(8)
            assert st == L.OK and iters[2] == 2 and iters[6] == 8, (tag, iters, st)

        n = 0
        for rnd in range(3):
            for k in range(70):                      # 70 attempts in a row: the ring wraps
                call(d_grid, want_grid, f"round {rnd}, grid call {k}"); n += 1
            call(d_off, want_off, f"round {rnd}, off-grid call (raises its flag)"); n += 1
            for k in range(64):                      # 63 calls without an attempt, then attempts again
                call(d_grid if k % 5 else d_off, want_grid if k % 5 else want_off, f"round {rnd}, call {k} behind the raised flag"); n += 1
        assert any("k_fp_q" in p for p in paths) and any("k_fp_s" in p for p in paths), paths
        assert n == 3 * 135
