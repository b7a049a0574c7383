"""The rows above V = min(first valid row of a wave's columns) - 8 are not streamed by k_fp_q / k_fp_s: the wave computes output
row V, keeps its value through the loops and stores it V more times behind its last row step.  The frames here put V everywhere: one
frame per first valid row r0 = 0 .. 87 of a 96-row frame (V = 0 and the clamp at r0 <= 8, V on and beside the 16-step block
boundaries, V small enough that interior blocks run between the row whose value is kept and the stores, V larger than the rows the
wave streams -- whatever places the top-row stores in or behind the stream has its edge cases among these), the same with ragged
tops (different first rows inside one wave,
different V in neighbouring strips), a wholly empty frame and a frame valid from row 0 beside ordinary ones, the table switched off
(V = 0 everywhere), and the benchmark's frames at 352 x 1216.  256 columns are three k_fp_q strips (both edge strips and an
interior one) and five k_fp_s strips.

Every output buffer is NaN before the call, so a top row that is never written shows; every case asserts the kernel it ran; every
frame has fill_iters == 1 in the oracle (asserted on the CPU), because k_tail rewrites a frame that needs a loop application as a
whole and would hide what k_fp_* stored.  All comparisons are bit for bit with the oracle."""
import functools

import numpy as np
import pytest

from conftest import assert_bit_equal

ROWS, COLS = 96, 256
R0S = tuple(range(88))

# how a case reaches its kernel: environment read by dcmt_create, the batch size of one call, what last_path() has to end with.
# (k_fp_s runs a batch this small in row bands unless DCMT_FBANDS says otherwise: 88 frames x 5 strips are far below one round of waves)
ROUTES = {
    "k_fp_q": ({"DCMT_Q16_MIN_WAVES": "0"}, None, "k_fp_q"),
    "k_fp_s": ({"DCMT_FP_Q16": "0", "DCMT_FBANDS": "1"}, None, "+ k_fp_s"),
    "k_fp_s_bands": ({}, 8, "+ k_fp_s (row bands)"),
}


def sweep_frame(r0, raise_by=(0,), rows=ROWS, cols=COLS):
    """Empty above r0 (plus raise_by[group] for every 16-column group), below it every pixel valid with probability 0.3, depths
    multiples of 1/256 m in [2, 80]."""
    g = np.random.Generator(np.random.PCG64(7000 + r0))
    k = np.where(g.random((rows, cols)) < 0.3, g.integers(2 * 256, 80 * 256 + 1, (rows, cols)), 0)
    first = r0 + np.asarray(raise_by)[(np.arange(cols) // 16) % len(raise_by)]
    k[np.arange(rows)[:, None] < first[None, :]] = 0
    return (k.astype(np.float32) / np.float32(256.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(frames, oracle outputs, oracle fill_iters) of a named batch, computed once and shared (never modified)."""
    from oracle import oracle as O
    if name == "sweep":
        frames = np.stack([sweep_frame(r0) for r0 in R0S])
    elif name == "ragged":
        frames = np.stack([sweep_frame(r0, (0, 7, 14)) for r0 in R0S])
    elif name == "empty":
        frames = np.stack([sweep_frame(40), np.zeros((ROWS, COLS), np.float32), sweep_frame(0), sweep_frame(70),
                           sweep_frame(23, (0, 7, 14)), np.zeros((ROWS, COLS), np.float32), sweep_frame(0), sweep_frame(9)])
    elif name == "bench":
        from depth_completion_mt_amd import synth
        frames = synth.synth_batch(16, 352, 1216, 0)
    else:
        raise KeyError(name)
    want, iters, holes = [], [], []
    for f in frames:
        w, info = O.img_completion(f, return_info=True)
        assert info["rc"] == 0
        want.append(w)
        iters.append(info["fill_iters"])
        holes.append(info.get("holes_after_extend", 0))
    frames.setflags(write=False)
    want = np.stack(want)
    want.setflags(write=False)
    return frames, want, tuple(iters), tuple(holes)


@pytest.mark.parametrize("name", ["sweep", "ragged", "empty", "bench"])
def test_every_frame_needs_no_loop_application_in_the_oracle(name):
    frames, want, iters, holes = case(name)
    assert np.array_equal(np.round(frames * 256) / 256, frames) and frames.max() <= 100.0
    assert iters == (1,) * len(frames), iters
    assert not np.isnan(want).any()
    if name in ("sweep", "ragged"):
        if name == "sweep":
            assert holes == (0,) * len(frames), holes
        valid = frames > 0
        first = np.where(valid.any(1), valid.argmax(1), ROWS)        # [frame][column]
        lo = first.min(1)
        assert lo.min() == 0 and (lo <= np.array(R0S) + 6).all() and (lo >= np.array(R0S)).all()   # the first valid row follows r0
        if name == "ragged":
            assert ((first.max(1) - lo)[:70] >= 14).all()           # different first rows inside one wave


def run(frames, want, iters_want, route, monkeypatch, rows=ROWS, cols=COLS):
    import torch
    from depth_completion_mt_amd import api
    env, batch, path_end = ROUTES[route]
    for k in ("DCMT_Q16_MIN_WAVES", "DCMT_FP_Q16", "DCMT_FBANDS", "DCMT_TOP_TABLE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                                    # read by dcmt_create
    batch = batch or len(frames)
    with api.Context(0, rows, cols, batch) as ctx:
        for b0 in range(0, len(frames), batch):
            d_dst = torch.full((batch, rows, cols), float("nan"), dtype=torch.float32, device="cuda")
            ctx.complete_dev(torch.tensor(frames[b0:b0 + batch], device="cuda"), d_dst)   # (a copy: the shared frames stay read-only)
            torch.cuda.synchronize()
            got = d_dst.cpu().numpy()
            path = ctx.last_path()
            iters, st = ctx.last_fill_iters(batch)
            assert path.endswith(path_end), (route, path)
            assert st == 0 and tuple(iters) == tuple(iters_want[b0:b0 + batch]), (route, b0, iters)
            for i in range(batch):
                assert not np.isnan(got[i]).any(), f"{route}: frame {b0 + i} has rows that were never written: " \
                                                   f"{np.flatnonzero(np.isnan(got[i]).any(1))[:8]}"
                assert_bit_equal(got[i], want[b0 + i], f"{route} frame {b0 + i}")


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", ["sweep", "ragged", "empty"])
def test_top_rows_reach_the_output(name, route, monkeypatch):
    frames, want, iters, _ = case(name)
    run(frames, want, iters, route, monkeypatch)


@pytest.mark.gpu
def test_without_the_table_nothing_changes(monkeypatch):
    """DCMT_TOP_TABLE=0: every wave streams from row 0 (V = 0), no top rows exist."""
    import torch
    from depth_completion_mt_amd import api
    frames, want, iters, _ = case("sweep")
    for k in ("DCMT_Q16_MIN_WAVES", "DCMT_FP_Q16", "DCMT_FBANDS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DCMT_TOP_TABLE", "0")
    n = len(frames)
    with api.Context(0, ROWS, COLS, n) as ctx:
        d_dst = torch.full((n, ROWS, COLS), float("nan"), dtype=torch.float32, device="cuda")
        ctx.complete_dev(torch.tensor(frames, device="cuda"), d_dst)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
        assert ctx.last_path().endswith("+ k_fp_s"), ctx.last_path()
        got_iters, st = ctx.last_fill_iters(n)
    assert st == 0 and tuple(got_iters) == iters
    for i in range(n):
        assert_bit_equal(got[i], want[i], f"no table, frame {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["k_fp_q", "k_fp_s_default"])
def test_benchmark_frames(route, monkeypatch):
    """352 x 1216, V about 100: the kept value crosses the interior loop."""
    frames, want, iters, _ = case("bench")
    if route == "k_fp_s_default":
        monkeypatch.setitem(ROUTES, route, ({}, None, "+ k_fp_s (row bands)"))
    run(frames, want, iters, route, monkeypatch, 352, 1216)
