"""k_fp_q's horizontal 31-maximum by where a row's holes lie in the wave (csrc/dcmt_kernels_fp_q16.h, fill_step): a row step whose
holes all lie in lanes 8..55 leaves the scans of the halo register B out, a hole in lanes 0..7 or 56..63 takes them.  Batches of
8 frames of 96 x 256 (three strips, two seams, both edge strips, rows enough for the interior body) on the 1/256 m grid, dense
but for planted empty rectangles, so that the oracle's X6 (stop_after = EXTEND) has its holes exactly where a case wants them;
every case first asserts that on the oracle alone, with the strip geometry restated here, then compares the 16-bit path's output
with the oracle bit for bit.  Frame k of a batch is the case's plan moved down by k rows: every phase of the 16-step block."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from depth_completion_mt_amd import _lib as L
from depth_completion_mt_amd import api

pytestmark = pytest.mark.gpu

ROWS, COLS, BATCH = 96, 256, 8
VW, H = 120, 4                              # FpQ: output columns per strip, columns lost per side; strip origin = strip * VW - H
STRIPS = (COLS + VW - 1) // VW
LANE = np.arange(64)
LO, HI, MID = LANE < 8, LANE >= 56, (LANE >= 8) & (LANE < 56)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def dense(seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.integers(2 * 256, 80 * 256, (ROWS, COLS)) / 256.0).astype(np.float32)


def plant(x, r0, c0, h, w):
    """Empties the rectangle that leaves X6 with the hole rows r0 .. r0+h-1 x columns c0 .. c0+w-1: H3 (5x5, the kernel as
    compiled), H4 (5x5 close) and H5 (7x7 fill) eat 4 rows above, 5 below, 2 columns left and 5 right of it.  (Every case
    asserts the result on the oracle's X6; nothing rests on these four numbers.)"""
    x[max(r0 - 4, 0):r0 + h + 5, max(c0 - 2, 0):c0 + w + 5] = 0


def lane_holes(holes, strip):
    """[rows][64]: does lane l of the strip's wave see a hole in the row?  Lane l holds the column pair at gx0 + 2l, clamped into
    the frame as the kernel's loads are (the out-of-image lanes of an edge strip repeat the edge pair)."""
    c = np.clip(strip * VW - H + 2 * LANE, 0, COLS - 2)
    return holes[:, c] | holes[:, c + 1]


class Case:
    def __init__(self, O, frames):
        self.O = O
        self.frames = np.stack(frames)
        assert self.frames.shape == (BATCH, ROWS, COLS)
        assert np.array_equal(np.round(self.frames * 256) / 256, self.frames)      # the 1/256 m grid: the 16-bit path takes them
        p6 = O.default_params(stop_after=O.STAGE_EXTEND)
        self.holes = [O.img_completion(x, p6) < np.float32(0.1) for x in self.frames]
        done = [O.img_completion(x, return_info=True) for x in self.frames]
        self.want = np.stack([d[0] for d in done])
        self.iters = [d[1]["fill_iters"] for d in done]

    def rows_where(self, strip, pred):
        """per frame: the rows in which the strip's wave has a hole and pred(lane mask of the row) holds"""
        out = []
        for h in self.holes:
            m = lane_holes(h, strip)
            out.append([r for r in range(ROWS) if m[r].any() and pred(m[r])])
        return out

    def run(self, monkeypatch):
        import torch
        monkeypatch.setenv("DCMT_Q16_MIN_WAVES", "0")      # read by dcmt_create: the 16-bit form at this frame size and batch
        with api.Context(0, ROWS, COLS, BATCH) as ctx:
            out = ctx.complete_dev(torch.from_numpy(self.frames).cuda())
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            iters, st = ctx.last_fill_iters(BATCH)
            assert "k_fp_q" in ctx.last_path(), ctx.last_path()
        assert st == L.OK and list(iters) == self.iters, (st, list(iters), self.iters)
        for f in range(BATCH):
            assert_bit_equal(got[f], self.want[f], f"frame {f}")


def moved(plan, seed):
    """frames k = 0..7: plan(x, k) plants the case's rectangles k rows further down"""
    frames = []
    for k in range(BATCH):
        x = dense(seed + k)
        plan(x, k)
        frames.append(x)
    return frames


def at_least(rows_per_frame, n=8):
    return all(len(r) >= n for r in rows_per_frame)


def test_holes_only_in_lanes_8_to_55(O, monkeypatch):
    def plan(x, k):
        plant(x, 6 + k, 30, 6, 40)            # strip 0, columns 30..69, also rows of the border body
        plant(x, 24 + k, 150, 14, 3)          # strip 1 (origin 116): lanes 17, 18
        plant(x, 44 + k, 16, 10, 88)          # strip 0, lanes 10..53
        plant(x, 70 + k, 140, 9, 60)          # strip 1, the wave's last blocks
    c = Case(O, moved(plan, 100))
    for s in (0, 1):
        assert at_least(c.rows_where(s, lambda m: not (m & (LO | HI)).any()), 16)
    for s in range(STRIPS):
        assert not any(c.rows_where(s, lambda m: (m & (LO | HI)).any())), s       # no wave sees a hole in a halo lane: A alone throughout
    c.run(monkeypatch)


def test_holes_in_lanes_0_to_7(O, monkeypatch):
    def plan(x, k):
        plant(x, 20 + k, 124, 10, 8)          # strip 1, lanes 4..7 alone (columns 124..131 lie behind strip 0's last lane)
        plant(x, 40 + k, 126, 10, 30)         # lanes 5..19: the prefix runs from B's lanes into A's
        plant(x, 60 + k, 2, 9, 5)             # strip 0, lanes 3..5 (columns 2..6)
    c = Case(O, moved(plan, 200))
    assert at_least(c.rows_where(1, lambda m: (m & LO).any() and not (m & (MID | HI)).any()))
    assert at_least(c.rows_where(1, lambda m: (m & LO).any() and (m & MID).any() and not (m & HI).any()))
    assert at_least(c.rows_where(0, lambda m: (m & LO).any() and not (m & HI).any()))
    c.run(monkeypatch)


def test_holes_in_lanes_56_to_63(O, monkeypatch):
    def plan(x, k):
        plant(x, 20 + k, 108, 10, 8)          # strip 0, lanes 56..59 alone (columns 108..115 lie in front of strip 1's first lane)
        plant(x, 40 + k, 90, 10, 24)          # lanes 47..58: the suffix runs from B's lanes into A's
        plant(x, 60 + k, 230, 9, 5)           # strip 1, lanes 57..59 (columns 230..234)
    c = Case(O, moved(plan, 300))
    assert at_least(c.rows_where(0, lambda m: (m & HI).any() and not (m & (MID | LO)).any()))
    assert at_least(c.rows_where(0, lambda m: (m & HI).any() and (m & MID).any() and not (m & LO).any()))
    assert at_least(c.rows_where(1, lambda m: (m & HI).any() and not (m & LO).any()))
    c.run(monkeypatch)


def test_holes_only_in_the_halo_columns_the_neighbour_owns(O, monkeypatch):
    """A strip's lanes 0, 1 and 62, 63 hold the 4 + 4 columns that go to the median and the Gaussian; the neighbouring strip stores them."""
    def plan(x, k):
        plant(x, 18 + k, 120, 10, 4)          # strip 0's lanes 62, 63 = strip 1's own lanes 2, 3
        plant(x, 38 + k, 116, 10, 4)          # strip 1's lanes 0, 1 = strip 0's own lanes 60, 61
        plant(x, 58 + k, 236, 10, 4)          # strip 2's lanes 0, 1 = strip 1's own lanes 60, 61
        plant(x, 72 + k, 240, 9, 4)           # strip 1's lanes 62, 63 = strip 2's own lanes 2, 3
    c = Case(O, moved(plan, 400))
    right_halo, left_halo = LANE >= 62, LANE < 2
    assert at_least(c.rows_where(0, lambda m: not (m & ~right_halo).any()))
    assert at_least(c.rows_where(1, lambda m: not (m & ~left_halo).any()))
    assert at_least(c.rows_where(1, lambda m: not (m & ~right_halo).any()))
    # (strip 2 is the right edge strip: its lanes from 10 on repeat the frame's last pair, no hole there)
    assert at_least(c.rows_where(2, lambda m: not (m & ~left_halo).any()))
    c.run(monkeypatch)


def test_rows_of_the_two_kinds_alternate(O, monkeypatch):
    """The fill values of a row are computed in one step and applied in the next: rows that leave B out between rows that take it.
    Strip 0: one tall hole in lanes 8..55 through all the rows, one-row holes in halo lanes on every second row -- four column
    slots for them (a one-row hole takes ten empty rows), so runs of eight alternating rows, a new run every twelve."""
    slots = (0, 9, 108, 117)                  # lanes 0, 4 | 56, 60 of strip 0 (origin -4)

    def plan(x, k):
        plant(x, 14 + k, 40, 46, 20)
        for run in (15, 27, 39, 51):
            for i, col in enumerate(slots):
                plant(x, run + 2 * i + k, col, 1, 1)
    c = Case(O, moved(plan, 500))
    for h in c.holes:
        m = lane_holes(h, 0)
        kind = ["-" if not m[r].any() else ("B" if (m[r] & (LO | HI)).any() else "A") for r in range(ROWS)]
        s = "".join(kind)
        assert s.count("ABA") >= 8 and s.count("B") >= 16 and "BB" not in s, s
    c.run(monkeypatch)


def test_holes_in_the_first_and_last_image_columns(O, monkeypatch):
    def plan(x, k):
        plant(x, 16 + k, 0, 12, 1)            # column 0 alone: strip 0's lane 2 and the two lanes left of it that repeat it
        plant(x, 36 + k, 255, 12, 1)          # column 255 alone: every out-of-image lane of strip 2 repeats it
        plant(x, 56 + k, 0, 10, 14)           # columns 0..13
        plant(x, 74 + k, 246, 9, 10)          # columns 246..255
    c = Case(O, moved(plan, 600))
    for h in c.holes:
        assert h[:, 0].sum() >= 16 and h[:, COLS - 1].sum() >= 16
        assert (h[:, 0] & ~h[:, 1]).sum() >= 8 and (h[:, COLS - 1] & ~h[:, COLS - 2]).sum() >= 8
    assert at_least(c.rows_where(0, lambda m: m[:3].all()))                        # the replicated lanes see the hole too
    assert at_least(c.rows_where(2, lambda m: m[10:].all()))
    c.run(monkeypatch)


def test_a_frame_the_tail_has_to_redo(O, monkeypatch):
    """An empty 40 x 40 block: H7 leaves holes in it, k_fp_q counts them and k_tail redoes the frame -- beside frames of the
    other kinds that it must leave alone."""
    def plan(x, k):
        if k == 5:
            x[30:70, 100:140] = 0
        elif k % 2:
            plant(x, 20 + k, 150, 12, 30)
        else:
            plant(x, 30 + k, 108, 10, 12)
    c = Case(O, moved(plan, 700))
    assert c.iters[5] >= 2 and all(i == 1 for f, i in enumerate(c.iters) if f != 5), c.iters
    assert c.holes[5][30:70, 100:140].sum() > 31 * 8                               # wider than the 31-maximum closes in one pass
    c.run(monkeypatch)
