"""k_tail's per-frame phase order (csrc/dcmt_kernels_tail.h), restated in numpy on the oracle's primitives and compared with the
oracle's own loop (LO :131-166): the redo of H7 into pp[0], application a + 1 while application a left holes and a < n_apps
(pp[0] <-> pp[1], holes counted into cnt[1 + a]), the plane the recompute reads (pp[a & 1]), and what dcmt_last_fill_iters makes
of the counters.  No GPU."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from oracle import oracle as O

THR = np.float32(0.1)


def fill31(x):
    return np.where(x < THR, O.dilate_rect(x, 31), x).astype(np.float32)


def tail(x6, n_apps):
    """(plane the post stage reads, counters, applications run) as k_tail leaves them for one frame."""
    cnt = np.zeros(2 + n_apps + 1, np.int64)
    x7 = fill31(x6)                                   # k_fp_*: H7, counted
    cnt[0], cnt[1] = (x6 < THR).sum(), (x7 < THR).sum()
    if cnt[1] == 0:
        return x7, cnt, 0                             # the workgroup returns: k_fp_* has finished the frame
    pp = [fill31(x6), None]                           # phase 0: the redo, not counted
    a = 0
    while a < n_apps and cnt[1 + a] > 0:              # phase a + 1 reads cnt[1 + a] behind the barrier and adds to cnt[2 + a]
        a += 1
        pp[a & 1] = fill31(pp[(a - 1) & 1])
        cnt[1 + a] = (pp[a & 1] < THR).sum()
    return pp[a & 1], cnt, a


def last_fill_iters(cnt, n_apps):
    a = 0
    while a < n_apps and cnt[1 + a] > 0:
        a += 1
    return -1 if cnt[1 + a] > 0 else a + 1


def gap(rows, h0, cols=48):
    x = np.zeros((rows, cols), np.float32)
    x[0:2] = 40.0
    x[h0:] = 12.0
    return x


@pytest.mark.parametrize("rows,h0", ((240, 30), (240, 60), (240, 80), (200, 198), (240, 232)))
@pytest.mark.parametrize("n_apps", (1, 3, 7, 64))
def test_phase_order_against_the_oracle_loop(rows, h0, n_apps):
    x = gap(rows, h0)
    x6 = O.img_completion(x, O.default_params(stop_after=O.STAGE_EXTEND))
    _, full = O.img_completion(x, return_info=True)
    need = full["fill_iters"] - 1                     # applications the frame needs
    want = O.img_completion(x, O.default_params(stop_after=O.STAGE_FILLLOOP, max_fill_iters=n_apps))
    got, cnt, a = tail(x6, n_apps)
    assert a == min(need, n_apps)
    assert_bit_equal(got, want, f"plane behind the loop, {n_apps} applications allowed, {need} needed")
    assert cnt[0] == full["holes_after_extend"]
    assert last_fill_iters(cnt, n_apps) == (full["fill_iters"] if need <= n_apps else -1)
