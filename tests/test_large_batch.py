"""tests/large_batch_cases.py without a GPU: the geometries' figures, the boundary frames against a frame-by-frame statement of
them, the inputs of every case (the expectations of its sources differ pairwise and from the sentinel, so a frame that holds
another frame's result or was never written cannot pass), and the verifier on fabricated outputs at a scaled-down size: it must
reject a frame left at the sentinel, a frame that holds another frame's result, and a result shifted by the 4096-byte distance a
wrapped 2^32-byte offset lands at in geometry A."""
import numpy as np
import pytest
import torch

import large_batch_cases as LB


def test_geometry_figures():
    LB.check_geometries()
    A, B, C = LB.A, LB.B, LB.C
    # the boundary frames of DESIGN.md section 24, from the element size of each plane
    assert LB.boundary_frames(A, (4,)) == [31775, 31776, 63550, 63551]
    assert LB.boundary_frames(A, (3,)) == [2 ** 31 // (3 * A.px), 2 ** 31 // (3 * A.px) + 1] and LB.boundary_frames(A, (1, 2)) == [63550, 63551]
    assert LB.boundary_frames(B, (4,)) == [1254, 1255, 2508, 2509] and LB.boundary_frames(B, (2, 1)) == [2508, 2509]
    assert LB.boundary_frames(C, (), (2 ** 31,)) == [64527, 64528] and LB.boundary_frames(C, (), (LB.SEG_PX,)) == [64525, 64526]
    seg = LB.color_seg_frames(C)
    assert LB.boundary_frames(C, (), (seg * C.px,)) == [seg - 1, seg, seg + 1]          # the last frame of segment 0, the first two of segment 1


def test_the_matcher_s_chunks_and_unique_frames():
    """dcmt_sgm_dev at geometry A through a workspace of 4096 frames: 4.43 GB, 16 chunks, the last of 4095 frames; byte 2^32 of the
    workspace lies in slot 3971 of every chunk.  The unique sources sit where the case says, beside the plane boundaries."""
    LB.check_sgm_figures()
    assert LB.sgm_figures(LB.A) == (1_081_344, 16, 4095, 3971)
    extra = LB.sgm_extra_frames(LB.A)
    assert sorted(extra) == [3971, 3972, 4095, 4096, 32767, 32768, 36739, 36740, 61439, 61440, 65411, 65412]
    lay = LB.cases()["sgm_dev A"].layout()
    assert set(extra) | {0, 31775, 31776, 63550, 63551, 65534} == set(lay.unique)
    assert len({lay.source_of(f) for f in lay.unique}) == len(lay.unique) == lay.n_src - lay.k


@pytest.mark.parametrize("g", list(LB.GEOMETRIES.values()), ids=list(LB.GEOMETRIES))
def test_boundary_frames_equal_the_frame_by_frame_statement(g):
    seg = LB.color_seg_frames(g)
    marks = (2 ** 31, LB.SEG_PX, seg * g.px, 7 * g.px, g.total_px - 1, g.total_px)
    for elems in ((4,), (2,), (1,), (3,), (4, 3, 2, 1), ()):
        for px in ((), marks[:2], marks):
            assert LB.boundary_frames(g, elems, px) == LB.boundary_frames_brute(g, elems, px), (g, elems, px)
    lay = LB.Layout(g, (4, 3, 2, 1), marks[:2])
    assert lay.unique[0] == 0 and lay.unique[-1] == g.batch - 1 and set(LB.boundary_frames(g, (4, 3, 2, 1), marks[:2])) <= set(lay.unique)
    assert lay.source_of(0) == lay.k and lay.source_of(g.batch - 1) == lay.n_src - 1
    tiled = np.setdiff1d(np.arange(g.batch), lay.unique)
    assert (lay.index[tiled] == tiled % lay.k).all() and sorted(lay.index[lay.unique]) == list(range(lay.k, lay.n_src))


@pytest.mark.parametrize("name", list(LB.cases()))
def test_inputs_of_every_case(name):
    """prepare() asserts that the expectations differ pairwise and from the sentinel; here also: the stated need is under the cap."""
    case = LB.cases()[name]
    case.prepare()
    assert 0 < case.need_bytes() < LB.CAP_BYTES, (name, case.need_bytes())


# ---------------------------------------------------------------------------------------------------------------- controls
ROWS, COLS, BATCH = 16, 64, 41                  # 4096 bytes per f32 frame: the wrap distance of geometry A is exactly one frame here


def fabricated(dtype=np.float32, trailing=(ROWS, COLS)):
    rng = np.random.default_rng(3)
    n_src = 9
    exp = rng.integers(1, 200, (n_src,) + trailing).astype(dtype)
    index = np.arange(BATCH) % 5
    index[[0, 17, 18, BATCH - 1]] = [5, 6, 7, 8]
    return torch.from_numpy(exp), torch.from_numpy(index), torch.from_numpy(exp[index].copy())


@pytest.mark.parametrize("dtype,label", [(np.float32, False), (np.int32, True), (np.uint8, False), (np.int16, False), (np.float64, False)])
def test_the_verifier_passes_a_right_output_and_rejects_the_three_wrong_ones(dtype, label):
    exp, index, right = fabricated(dtype)
    assert LB.mismatched_frames(right, exp, index) == (0, [])
    assert LB.mismatched_frames(right, exp, index, chunk_bytes=1) == (0, [])            # one frame per chunk
    LB.assert_frames("control", right, exp, index, label)

    never = right.clone()                       # a frame the kernel never reached
    LB.fill_sentinel(never[18], label)
    assert LB.is_sentinel_frame(never[18].numpy(), label) and not LB.is_sentinel_frame(right[18].numpy(), label)
    assert LB.mismatched_frames(never, exp, index, chunk_bytes=3 * never[0].numel() * never.element_size()) == (1, [18])
    with pytest.raises(AssertionError, match="never written"):
        LB.assert_frames("control", never, exp, index, label)

    other = right.clone()                       # a frame that holds another frame's result (a read or a write at a wrapped offset)
    other[23] = right[24]
    assert LB.mismatched_frames(other, exp, index) == (1, [23])
    with pytest.raises(AssertionError, match="another frame's result"):
        LB.assert_frames("control", other, exp, index, label)

    shifted = torch.empty_like(right)           # the whole result 4096 bytes late: every store at offset + 4096
    LB.fill_sentinel(shifted, label)
    flat, src = shifted.view(-1), right.view(-1)
    d = 4096 // right.element_size()
    flat[d:] = src[:-d]
    count, first = LB.mismatched_frames(shifted, exp, index)
    assert count >= BATCH - 1 and first[0] == 0
    with pytest.raises(AssertionError):
        LB.assert_frames("control", shifted, exp, index, label)


def test_the_verifier_on_per_frame_scalars_and_distinctness():
    exp, index, right = fabricated(np.int32, ())
    assert LB.mismatched_frames(right, exp, index) == (0, [])
    wrong = right.clone()
    wrong[40] += 1
    assert LB.mismatched_frames(wrong, exp, index) == (1, [40])
    a = np.arange(24, dtype=np.float32).reshape(3, 2, 4)
    LB.assert_distinct("control", a)
    with pytest.raises(AssertionError, match="same expectation"):
        LB.assert_distinct("control", np.stack([a[0], a[1], a[0]]))
    with pytest.raises(AssertionError, match="sentinel"):
        LB.assert_distinct("control", np.stack([a[0], LB.sentinel((2, 4), torch.float32, "cpu").numpy()]))
    with pytest.raises(AssertionError, match="sentinel"):
        LB.assert_distinct("control", np.stack([np.ones((2, 2), np.int32), np.full((2, 2), LB.SENT_LABEL, np.int32)]), label=True)
