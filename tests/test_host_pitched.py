"""The three oldest single-frame host entry points -- dcmt_project_points, dcmt_slic_labels, dcmt_stereo_refine -- called through
ctypes with rows that are NOT packed: every plane lives in a wider parent array, so row bytes != pitch (and 3 bytes per pixel for
the Lab image, two differently pitched inputs in one stereo call).  24 x 40 is the smallest frame at which that arithmetic can go
wrong; the results are bit-equal to the oracle and the parents' padding, pre-filled with a sentinel, is untouched.  Likewise the two
batched cv::Mat entry points, dcmt_complete_f32 and dcmt_complete_labeled_f32: two frames in one 24 x 56 parent whose frame stride
is larger than a frame."""
import ctypes

import numpy as np
import pytest

from conftest import assert_bit_equal
from depth_completion_mt_amd import Context, synth
from depth_completion_mt_amd import _lib as L
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROWS, COLS, PARENT = 24, 40, 48
SENTINEL = 0xDEADBEEF
T = synth.KITTI_T_VELO_TO_CAM
P = np.array([[20.0, 0, COLS / 2, 3.0], [0, 20.0, ROWS / 2, 0.01], [0, 0, 1, 0.002]], np.float32)     # a camera that sees the small frame


@pytest.fixture(scope="module")
def ctx():
    with Context(0, ROWS, COLS, 1) as c:
        yield c


def _parent(cols=PARENT, rows=ROWS):
    """An f32 [rows][cols] parent full of the sentinel; the frame is its first COLS columns."""
    return np.full((rows, cols), SENTINEL, dtype=np.uint32).view(np.float32)


def _in_parent(frame, parent_cols):
    """frame ([rows][cols] f32 or u8, or [rows][cols][3] u8) as the first columns of a parent of parent_cols columns."""
    if frame.dtype == np.float32:
        par = _parent(parent_cols, frame.shape[0])
    else:
        par = np.full((frame.shape[0], parent_cols) + frame.shape[2:], 0xAB, dtype=np.uint8)
    par[:, :frame.shape[1]] = frame
    return par


def _padding_untouched(par, cols=COLS):
    return bool((par.view(np.uint32)[:, cols:] == SENTINEL).all())


def _mats():
    return (np.ascontiguousarray(T, dtype=np.float32).reshape(16), np.ascontiguousarray(P, dtype=np.float32).reshape(12))


def _project(ctx, pts, out, pitch, rows=ROWS, cols=COLS):
    t, p = _mats()
    return L.lib().dcmt_project_points(ctx._h, pts.ctypes.data if pts is not None else None, 0 if pts is None else len(pts), t.ctypes.data,
                                       p.ctypes.data, out.ctypes.data, pitch, rows, cols)


def _stereo_params():
    sp = L.StereoParams()
    L.lib().dcmt_default_stereo_params(ctypes.byref(sp))
    return sp


def test_project_points_into_a_pitched_plane(ctx):
    pts = synth.synth_points(400, 3)
    want = O.project_points(pts, T, P, ROWS, COLS)
    assert (want > 0).sum() >= 20, "the test's camera must see some of its points"
    out = _parent()
    assert _project(ctx, pts, out, out.strides[0]) == L.OK
    assert_bit_equal(out[:, :COLS], want, "dcmt_project_points, pitched")
    assert _padding_untouched(out)


def test_project_points_without_points_gives_an_all_zero_plane(ctx):
    for pts in (None, np.empty((0, 4), np.float32)):
        out = _parent()
        assert _project(ctx, pts, out, out.strides[0]) == L.OK
        assert not out[:, :COLS].view(np.uint32).any()
        assert _padding_untouched(out)


@pytest.mark.parametrize("want_centers", [False, True])
def test_slic_labels_of_a_pitched_lab_image(ctx, want_centers):
    step, nc = 6, 50
    img = synth.synth_lab(ROWS, COLS, 5)
    want_lab, n, want_cen = O.slic(img, step, nc, return_centers=True)
    assert n == L.lib().dcmt_slic_num_centers(ROWS, COLS, step) == 18
    par = _in_parent(img, PARENT)                                            # 40 x 3 bytes in rows of 48 x 3
    assert par.strides[0] == 3 * PARENT
    labels = np.full(ROWS * COLS + 8, -7, dtype=np.int32)                    # (labels and centres have no pitch: a tail behind them instead)
    centers = np.full(n * 5 + 4, -7.0, dtype=np.float64)
    st = L.lib().dcmt_slic_labels(ctx._h, par.ctypes.data, par.strides[0], ROWS, COLS, step, nc, labels.ctypes.data,
                                  centers.ctypes.data if want_centers else None)
    assert st == L.OK
    assert np.array_equal(labels[:ROWS * COLS].reshape(ROWS, COLS), want_lab)
    assert (labels[ROWS * COLS:] == -7).all()
    if want_centers:
        got_cen, dead = centers[:n * 5].reshape(n, 5), np.isnan(want_cen)      # live centres bit for bit, dead ones (0 / 0) as NaN
        assert np.array_equal(np.isnan(got_cen), dead) and np.array_equal(got_cen[~dead].view(np.uint64), want_cen[~dead].view(np.uint64))
        assert (centers[n * 5:] == -7.0).all()
    else:
        assert (centers == -7.0).all()


def test_stereo_refine_of_differently_pitched_planes(ctx):
    left, right, depth = synth.synth_stereo(ROWS, COLS, 2)
    want = O.stereo_refine(depth, left, right)
    d, l, r, out = _in_parent(depth, PARENT), _in_parent(left, PARENT), _in_parent(right, 56), _parent()
    assert (d.strides[0], l.strides[0], r.strides[0]) == (4 * PARENT, PARENT, 56)
    sp = _stereo_params()
    st = L.lib().dcmt_stereo_refine(ctx._h, d.ctypes.data, d.strides[0], l.ctypes.data, l.strides[0], r.ctypes.data, r.strides[0],
                                    out.ctypes.data, out.strides[0], ROWS, COLS, ctypes.byref(sp))
    assert st == L.OK
    assert_bit_equal(out[:, :COLS], want, "dcmt_stereo_refine, pitched")
    assert _padding_untouched(out)


def test_frames_wider_than_the_context_and_short_pitches_are_invalid(ctx):
    lib = L.lib()
    pts = synth.synth_points(16, 0)
    left, right, depth = synth.synth_stereo(ROWS, PARENT, 2)                     # 48 columns wide: room for the 41-column calls
    lab, labels, out = synth.synth_lab(ROWS, PARENT, 5), np.empty(ROWS * PARENT, np.int32), _parent()
    sp = ctypes.byref(_stereo_params())

    def slic(pitch, cols=COLS):
        return lib.dcmt_slic_labels(ctx._h, lab.ctypes.data, pitch, ROWS, cols, 6, 50, labels.ctypes.data, None)

    def stereo(dp=4 * PARENT, lp=PARENT, rp=PARENT, op=4 * PARENT, cols=COLS):
        return lib.dcmt_stereo_refine(ctx._h, depth.ctypes.data, dp, left.ctypes.data, lp, right.ctypes.data, rp, out.ctypes.data, op, ROWS, cols, sp)

    # the calls themselves are fine ...
    assert _project(ctx, pts, out, 4 * PARENT) == L.OK and slic(3 * PARENT) == L.OK and stereo() == L.OK
    # ... a 24 x 41 frame in the 24 x 40 context is not ...
    assert _project(ctx, pts, out, 4 * PARENT, cols=COLS + 1) == L.E_INVALID
    assert slic(3 * PARENT, cols=COLS + 1) == L.E_INVALID
    assert stereo(cols=COLS + 1) == L.E_INVALID
    # ... and neither is a pitch one byte short of a row
    assert _project(ctx, pts, out, 4 * COLS - 1) == L.E_INVALID
    assert slic(3 * COLS - 1) == L.E_INVALID
    for short in ({"dp": 4 * COLS - 1}, {"lp": COLS - 1}, {"rp": COLS - 1}, {"op": 4 * COLS - 1}):
        assert stereo(**short) == L.E_INVALID, short
    # a packed frame (pitch == row bytes) is the limit that passes
    assert _project(ctx, pts, out, 4 * COLS) == L.OK and slic(3 * COLS) == L.OK and stereo(4 * COLS, COLS, COLS, 4 * COLS) == L.OK


# ---- dcmt_complete_f32 / dcmt_complete_labeled_f32: batch 2, 24 x 40 inside 24 x 56, three parent rows between the frames

BATCH, WIDE, GAP = 2, 56, 3


@pytest.fixture(scope="module")
def ctx2():
    with Context(0, ROWS, COLS, BATCH) as c:
        yield c


def _batch_parent(cols=WIDE, dtype=np.float32):
    """[BATCH][ROWS + GAP][cols] full of the sentinel: frame f is its [f, :ROWS, :COLS]"""
    return np.full((BATCH, ROWS + GAP, cols), SENTINEL, dtype=np.uint32).view(dtype)


def _only_the_frames_written(par):
    mask = np.ones(par.shape, bool)
    mask[:, :ROWS, :COLS] = False
    return bool((par.view(np.uint32)[mask] == SENTINEL).all())


def _complete(ctx, src, dst, lab=None, n_labels=0, *, rows=ROWS, cols=COLS, srs=None, drs=None, lrs=None, sfs=None, dfs=None):
    """the entry point on the frames at the start of the parents src / dst / lab; row and frame strides are the parents' unless given"""
    from depth_completion_mt_amd import make_params
    p = ctypes.byref(make_params())
    srs, sfs, drs, dfs = srs or src.strides[1], sfs or src.strides[0], drs or dst.strides[1], dfs or dst.strides[0]
    if lab is None:
        return L.lib().dcmt_complete_f32(ctx._h, src.ctypes.data, srs, sfs, dst.ctypes.data, drs, dfs, rows, cols, BATCH, p)
    return L.lib().dcmt_complete_labeled_f32(ctx._h, src.ctypes.data, srs, sfs, lab.ctypes.data, lrs or lab.strides[1], lab.strides[0], n_labels,
                                             dst.ctypes.data, drs, dfs, rows, cols, BATCH, p, 1)


def _batch_inputs():
    frames = synth.synth_batch(BATCH, ROWS, COLS, 11)
    labels, n_labels = synth.synth_labels(ROWS, COLS, 12, 3)
    src, lab = _batch_parent(), _batch_parent(PARENT, np.int32)         # the label planes' pitch differs from the frames'
    src[:, :ROWS, :COLS] = frames
    lab[:, :ROWS, :COLS] = labels
    return frames, labels.astype(np.int32), n_labels, src, lab


def test_complete_f32_of_a_pitched_batch(ctx2):
    frames, _, _, src, _ = _batch_inputs()
    dst = _batch_parent()
    assert (src.strides[1], src.strides[0]) == (4 * WIDE, 4 * WIDE * (ROWS + GAP)) and src.strides[0] > 4 * WIDE * ROWS
    assert _complete(ctx2, src, dst) == L.OK
    for f in range(BATCH):
        assert_bit_equal(dst[f, :ROWS, :COLS], O.img_completion(frames[f]), f"dcmt_complete_f32, pitched, frame {f}")
    assert _only_the_frames_written(dst)


def test_complete_labeled_f32_of_a_pitched_batch(ctx2):
    frames, labels, n_labels, src, lab = _batch_inputs()
    dst = _batch_parent(COLS + 1)                                        # a third pitch, one element more than a row
    assert lab.strides[1] == 4 * PARENT != src.strides[1] and dst.strides[1] == 4 * COLS + 4
    assert _complete(ctx2, src, dst, lab, n_labels) == L.OK
    for f in range(BATCH):
        assert_bit_equal(dst[f, :ROWS, :COLS], O.interpolate_with_superpixels(frames[f], labels, n_labels),
                         f"dcmt_complete_labeled_f32, pitched, frame {f}")
    assert _only_the_frames_written(dst)


def test_complete_short_pitches_and_oversized_frames_are_invalid(ctx2):
    frames, labels, n_labels, src, lab = _batch_inputs()
    row = 4 * COLS
    # the limit that passes: packed frames, pitch == row bytes ...
    packed, packed_lab, out = np.ascontiguousarray(frames), np.ascontiguousarray(np.stack([labels] * BATCH)), np.empty_like(frames)
    assert packed.strides[1] == packed_lab.strides[1] == out.strides[1] == row
    assert _complete(ctx2, packed, out) == L.OK and _complete(ctx2, packed, out, packed_lab, n_labels) == L.OK
    # ... one byte less does not, in any of the planes ...
    dst = _batch_parent()
    for short in ({"srs": row - 1}, {"drs": row - 1}):
        assert _complete(ctx2, src, dst, **short) == L.E_INVALID, short
    for short in ({"srs": row - 1}, {"drs": row - 1}, {"lrs": row - 1}):
        assert _complete(ctx2, src, dst, lab, n_labels, **short) == L.E_INVALID, short
    # ... and neither does a frame of 24 x 41 or 25 x 40 in the 24 x 40 context (the parents have the room)
    for big in ({"cols": COLS + 1}, {"rows": ROWS + 1}):
        assert _complete(ctx2, src, dst, **big) == L.E_INVALID, big
        assert _complete(ctx2, src, dst, lab, n_labels, **big) == L.E_INVALID, big
    assert (dst.view(np.uint32) == SENTINEL).all(), "a refused call writes nothing"
