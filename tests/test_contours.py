"""SLIC's two pixel renderings without a GPU: the two restatements of tests/contours_restatement.py against each other (the
reference's column-major scan with its istaken matrix and the closed form of include/dcmt.h; the reference's double sums and integer
division), the properties the GPU test relies on, hand-worked cases, the launch plans (tests/plan_contour_test.cpp, built against the
headers alone), the refusals that need no device and the ABI."""
import numpy as np
import pytest

import contours_restatement as R
from depth_completion_mt_amd import _lib as L
from test_plan import _build_and_run

i32 = np.int32
SIZES = [(1, 1), (1, 70), (70, 1), (65, 9), (130, 3), (67, 133)]


def both(plane, what, runs=None):
    """The two restatements agree; returns the mask."""
    lit, closed = R.literal_contours(plane), R.closed_contours(plane, runs)
    assert lit.dtype == np.uint8 and lit.shape == plane.shape and set(np.unique(lit)) <= {0, 255}, what
    assert np.array_equal(lit, closed), f"{what}: {int((lit != closed).sum())} pixels differ, first at {tuple(np.argwhere(lit != closed)[0])}"
    return lit


@pytest.mark.parametrize("rows,cols", SIZES)
def test_restatements_agree_on_random_planes(rows, cols):
    for nv in (2, 3, 50):
        for seed in range(3):
            both(R.noise(rows, cols, nv, 10 * nv + seed), f"noise {rows}x{cols}, {nv} labels, seed {seed}")
    both(R.voronoi(rows, cols), f"voronoi {rows}x{cols}")


@pytest.mark.parametrize("rows,cols", SIZES)
def test_restatements_agree_on_the_adversarial_planes(rows, cols):
    cases = R.plane_cases(rows, cols)
    assert {c[0].split()[0] for c in cases} == set(R.PLANES)
    for name, plane in cases:
        both(plane, name)


def test_what_the_gpu_test_relies_on():
    """The adversarial set holds an alternating run longer than 64 rows that crosses a multiple-of-64 row, and one that starts at row 0
    of a chunk of 64 rows: the two places where the column pass hands a bit from one step to the next."""
    runs = []
    for rows, cols in SIZES:
        for name, plane in R.plane_cases(rows, cols):
            both(plane, name, runs)
    assert any(n > 64 and y // 64 != (y + n - 1) // 64 for _, y, n in runs)
    assert any(y % 64 == 0 and y > 0 for _, y, n in runs)
    assert max(n for _, _, n in runs) >= 127                 # 130 x 3, every row its own label: rows 1 .. 127 of a column and more
    # the alternating run really alternates: rows 1 .. 127 of the last column (row 128 has two untaken differing neighbours, (2, 129)
    # and (1, 129), and is a constant again)
    m = both(R.rows_own_label(130, 3), "rows 130x3")
    assert (2, 1, 127) in runs and m[:, 2].tolist() == [255 * (y & 1) for y in range(128)] + [255, 0]


def test_hand_worked_cases():
    # a vertical boundary: the left side is taken (two later neighbours differ), the right side is not (its differing neighbours are taken)
    plane = np.zeros((5, 6), i32)
    plane[:, 3:] = 1
    m = both(plane, "vertical boundary")
    assert (m[:, 2] == 255).all() and (m[:, :2] == 0).all() and (m[:, 3:] == 0).all()
    # a horizontal boundary: the upper side is taken, the lower side is not (in the last column too: (4, 2) counts (4, 3) and the
    # untaken (3, 3), and (4, 3) has nothing left: its only differing visited neighbours are taken)
    plane = np.zeros((6, 5), i32)
    plane[3:, :] = 1
    m = both(plane, "horizontal boundary")
    assert (m[2, :] == 255).all() and (m[3, :] == 0).all() and (m[[0, 1, 4, 5], :] == 0).all()
    # every row its own label: the last column alternates from row 1 down; the columns in front of it are taken (three later
    # neighbours differ) down to their last row, which has one and negates the pixel above it
    m = both(R.rows_own_label(7, 4), "rows")
    assert m[:, 3].tolist() == [0, 255, 0, 255, 0, 255, 0] and (m[:6, :3] == 255).all() and (m[6, :3] == 0).all()
    # one pixel, one label: nothing
    assert both(np.zeros((1, 1), i32), "1x1").tolist() == [[0]] and (both(R.constant(9, 9), "constant") == 0).all()
    # any int32 compares: (0, 0) sees one differing later neighbour, INT32_MIN below it; that pixel and the two of column 1 see two;
    # column 2's differing neighbours are all taken
    plane = np.array([[-1, -1, 7], [np.iinfo(i32).min, -1, 7]], i32)
    m = both(plane, "odd values")
    assert m.tolist() == [[0, 255, 0], [255, 255, 0]]
    # paint: (uchar)colour[0..2] on the taken pixels, nothing else
    img = R.image_for(2, 3, 0)
    out = R.paint(img, m, (0, 0, 200))
    assert (out[m == 255] == [0, 0, 200]).all() and np.array_equal(out[m == 0], img[m == 0]) and out.dtype == np.uint8


def test_the_means_are_integer_division_and_out_of_range_labels_are_left_alone():
    for rows, cols in SIZES:
        for seed, plane in enumerate([R.noise(rows, cols, 5, 77), R.out_of_range(rows, cols), R.voronoi(rows, cols)]):
            img = R.image_for(rows, cols, seed)
            lit, ls = R.literal_means(plane, img, 6)
            closed, cs = R.closed_means(plane, img, 6)
            assert np.array_equal(lit, closed) and np.array_equal(ls, cs) and ls.dtype == i32 and ls.shape == (6, 4)
            bad = (plane < 0) | (plane >= 6)
            assert np.array_equal(lit[bad], img[bad]) and int(ls[:, 3].sum()) == int((~bad).sum())
    assert ((R.out_of_range(67, 133) < 0) | (R.out_of_range(67, 133) >= 6)).sum() > 1000
    # truncation, not rounding: 255 + 254 over 2 pixels is 254
    plane, img = np.zeros((1, 2), i32), np.array([[[255, 1, 0], [254, 2, 0]]], np.uint8)
    out, sums = R.literal_means(plane, img, 3)
    assert out.tolist() == [[[254, 1, 0], [254, 1, 0]]] and sums.tolist() == [[509, 3, 0, 2], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert np.array_equal(R.closed_means(plane, img, 3)[0], out)


def test_plans(tmp_path):
    _build_and_run(tmp_path, "plan_contour_test")


def test_refusals_without_a_device_and_the_abi():
    from depth_completion_mt_amd import api
    import depth_completion_mt_amd as pkg
    lib = L.lib()
    for name in ("dcmt_slic_contours_dev", "dcmt_slic_cluster_means_dev", "dcmt_slic_contours", "dcmt_slic_cluster_means"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.dcmt_version() == 120
    # without a context every argument check is moot: refused before anything touches a device
    assert lib.dcmt_slic_contours_dev(None, None, 4, 4, 1, None, None, None, None) == L.E_INVALID
    assert lib.dcmt_slic_cluster_means_dev(None, None, 4, 4, 1, 1, None, None, None) == L.E_INVALID
    assert lib.dcmt_slic_contours(None, None, 16, 4, 4, None, 12, None, None, 4) == L.E_INVALID
    assert lib.dcmt_slic_cluster_means(None, None, 16, 4, 4, 1, None, 12, None) == L.E_INVALID
    assert pkg.slic_display_contours is api.slic_display_contours and pkg.slic_colour_with_cluster_means is api.slic_colour_with_cluster_means
    for name in ("slic_contours_dev", "slic_cluster_means_dev", "slic_contours", "slic_cluster_means"):
        assert hasattr(api.Context, name)
