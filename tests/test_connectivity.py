"""The SLIC connectivity pass without a GPU: the two restatements of tests/connectivity_restatement.py against each other (the
reference's sequential scan and the component formulation of include/dcmt.h), what the result promises, the launch plan
(tests/plan_connect_test.cpp, built against the headers alone), the bound, the refusals that need no device and the ABI."""
import numpy as np
import pytest

import connectivity_restatement as R
from depth_completion_mt_amd import _lib as L
from test_plan import _build_and_run

i32 = np.int32
SIZES = [(67, 133), (17, 65), (16, 64), (15, 63), (1, 70), (70, 1)]


def both(plane, nc, what):
    """The two restatements agree; returns their result."""
    s, cs = R.sequential(plane, nc)
    p, cp = R.components(plane, nc)
    assert cs == cp and np.array_equal(s, p), what
    assert s.dtype == i32 and s.shape == plane.shape
    return s, cs


def promises(plane, nc, out, count, what):
    rows, cols = plane.shape
    assert 0 <= count <= R.max_labels(rows, cols, nc), what
    assert out.min() >= 0 and out.max() < max(1, count), what
    assert sorted(np.unique(out)) == list(range(max(1, count))), what           # every label below the count is used
    assert all(v == 1 for v in R.label_regions(out).values()), what             # every label is one 4-connected region
    # pixels of one input component stay together
    ids, _ = R.component_ids(plane)
    assert len(np.unique(ids.astype(np.int64) * (count + 1) + out)) == len(np.unique(ids)), what


def random_planes():
    """297 planes up to 23 x 29 with 1..4 labels: noise, blocky patterns, some with -1."""
    g = np.random.Generator(np.random.PCG64(2024))
    out = []
    while len(out) < 297:
        rows, cols = int(g.integers(1, 24)), int(g.integers(1, 30))
        if rows * cols < 4:
            continue
        nv = int(g.integers(1, 5))
        kind = len(out) % 3
        if kind == 0:
            a = g.integers(0, nv, (rows, cols))
        else:
            by, bx = int(g.integers(1, 4)), int(g.integers(1, 5))
            a = np.kron(g.integers(0, nv, ((rows + by - 1) // by, (cols + bx - 1) // bx)), np.ones((by, bx), np.int64))[:rows, :cols]
        a = a.astype(i32)
        if kind == 2:
            a[g.random(a.shape) < 0.1] = -1
        out.append((a, int(g.integers(1, rows * cols // 4 + 1))))
    return out


def test_restatements_agree_on_random_planes():
    small_origin = 0
    for k, (plane, nc) in enumerate(random_planes()):
        out, count = both(plane, nc, f"random plane {k} {plane.shape} nc {nc}")
        promises(plane, nc, out, count, f"random plane {k}")
        ids, _ = R.component_ids(plane)
        size = int((ids == ids[0, 0]).sum())
        small_origin += size + (size >= 2) <= R.lims_of(*plane.shape, nc) >> 2
    assert small_origin > 50                                                   # the case the origin rule is for is well covered


@pytest.mark.parametrize("rows,cols", SIZES)
def test_restatements_agree_on_the_adversarial_planes(rows, cols):
    cases = R.plane_cases(rows, cols)
    assert {c[0].split()[0] for c in cases} == set(R.PLANES)
    for name, plane, nc in cases:
        out, count = both(plane, nc, name)
        promises(plane, nc, out, count, name)


def test_what_the_planes_are_there_for():
    rows, cols, n = 67, 133, 67 * 133
    out, count = R.components(R.checkerboard(rows, cols), 1)
    assert count == 0 and (out == 0).all()
    out, count = R.components(R.small_blocks(rows, cols), 1)
    assert count == 0 and (out == 0).all()
    out, count = R.components(R.constant(rows, cols), n // 4)
    assert count == 1 and (out == 0).all()
    out, count = R.components(R.h_stripes(rows, cols), n // 4)
    assert count == rows and (out == np.arange(rows)[:, None]).all()
    out, count = R.components(R.v_stripes(rows, cols), n // 4)
    assert count == cols and (out == np.arange(cols)[None, :]).all()
    s = R.serpentine(rows, cols)
    assert R.component_ids(s)[1] == 1 + (rows - 1) // 2 and (s == 1).sum() == (rows + 1) // 2 * cols + (rows - 1) // 2
    assert len(np.unique(R.odd_values(rows, cols))) == 6 and R.odd_values(rows, cols).min() == np.iinfo(i32).min


def test_the_count_counts_the_seed_twice():
    """size 2 with lims >> 2 = 2: count = 3, not small; size 1: count = 1, small (slic.cpp:207, :227-230)."""
    plane = np.array([[0, 0, 1, 1], [2, 2, 1, 1], [2, 2, 3, 3]], i32)          # 12 pixels, nc 1: lims 12, lims >> 2 = 3
    plane[0, 0] = 5                                                            # components of 1, 1, 4, 4, 2 pixels
    out, count = both(plane, 1, "sizes")
    # the pair (count 3 <= 3) and the single pixels are small, the squares (count 5) are not
    assert count == 2 and out.tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1]]
    out, count = both(np.array([[0, 0, 1, 1, 1, 1, 1, 1]], i32), 1, "pair")   # lims 8, >> 2 = 2: the pair's count is 3
    assert count == 2 and out.tolist() == [[0, 0, 1, 1, 1, 1, 1, 1]]


def test_the_last_labelled_neighbour_wins_and_chains_follow_links():
    # column-major scan: (x, y) = (0, 0), (0, 1), (1, 0), ...  lims = 18 / 1 >> 2 = 4: components of up to 3 pixels are small
    plane = np.array([[1, 1, 1, 2, 2, 2],
                      [1, 1, 7, 2, 2, 2],
                      [1, 1, 1, 2, 2, 2]], i32)
    out, count = both(plane, 1, "island")
    assert count == 2 and out[1, 2] == 0                   # at the island's seed only (x - 1, y), (x, y - 1) and (x, y + 1) ... are labelled: label 0's
    # 8's seed (7, 0) sees the 1s to its left: label 0.  9's seed (7, 1) sees the 2s to its left (label 1) and then 8 above it: the LAST
    # one wins, and what it gives is the FINAL label of 8's component, 0 -- through 8's own link
    plane = np.array([[1, 1, 1, 1, 1, 1, 1, 8],
                      [2, 2, 2, 2, 2, 2, 2, 9]], i32)      # lims = 16 >> 2 = 4
    out, count = both(plane, 1, "chain")
    assert count == 2 and out.tolist() == [[0] * 8, [1] * 7 + [0]]


def test_a_small_origin_component_shares_label_0():
    """The stated quirk: with no labelled neighbour the component of pixel (0, 0) keeps the reference's initial adjlabel, 0 -- the label
    of the first non-small component as well, to which no link of it leads.  The two are always one region: every component in
    front of the first non-small one is small and ends, link by link, at the origin's, and the first non-small seed touches one
    of them -- so label 0, like every other label, stays 4-connected (promises() holds that on every plane above; a search over
    5595 random planes up to 8 x 9, 2523 of them with a small origin component, found no label in two regions)."""
    plane = np.array([[9, 4, 4, 4],
                      [3, 4, 4, 4],
                      [3, 4, 4, 4]], i32)                                      # lims = 12 / 1 >> 2 = 3: 9 and the 3s are small
    out, count = both(plane, 1, "origin")
    assert count == 1 and (out == 0).all()
    plane = np.array([[9, 4, 4, 4, 6, 6, 6],
                      [3, 4, 4, 4, 6, 6, 6]], i32)                             # lims >> 2 = 3: 4s are label 0 as well, 6s label 1
    out, count = both(plane, 1, "origin and two regions")
    assert count == 2 and out.tolist() == [[0, 0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 1, 1, 1]]
    assert R.label_regions(out) == {0: 1, 1: 1}


def test_max_labels_bounds_every_count():
    lib = L.lib()
    for rows, cols in SIZES + [(352, 1216), (2, 2), (1, 4)]:
        n = rows * cols
        for nc in sorted({1, 2, max(1, n // 100), max(1, n // 16), n // 4}):
            if R.lims_of(rows, cols, nc) < 4:
                continue
            m = lib.dcmt_slic_connectivity_max_labels(rows, cols, nc)
            assert m == R.max_labels(rows, cols, nc) and m >= 1
            lim4 = R.lims_of(rows, cols, nc) >> 2
            assert m * (lim4 + 1) <= n or m == 1                               # that many components of more than lims >> 2 pixels fit
    # the planes that reach it: stripes of exactly lims >> 2 + 1 pixels
    for lim4 in (1, 2, 5):
        nc = 60 // (4 * lim4)
        assert R.lims_of(1, 60, nc) >> 2 == lim4
        plane = (np.arange(60, dtype=i32) // (lim4 + 1) % 2)[None, :]
        assert R.components(plane, nc)[1] == R.max_labels(1, 60, nc) == 60 // (lim4 + 1)


def test_plans(tmp_path):
    _build_and_run(tmp_path, "plan_connect_test")


def test_refusals_without_a_device_and_the_abi():
    from depth_completion_mt_amd import api
    import depth_completion_mt_amd as pkg
    lib = L.lib()
    for name in ("dcmt_slic_connectivity_max_labels", "dcmt_slic_connectivity_dev", "dcmt_slic_connectivity"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.dcmt_version() == 120
    bound = lib.dcmt_slic_connectivity_max_labels
    assert bound(352, 1216, 1273) == 5035 == api.slic_connectivity_max_labels(352, 1216, 1273)
    for args in ((4, 4, 5), (1, 3, 1), (0, 4, 1), (4, 0, 1), (4, 4, 0), (4, 4, -1), (-4, -4, 1), (65536, 65536, 1), (1, 0x1ffffff1, 1)):
        assert bound(*args) == L.E_INVALID, args
        with pytest.raises(ValueError):
            api.slic_connectivity_max_labels(*args)
    assert bound(4, 4, 4) == 8 and bound(1, 0x1ffffff0, 1) == 3
    # without a context every argument check is moot: refused before anything touches a device
    assert lib.dcmt_slic_connectivity_dev(None, None, 4, 4, 1, 1, None, None, None) == L.E_INVALID
    assert lib.dcmt_slic_connectivity(None, None, 16, 4, 4, 1, None, 16, None) == L.E_INVALID
    assert pkg.slic_enforce_connectivity is api.slic_enforce_connectivity and pkg.slic_connectivity_max_labels is api.slic_connectivity_max_labels
    assert hasattr(api.Context, "slic_connectivity_dev") and hasattr(api.Context, "slic_connectivity")
