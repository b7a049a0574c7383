"""The speckle filter (dcmt_filter_speckles_dev) without a GPU: the two restatements of tests/speckle_restatement.py against each other
over the parameter grid and on the matcher's outputs, scan-order independence, the named cases of the non-transitive edge relation,
a usefulness condition on a matched scene with stamped blobs, the launch plan (tests/plan_speckle_test.cpp, built against the
headers alone), the refusals that need no device and the ABI."""
import ctypes
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import sgm_restatement as G
import speckle_restatement as R
from depth_completion_mt_amd import _lib as L
from test_plan import _build_and_run

SHAPES = [(1, 1), (1, 7), (5, 1), (2, 2), (7, 9), (16, 64), (17, 65), (40, 130)]


def both(v, **kw):
    a, ca = R.flood(v, **kw)
    b, cb = R.vectorised(v, **kw)
    assert a.dtype == b.dtype == np.int16
    assert np.array_equal(a, b) and np.array_equal(ca, cb), f"{v.shape} {kw}: first at {tuple(np.argwhere(a != b)[0]) if (a != b).any() else None}"
    keep = ~ca
    assert np.array_equal(a[keep], v[keep]) and (a[ca] == R.params(**kw)["new_val"]).all()
    return a, ca


def sizes(rows, cols):
    return sorted({0, 1, 5, 200, rows * cols})


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_restatements_agree_on_random_planes(rows, cols):
    changed = kept = 0
    for i, (k, live) in enumerate(itertools.product((1, 3, 8), (0.3, 0.6, 0.9))):
        v = R.random_plane(rows, cols, k, live, 100 * rows + cols + i)
        for max_diff, max_size in itertools.product(R.MAX_DIFFS, sizes(rows, cols)):
            out, c = both(v, max_size=max_size, max_diff=max_diff)
            if max_size == 0:
                assert not c.any()
            if max_size == rows * cols:
                assert (out == -16).all()
            changed += int(c.sum())
            kept += int(((v != -16) & ~c).sum())
    assert changed > 0 and (kept > 0 or rows * cols == 1)


@functools.lru_cache(maxsize=None)
def matched(maker, rows, cols, D, seed):
    if maker == "box":
        left, right, _ = G.box_scene(rows, cols, D, seed)
    elif maker == "shifted":
        left, right = G.shifted_pair(rows, cols, seed)
    else:
        left, right = G.random_pair(rows, cols, seed)
    d16, depth = G.vectorised(left, right, num_disparities=D)
    d16.setflags(write=False)
    depth.setflags(write=False)
    return d16, depth


@pytest.mark.parametrize("maker,rows,cols,D,seed", [("box", 24, 96, 32, 1), ("shifted", 12, 40, 16, 62), ("random", 24, 96, 32, 3)])
def test_restatements_agree_on_the_matcher_s_output(maker, rows, cols, D, seed):
    d16, depth = matched(maker, rows, cols, D, seed)
    for max_diff, max_size in itertools.product(R.MAX_DIFFS, sizes(rows, cols)):
        both(d16, max_size=max_size, max_diff=max_diff)
    out, z, n = R.with_depth(R.vectorised, d16, depth)
    assert n == int((out != d16).sum()) and (z[out != d16] == 0).all() and np.array_equal(z[out == d16].view(np.uint32), depth[out == d16].view(np.uint32))
    if maker == "random":
        # textureless input: what survives the per-pixel checks is small blobs, and the default window removes all of them
        _, size = R.components(d16, 32, -16)
        assert 0 < size.max() <= 200 and (d16 != -16).sum() > 100 and (out == -16).all()


def test_scan_order_independence():
    for i, (rows, cols) in enumerate([(7, 9), (17, 33), (12, 40)]):
        v = R.random_plane(rows, cols, 3, 0.7, 40 + i)
        for max_diff, max_size in itertools.product((0, 16, 32), (1, 5, 30)):
            kw = dict(max_size=max_size, max_diff=max_diff)
            out, _ = R.flood(v, **kw)
            assert np.array_equal(R.flood(np.ascontiguousarray(v.T), **kw)[0], out.T)
            assert np.array_equal(R.flood(np.ascontiguousarray(v[::-1]), **kw)[0], out[::-1])
            assert np.array_equal(R.flood(np.ascontiguousarray(v[:, ::-1]), **kw)[0], out[:, ::-1])
            assert np.array_equal(R.flood(np.ascontiguousarray(v[::-1, ::-1]), **kw)[0], out[::-1, ::-1])


def test_the_block_whose_top_pair_is_no_edge():
    """[[-32, 32], [0, 0]] at max_diff 32: the bottom pixels are an edge, each is an edge to the pixel above it, the top pair is not.
    One component of 4: removed at max_size 4, kept at 3.  A filter that drops the bottom union sees two components of 2."""
    for rot in range(4):
        v = R.block_plane(6, 7, 2, 3, rot)
        _, size = R.components(v, 32, -16)
        assert size.max() == 4 and (size > 0).sum() == 4
        out, c = both(v, max_size=3, max_diff=32)
        assert not c.any()
        out, c = both(v, max_size=4, max_diff=32)
        assert c.sum() == 4 and (out == -16).all()
        _, size = R.components(v, 31, -16)                     # one step tighter: the bottom pair and two singletons
        assert sorted(size[size > 0].tolist()) == [1, 1, 2, 2]


def test_ramps():
    for max_diff in (1, 16, 32, 100):
        v = R.ramp(9, 14, max_diff)
        _, size = R.components(v, max_diff, -16)
        assert (size == 9 * 14).all()                           # one component, though its ends are 21 steps apart
        assert not both(v, max_size=9 * 14 - 1, max_diff=max_diff)[1].any() and both(v, max_size=9 * 14, max_diff=max_diff)[1].all()
        v = R.ramp(9, 14, max_diff + 1)
        _, size = R.components(v, max_diff, -16)
        assert (size == 1).all()                                # all singletons
        assert both(v, max_size=1, max_diff=max_diff)[1].all() and not both(v, max_size=0, max_diff=max_diff)[1].any()


def test_serpentines_at_the_threshold():
    for max_size in (1, 7, 40, 200):
        for length, removed in ((max_size, True), (max_size + 1, False)):
            v = R.serpentine(21, 20, length)
            assert (v != -16).sum() == length
            out, c = both(v, max_size=max_size, max_diff=0)
            assert c.sum() == (length if removed else 0)


def test_int16_extremes_and_other_new_vals():
    v = np.array([[-32768, 32767]], np.int16)
    assert both(v, max_size=2, max_diff=65535)[1].all()                    # joined: one component of 2
    assert not both(v, max_size=1, max_diff=65535)[1].any()
    assert both(v, max_size=1, max_diff=65534)[1].all()                    # not joined: two singletons
    assert both(v.T.copy(), max_size=1, max_diff=65534)[1].all() and not both(v.T.copy(), max_size=1, max_diff=65535)[1].any()
    for new_val in (0, 123, -32768, 32767):
        for i, (rows, cols) in enumerate([(7, 9), (17, 33)]):
            v = R.random_plane(rows, cols, 3, 0.6, 70 + i, new_val=new_val)
            v[0, 0] = -16                                                   # live here
            for max_size in (1, 5, 200):
                out, c = both(v, max_size=max_size, max_diff=16, new_val=new_val)
                assert not c[v == new_val].any()
    v = np.full((5, 8), -16, np.int16)
    assert not both(v, max_size=40)[1].any()                                # an all-new_val plane: nothing live, nothing changed
    v = np.full((5, 8), 77, np.int16)
    assert not both(v, max_size=39, max_diff=0)[1].any() and both(v, max_size=40, max_diff=0)[1].all()


def test_the_filter_removes_exactly_the_stamped_blobs():
    """A condition, not a measurement: box_scene(24, 96, 32, 1) through the vectorised matcher, eight blobs of at most 9 pixels stamped
    at disparities more than 32 sixteenths from everything around them.  With the defaults (200, 32) exactly the stamped pixels are
    changed.  The unstamped map has two components, both above 200 pixels, and the stamps split neither below the window."""
    d16, _ = matched("box", 24, 96, 32, 1)
    _, size = R.components(d16, 32, -16)
    live_sizes = sorted(set(size[size > 0].tolist()))
    assert len(live_sizes) == 2 and live_sizes[0] > 200 and live_sizes[1] == 1724, live_sizes
    assert not R.vectorised(d16)[1].any()
    stamped, mask = R.stamp_blobs(d16, 8, seed=5)
    assert 8 <= mask.sum() <= 72 and (stamped[~mask] == d16[~mask]).all()
    _, size = R.components(stamped, 32, -16)
    rest = size[~mask & (stamped != -16)]
    assert rest.min() > 200 and size[mask].max() <= 9                       # the stamps do not split what was there
    out, changed = both(stamped)
    assert np.array_equal(changed, mask)
    assert (out[mask] == -16).all() and np.array_equal(out[~mask], d16[~mask])


def test_plans(tmp_path):
    _build_and_run(tmp_path, "plan_speckle_test")


def test_abi_defaults_and_refusals_without_a_device():
    from depth_completion_mt_amd import api
    import depth_completion_mt_amd as pkg
    lib = L.lib()
    names = ("dcmt_default_speckle_params", "dcmt_filter_speckles_dev", "dcmt_filter_speckles")
    for name in names:
        assert name in L.EXPORTS and hasattr(lib, name)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (dcmt_[a-z0-9_]+)", nm))
    assert set(names) <= exported
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dcmt.h")).read()
    for name in names:
        assert len(re.findall(r"\b" + name + r"\s*\(", hdr)) == 1            # declared once, never written as a call in a comment
    assert lib.dcmt_version() == 120
    assert ctypes.sizeof(L.SpeckleParams) == 12 and [f[0] for f in L.SpeckleParams._fields_] == list(R.DEFAULTS)
    assert (L.SpeckleParams.max_size.offset, L.SpeckleParams.max_diff.offset, L.SpeckleParams.new_val.offset) == (0, 4, 8)
    p = api.make_speckle_params()
    assert (p.max_size, p.max_diff, p.new_val) == (200, 32, -16) == tuple(R.DEFAULTS.values())
    q = api.make_speckle_params(max_size=0, max_diff=65535, new_val=-32768)
    assert (q.max_size, q.max_diff, q.new_val) == (0, 65535, -32768)
    q = api.make_speckle_params(max_size=2 ** 31 - 1, max_diff=0, new_val=32767)
    assert (q.max_size, q.max_diff, q.new_val) == (2 ** 31 - 1, 0, 32767)
    lib.dcmt_default_speckle_params(None)                     # no-op
    for bad in (dict(max_size=-1), dict(max_diff=-1), dict(max_diff=65536), dict(new_val=-32769), dict(new_val=32768), dict(max_size=1.5),
                dict(max_size=2 ** 31), dict(max_diff=2 ** 40)):
        with pytest.raises(ValueError):
            api.make_speckle_params(**bad)
    # StereoSGBM's units: a window in pixels, a range in whole disparities
    assert api._speckle_kw(None, None) is None and api._speckle_kw(0, 2) is None
    assert api._speckle_kw(200, 2) == dict(max_size=200, max_diff=32) and api._speckle_kw(50, None) == dict(max_size=50)
    for bad in ((-1, 2), (200, -1), (200, 4096), (200, 0.5)):
        with pytest.raises(ValueError):
            api._speckle_kw(*bad)
    # without a context every argument check is moot: refused before anything touches a device
    assert lib.dcmt_filter_speckles_dev(None, 16, 32, None, 4, 4, 1, ctypes.byref(p), None, None) == L.E_INVALID
    assert lib.dcmt_filter_speckles_dev(None, None, None, None, 4, 4, 1, None, None, None) == L.E_INVALID
    assert lib.dcmt_filter_speckles(None, None, 8, None, 8, None, 0, 4, 4, ctypes.byref(p), None) == L.E_INVALID
    assert pkg.filter_speckles is api.filter_speckles and pkg.make_speckle_params is api.make_speckle_params
    for name in ("filter_speckles_dev", "filter_speckles"):
        assert hasattr(api.Context, name)
    import inspect
    for fn in (api.Context.sgm_dev, api.Context.sgm, api.stereo_sgm):
        sig = inspect.signature(fn).parameters
        assert sig["speckle_window"].default is None and sig["speckle_range"].default is None
