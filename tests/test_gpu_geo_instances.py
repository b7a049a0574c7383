"""Every instance of the seven geometric kernel templates, once: the calibration source -- one record for the whole batch (ProjMats,
ReprojK, CloudK by value) or a device table of per-frame records (ProjTable, ReprojTable, CloudTable) -- is a template type, and the
resolve and fix-up passes come in three store widths.  Every result is bit for bit the restatement that already pins the call:
oracle.project_points and np_reproject under the last-wins rule, nearest_restatement under the nearest-wins rule, each frame with
its own record (calib_cases.py) or, for the uniform source, every frame with record UNIFORM.

Which test reaches which instance (PW = 4, 2, 1 by an output 0, 2, 1 elements behind a 16-byte boundary):
    k_project_scatter<ProjMats>, k_project_resolve<PW, ProjMats>          projection, last, uniform, offsets 0 / 2 / 1
    k_project_scatter<ProjTable>, k_project_resolve<PW, ProjTable>        projection, last, table, offsets 0 / 2 / 1
    k_project_nearest_scatter<ProjMats>, k_nearest_fixup<PW>              projection, nearest, uniform, offsets 0 / 2 / 1
    k_project_nearest_scatter<ProjTable>, k_nearest_fixup<PW>             projection, nearest, table, offsets 0 / 2 / 1
    k_reproject_scatter<ReprojK>, k_reproject_resolve<PW, ReprojK>        reprojection, last, uniform, offsets 0 / 2 / 1
    k_reproject_scatter<ReprojTable>, k_reproject_resolve<PW, ReprojTable>  reprojection, last, table, offsets 0 / 2 / 1
    k_reproject_nearest_scatter<ReprojK>, k_nearest_fixup<PW>             reprojection, nearest, uniform, offsets 0 / 2 / 1
    k_reproject_nearest_scatter<ReprojTable>, k_nearest_fixup<PW>         reprojection, nearest, table, offsets 0 / 2 / 1
    k_cloud_count<CloudK>       test_gpu_calib.py: every uniform call on a frame alone (cloud_alone) of its 96 x 96 cases
    k_cloud_count<CloudTable>   test_gpu_calib.py: the 96 x 96 cases (two chunks a frame, an all-zero frame), and the bad-record test
                                (a bad record counts nothing)

Shapes, the smallest at which each path of the kernels occurs:
    projection     "project 20x30": 20 x 30, batch 3, sweeps of 300, 0 and 200 points -- a sweep boundary at point 300, inside wave 0 of
                   workgroup 1, and an empty sweep.  600 pixels a frame, 1800 in all: with 16-byte stores waves 0 and 1 of the resolve lie in
                   frame 0 (one record through the scalar cache) and wave 2 straddles pixel 600 (each lane its own frame); with 8-byte
                   stores wave 4 straddles, with 4-byte stores wave 9.  Frame 1 is empty, so the wave that straddles pixel 1200 starts
                   in a frame without winners and all of its winners lie in the NEXT frame (checked below without a GPU).
    reprojection   "reproject 40x50 -> 33x41", batch 4: 1353 pixels a frame, so frames end inside a thread's 4 (2) pixels; two scatter
                   workgroups a frame; waves on both paths of the resolve."""
import functools

import numpy as np
import pytest

import calib_cases as C
import nearest_restatement as R
from conftest import assert_bit_equal
from depth_completion_mt_amd import api
from test_gpu_calib import check_guards, dev, host, offset_view, tab

gpu = pytest.mark.gpu
f32 = np.float32

PROJECT, REPROJECT = "project 20x30", "reproject 40x50 -> 33x41"
UNIFORM = 0                                      # the record the uniform calls take for the whole batch
OFFSETS = (0, 1, 2)                              # elements behind a 16-byte boundary: 16-, 4- and 8-byte stores
PRODUCT = [(nearest, table, off) for nearest in (False, True) for table in (False, True) for off in OFFSETS]
IDS = [f"{'nearest' if n else 'last'}-{'table' if t else 'uniform'}-offset{o}" for n, t, o in PRODUCT]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0, 40, 50, 4)
    yield c
    c.close()


def reproject_rec(case, g):
    return dict(M=case.M[g], K=case.K[g], **case.kw[g])


@functools.lru_cache(maxsize=None)
def project_want(nearest, table):
    """[batch][rows][cols], computed once and shared (never modified): frame f with record f (table) or with record UNIFORM."""
    case = C.cases()[PROJECT]
    o = case.offsets
    out = []
    for f in range(case.b):
        g = f if table else UNIFORM
        out.append(R.project_frame(case.points[o[f]:o[f + 1]], case.T[g], case.P[g], case.rows, case.cols) if nearest else case.frame(f, g))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def reproject_want(nearest, table):
    case = C.cases()[REPROJECT]
    out = []
    for f in range(case.b):
        g = f if table else UNIFORM
        out.append(R.reproject_frame(case.frames[f], case.orows, case.ocols, reproject_rec(case, g)) if nearest else case.frame(f, g))
    return np.stack(out)


def test_the_projection_case_puts_waves_on_both_paths_of_the_resolve_at_every_store_width():
    """No GPU: where the winners of "project 20x30" lie, per store width.  A wave of the resolve covers 64 * PW consecutive pixels of
    the batch.  Some wave lies inside one frame and holds winners (the one-record path); the wave across pixel 600 holds winners of
    its first frame, the wave across pixel 1200 only winners of the frame BEHIND its first (the per-lane path, both ways)."""
    case = C.cases()[PROJECT]
    px = case.rows * case.cols
    assert (case.b, px, case.offsets.tolist()) == (3, 600, [0, 300, 300, 500]) and case.empty == (1,)
    for table in (False, True):
        for nearest in (False, True):
            hit = project_want(nearest, table).ravel().view(np.uint32) != 0
            assert not hit[px:2 * px].any() and hit[:px].any() and hit[2 * px:].any()
            if not table:
                continue                                               # (one record: the uniform instances choose no frame)
            for pw, first in ((4, 2), (2, 4), (1, 9)):
                run = 64 * pw
                assert first * run < px < (first + 1) * run, "the wave the docstring names straddles pixel 600"
                assert hit[:run].any(), f"PW {pw}: wave 0 lies in frame 0 and holds winners"
                assert hit[first * run:px].any(), f"PW {pw}: the wave across pixel 600 holds winners of its first frame"
                w = 2 * px // run                                      # the wave across (or starting at) pixel 1200
                if w * run < 2 * px:
                    assert hit[2 * px:(w + 1) * run].any(), f"PW {pw}: the wave across pixel 1200 holds winners of the next frame"
    # the two rules differ on this input, and so do the two sources: no case can pass with another case's expectation
    wants = [project_want(n, t) for n in (False, True) for t in (False, True)]
    assert all(not C.same_bits(a, b) for i, a in enumerate(wants) for b in wants[i + 1:])


def test_the_reprojection_case_tells_the_rules_and_the_sources_apart():
    """No GPU: the four expectations of the reprojection differ pairwise, and every frame has winners."""
    wants = [reproject_want(n, t) for n in (False, True) for t in (False, True)]
    assert all(not C.same_bits(a, b) for i, a in enumerate(wants) for b in wants[i + 1:])
    assert all(w[f].any() for w in wants for f in range(len(w)))


@gpu
@pytest.mark.parametrize("nearest,table,off", PRODUCT, ids=IDS)
def test_projection_instance_is_the_restatement_bit_for_bit(ctx, nearest, table, off):
    case = C.cases()[PROJECT]
    what = f"{PROJECT}, {'nearest' if nearest else 'last'} wins, {'table' if table else 'uniform'}, output offset {off}"
    buf, view = offset_view((case.b, case.rows, case.cols), off)
    assert view.data_ptr() % 16 == 4 * off
    pts, offsets = dev(case.points), dev(case.offsets)
    if table:
        ctx.project_points_calib_dev(pts, offsets, tab(case), case.rows, case.cols, d_sparse=view, nearest=nearest)
    else:
        ctx.project_points_dev(pts, offsets, case.T[UNIFORM], case.P[UNIFORM], case.rows, case.cols, d_sparse=view, nearest=nearest)
    got, want = host(view), project_want(nearest, table)
    for f in range(case.b):
        assert_bit_equal(got[f], want[f], f"{what}: frame {f}")
    check_guards(buf, view, what)


@gpu
@pytest.mark.parametrize("nearest,table,off", PRODUCT, ids=IDS)
def test_reprojection_instance_is_the_restatement_bit_for_bit(ctx, nearest, table, off):
    case = C.cases()[REPROJECT]
    what = f"{REPROJECT}, {'nearest' if nearest else 'last'} wins, {'table' if table else 'uniform'}, output offset {off}"
    buf, view = offset_view((case.b, case.orows, case.ocols), off)
    assert view.data_ptr() % 16 == 4 * off
    src = dev(case.frames)
    if table:
        ctx.reproject_depth_calib_dev(src, case.orows, case.ocols, tab(case), d_out=view, nearest=nearest)
    else:
        ctx.reproject_depth_dev(src, case.orows, case.ocols, api.make_reproject_params(**reproject_rec(case, UNIFORM)), d_out=view, nearest=nearest)
    got, want = host(view), reproject_want(nearest, table)
    for f in range(case.b):
        assert_bit_equal(got[f], want[f], f"{what}: frame {f}")
    check_guards(buf, view, what)
    assert_bit_equal(host(src), case.frames, "the source planes")
