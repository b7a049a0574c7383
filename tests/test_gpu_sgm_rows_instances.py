"""Every instance of the rows kernel, k_sgm_rows<NPL, LDS, GUIDED, COST>, once: two disparities a lane or one, the row staged in LDS or
read from global memory, with and without a guide, absolute differences and census -- 16 cases, each at four paths, and one case of
either route at eight.  disp16, depth and both volumes, read back from the caller's workspace, are bit for bit the vectorised
restatements (tests/sgm_guided_restatement.py for absolute differences, tests/sgm_census_restatement.py for census; without a guide
and with four paths they are tests/sgm_restatement.py's).

Shapes, the smallest that reach what can go wrong:
    LDS route      5 x 70: a second pass of the staging loop, a second 64-column register window of the census left codes, and rows
                   0, 1, 3, 4 take the clamped rows of the pack and of the census codes
    global route   3 x 4097: beyond both limits of the LDS route, 4096 columns and, with a guide, 3640
    D              16 (one disparity a lane, 48 lanes idle) and 128 (two a lane)
    guide          the kinds of sgm_guided_restatement.guide_kinds, a frame each in one batch (the three that tests/test_gpu_sgm_guided.py
                   keeps at the largest shape): the hostile plane alone holds "no hint", hints beyond the range and the two floats on
                   either side of t = D
The helpers are those of tests/test_gpu_sgm.py and tests/test_gpu_sgm_guided.py."""
import functools

import numpy as np
import pytest

import sgm_census_restatement as CR
import sgm_guided_restatement as GR
import sgm_restatement as R
import test_gpu_sgm as G
import test_gpu_sgm_guided as TG
from depth_completion_mt_amd import api

gpu = pytest.mark.gpu
dev, host, same = G.dev, G.host, G.same

LDS_SHAPE, GLOBAL_SHAPE = (5, 70), (3, 4097)
LDS_BUDGET = 64 * 1024                          # kSgmLdsBudget; a column stages 16 bytes, 18 with its hint, with either cost
# (rows, cols), D, guided, cost, paths
CASES = [(shape, D, guided, cost, 4) for shape in (LDS_SHAPE, GLOBAL_SHAPE) for D in (16, 128) for guided in (False, True) for cost in CR.COSTS]
CASES += [(LDS_SHAPE, 128, True, "census", 8), (GLOBAL_SHAPE, 128, True, "absdiff", 8)]


@functools.lru_cache(maxsize=4)
def wanted(rows, cols, D, guided, cost, paths):
    """[(C or C', S, disp16)] per frame: one frame without a guide, a frame per guide kind with one."""
    left, right = G.pair("shifted", rows, cols, D)
    volumes = CR.vectorised_volumes if cost == "census" else GR.vectorised_volumes
    out = []
    for plane in (TG.guides(rows, cols, D)[1] if guided else [None]):
        C, S = volumes(left, right, plane, D, 200, 800, paths)
        out.append((C, S, R.vectorised_select(S, 10, 1)))
    return out


@gpu
@pytest.mark.parametrize("shape,D,guided,cost,paths", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_every_instance_is_the_restatement_bit_for_bit(shape, D, guided, cost, paths):
    import torch
    rows, cols = shape
    assert ((16 + 2 * guided) * cols <= LDS_BUDGET) == (shape == LDS_SHAPE)       # the route the case is there for
    want = wanted(rows, cols, D, guided, cost, paths)
    b = len(want)
    left, right = G.pair("shifted", rows, cols, D)
    planes = dev(TG.guides(rows, cols, D)[1]) if guided else None
    what = f"k_sgm_rows<{1 if D <= 64 else 2}, {shape == LDS_SHAPE}, {guided}, {cost}>, {rows}x{cols} D {D}, {paths} paths"
    one = api.sgm_workspace_bytes(rows, cols, D, 1)
    work = torch.full(((b + 1) * one,), 0xFF, dtype=torch.uint8, device="cuda")
    with api.Context(0, rows, cols, b) as ctx:
        d16, depth = ctx.sgm_dev(dev(np.stack([left] * b)), dev(np.stack([right] * b)), depth=True, d_work=work, num_disparities=D, paths=paths,
                                 d_guide=planes, cost=cost)
    want16 = np.stack([w[2] for w in want])
    same(host(d16), want16, what + ": disp16")
    same(host(depth), R.depth_of(want16), what + ": depth")
    for f, (wantC, wantS, _) in enumerate(want):
        C, S = G.workspace_volumes(work, f, rows, cols, D)
        same(C, wantC.astype(np.uint16), f"{what}, frame {f}: C")
        same(S, wantS.astype(np.uint16), f"{what}, frame {f}: S")
    assert bool((work[b * one:] == 0xFF).all()), f"{what}: the workspace was written behind its {b} frames"
    if guided:                                                      # the guides differ, and so does what they give (at D = 16 some hint nothing)
        assert len({w[0].tobytes() for w in want}) >= 3
    elif cost == "absdiff" and paths == 4:                          # the restatement every other one grew from
        plainC, plainS = G.volumes("shifted", rows, cols, D, 0, 200, 800)
        assert np.array_equal(want[0][0], plainC) and np.array_equal(want[0][1], plainS)
