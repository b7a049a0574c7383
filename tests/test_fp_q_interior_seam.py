"""k_fp_q runs the blocks of 16 row steps whose rows no column clamps and whose output rows need no border rule through an interior
body (one dword load per column pair, no row-range tests, the Gaussian's plain rows); every other block through the border
body.  The frames here put the seam between the two everywhere: ragged tops (first valid rows that jump by more than 32 rows from
one group of columns to the next), columns that end far above the bottom, empty columns inside a strip and in the halo of an edge
strip, frames valid from row 0 (cold start, V = 0), every row count modulo 16 (the length of the last block), heights without any
interior block, one strip, two strips and 1216 columns.  All depths are multiples of 1/256 m; the 16-bit path is forced at a small
batch with DCMT_Q16_MIN_WAVES=0, the f32 twin (k_fp_s) runs the same frames at the default dispatch.  Both are compared bit for
bit with the oracle.  The CPU test checks the oracle side first: every frame converges within the default loop cap."""
import numpy as np
import pytest

from conftest import assert_bit_equal

BATCH = 8
# every residue of the row count modulo 16 at one strip (rows + 35 - 32 = 0, 1, 4, 15, 16 modulo 16 among them), then two strips, three,
# a width whose right edge strip is nearly empty, heights without an interior block (an interior block needs 55 streamed rows), 1216 columns
SHAPES = [(r, 96) for r in range(100, 116)] + [(109, 200), (141, 250), (125, 366), (40, 200), (54, 120), (57, 96), (160, 1216), (352, 1216)]


def seam_frame(rows, cols, kind, seed):
    """One frame on the 1/256 m grid.  kind 0: valid from row 0; 1: ragged top; 2: ragged top and bottom; 3: as 2 with empty columns."""
    g = np.random.Generator(np.random.PCG64(seed))
    k = np.where(g.random((rows, cols)) < 0.3, g.integers(300, 21000, (rows, cols)), 0)
    k[g.random((rows, cols)) < 0.002] = 25600                      # the 100 m code among them
    first = np.zeros(cols, int)
    last = np.full(cols, rows - 1)
    if kind >= 1:
        top = int(g.integers(0, 30)) if rows > 60 else int(g.integers(0, 8))
        reach = max(min(70, rows - top - 12), 1)
        c = n = 0
        while c < cols:                                            # groups wider than the front end's horizontal reach keep their own rows
            w = int(g.integers(22, 48))
            jump = int(g.integers(0, min(8, reach))) if n % 2 else int(g.integers(min(40, reach - 1), reach))   # tall steps between groups
            n += 1
            first[c:c + w] = top + jump
            if kind >= 2 and g.random() < 0.5:
                last[c:c + w] = max(rows - 1 - int(g.integers(0, reach)), top + jump + 4)
            c += w
        first[::41] = top                                           # every strip has a column that starts at the frame's top row
    rr = np.arange(rows)[:, None]
    k[(rr < first[None, :]) | (rr > last[None, :])] = 0
    k[first, np.arange(cols)] = 5000 + 7 * np.arange(cols)
    k[last, np.arange(cols)] = 9000 + 3 * np.arange(cols)
    if kind == 0:
        k[0] = 4000 + np.arange(cols)
    if kind == 3:
        k[:, 50:62] = 0                                             # inside a strip
        k[:, :3] = 0
        k[:, cols - 3:] = 0                                         # the image's own edge columns
        if cols > 140:
            k[:, 124:134] = 0                                       # right halo of the left edge strip
            s = (cols + 119) // 120 - 1                             # left halo of the right edge strip (origin 120 s - 4)
            k[:, max(120 * s - 14, 0):120 * s - 5] = 0
    return (k.astype(np.float32) / np.float32(256.0)).astype(np.float32)


def seam_batch(rows, cols):
    kinds = (0, 1, 2, 3, 1, 2, 3, 0)
    return np.stack([seam_frame(rows, cols, kinds[i], 100000 * rows + 100 * cols + i) for i in range(BATCH)])


def test_seam_frames_are_on_the_grid_and_converge_in_the_oracle():
    from oracle import oracle as O
    seen = set()
    for rows, cols in SHAPES[:-1]:                                  # (the largest shape is the second largest with more rows)
        frames = seam_batch(rows, cols)
        assert np.array_equal(np.round(frames * 256) / 256, frames) and frames.max() <= 100.0
        for i in range(BATCH):
            valid = frames[i] > 0
            assert valid.any()
            fr = np.where(valid.any(0), valid.argmax(0), -1)
            live = fr[fr >= 0]
            if i in (1, 2, 3, 4, 5, 6) and rows > 100:
                assert np.abs(np.diff(live)).max() > 32, (rows, cols, i)   # ragged: neighbouring columns start more than 32 rows apart
            _, info = O.img_completion(frames[i], return_info=True)
            assert info["rc"] == 0 and info["fill_iters"] < 64, (rows, cols, i, info)
        seen.add((rows + 3) % 16)
    assert seen == set(range(16))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_interior_and_border_blocks_give_the_oracles_bits(rows, cols, monkeypatch):
    import torch
    from depth_completion_mt_amd import api
    from oracle import oracle as O
    frames = seam_batch(rows, cols)
    want, iters_want = [], []
    for f in frames:
        w, info = O.img_completion(f, return_info=True)
        want.append(w)
        iters_want.append(info["fill_iters"])
    for kernel, env in (("k_fp_q", "0"), ("k_fp_s", None)):
        if env is None:
            monkeypatch.delenv("DCMT_Q16_MIN_WAVES", raising=False)
        else:
            monkeypatch.setenv("DCMT_Q16_MIN_WAVES", env)           # read by dcmt_create
        with api.Context(0, rows, cols, BATCH) as ctx:
            out = ctx.complete_dev(torch.from_numpy(frames).cuda())
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            path = ctx.last_path()
            iters, st = ctx.last_fill_iters(BATCH)
        assert kernel in path, (kernel, path)
        assert st == 0 and list(iters) == iters_want, (kernel, iters, iters_want)
        for i in range(BATCH):
            assert_bit_equal(got[i], want[i], f"{kernel} {rows}x{cols} frame {i}")
