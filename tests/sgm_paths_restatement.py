"""Two independent statements of the stereo matcher's volumes with eight paths (include/dcmt.h, step 3 with paths == 8;
dcmt_sgm_paths_dev), built on tests/sgm_restatement.py: the block cost C, the selection (*_select) and the depth (depth_of) are its own.

literal     every one of the eight directions spelled out on Python ints: the start pixels of a direction listed explicitly (the
            frame's first row and first column as the direction sees them), each path walked pixel by pixel until it leaves the frame.
vectorised  the four-path sum of sgm_restatement.vectorised_volumes plus the diagonals, which are extracted with index arrays -- one
            row of indices per diagonal offset, padded behind its end -- and scanned all at once; the anti-diagonals are the diagonals
            of the mirrored frame.

Neither walks the wrapped lines of k_sgm_diag; tests/test_sgm_paths.py restates those on their own and holds them against these.
Both assert S <= 65535 and S <= 8 * (6375 + p2)."""
import numpy as np

import sgm_restatement as R

MAX_P2 = 1800                                   # eight paths: 8 * (6375 + 1800) = 65400
S_BOUND = 8 * (25 * 255 + MAX_P2)
AXIS = ((0, 1), (0, -1), (1, 0), (-1, 0))       # (dy, dx): the four paths of dcmt_sgm_dev
DIAGONAL = ((1, 1), (-1, -1), (1, -1), (-1, 1))


def params(paths=8, **kw):
    p = R.params(**kw)
    assert paths in (4, 8) and (paths == 4 or p["p2"] <= MAX_P2), (paths, p["p2"])
    return p


# ---- the statement, pixel by pixel ---------------------------------------------------------------------------------------------------
def literal_starts(rows, cols, dy, dx):
    """The pixels of the frame that have no predecessor (y - dy, x - dx) inside it, listed: the row the direction enters by, if it moves
    in y, and the column it enters by, if it moves in x, without the corner twice."""
    starts = []
    if dy:
        y0 = 0 if dy > 0 else rows - 1
        starts += [(y0, x) for x in range(cols)]
    if dx:
        x0 = 0 if dx > 0 else cols - 1
        starts += [(y, x0) for y in range(rows) if not (dy and y == (0 if dy > 0 else rows - 1))]
    return starts


def literal_paths(C, directions, p1, p2):
    """sum over the directions of L_r, as nested lists [rows][cols][D] of ints; C likewise."""
    rows, cols, D = len(C), len(C[0]), len(C[0][0])
    S = [[[0] * D for _ in range(cols)] for _ in range(rows)]
    for dy, dx in directions:
        seen = 0
        for y, x in literal_starts(rows, cols, dy, dx):
            assert not (0 <= y - dy < rows and 0 <= x - dx < cols)
            prev = None
            while 0 <= y < rows and 0 <= x < cols:
                c = C[y][x]
                if prev is None:
                    cur = list(c)
                else:
                    m = min(prev)
                    cur = []
                    for d in range(D):
                        best = min(prev[d], m + p2)
                        if d - 1 >= 0:
                            best = min(best, prev[d - 1] + p1)
                        if d + 1 < D:
                            best = min(best, prev[d + 1] + p1)
                        cur.append(c[d] + best - m)
                s = S[y][x]
                for d in range(D):
                    assert c[d] <= cur[d] <= c[d] + p2
                    s[d] += cur[d]
                prev = cur
                seen += 1
                y, x = y + dy, x + dx
        assert seen == rows * cols, (dy, dx, seen)          # the paths of one direction cover every pixel once
    return S


def literal_volumes(left, right, D, p1, p2, paths=8, C=None):
    """(C, S) int64 [rows][cols][D].  C: the block cost if the caller has it already (it does not depend on p1, p2)."""
    if C is None:
        C = R.literal_volumes(left, right, D, 0, 0)[0]
    S = np.array(literal_paths(C.tolist(), AXIS + (DIAGONAL if paths == 8 else ()), p1, p2), dtype=np.int64)
    assert C.max() <= 6375 and S.max() <= 65535 and S.max() <= paths * (6375 + p2), (C.max(), S.max())
    return C, S


# ---- the same, all diagonals at a time ----------------------------------------------------------------------------------------------
def diagonal_indices(rows, cols):
    """(ys, xs, valid) [rows + cols - 1][min(rows, cols)]: row k holds the pixels of the diagonal x - y = k - (rows - 1), top to bottom,
    padded behind its end."""
    n, longest = rows + cols - 1, min(rows, cols)
    ys, xs, valid = np.zeros((n, longest), np.int64), np.zeros((n, longest), np.int64), np.zeros((n, longest), bool)
    for k in range(n):
        off = k - (rows - 1)
        y = np.arange(max(0, -off), min(rows, cols - off))
        ys[k, :len(y)], xs[k, :len(y)], valid[k, :len(y)] = y, y + off, True
    assert valid.sum() == rows * cols
    return ys, xs, valid


def scan_lines(A, p1, p2):
    """A [lines][length][D]: the path along every line from its first element; what lies behind a line's end is padding, which a
    forward scan never carries back."""
    out = np.empty_like(A)
    out[:, 0] = A[:, 0]
    absent = np.full((A.shape[0], 1), 1 << 28, A.dtype)
    for i in range(1, A.shape[1]):
        prev = out[:, i - 1]
        m = prev.min(axis=-1, keepdims=True)
        below = np.concatenate([absent, prev[:, :-1]], axis=-1) + p1
        above = np.concatenate([prev[:, 1:], absent], axis=-1) + p1
        out[:, i] = A[:, i] + np.minimum(np.minimum(prev, m + p2), np.minimum(below, above)) - m
    return out


def vectorised_diagonals(C, p1, p2):
    """The sum of the four diagonal L_r, [rows][cols][D] int32."""
    rows, cols, D = C.shape
    ys, xs, valid = diagonal_indices(rows, cols)
    length = valid.sum(axis=1)
    # the same diagonals bottom to top: each row of indices reversed within its valid part
    pos = np.where(valid, length[:, None] - 1 - np.arange(valid.shape[1])[None, :], 0)
    ys_up, xs_up = np.take_along_axis(ys, pos, 1), np.take_along_axis(xs, pos, 1)
    total = np.zeros_like(C)
    for mirrored in (False, True):                           # the anti-diagonals: the diagonals of the frame mirrored left-right
        V = C[:, ::-1] if mirrored else C
        acc = np.zeros_like(C)
        for yy, xx in ((ys, xs), (ys_up, xs_up)):
            L = scan_lines(V[yy, xx], p1, p2)
            acc[yy[valid], xx[valid]] += L[valid]            # (every pixel is on one diagonal: no index twice)
        total += acc[:, ::-1] if mirrored else acc
    return total


def vectorised_volumes(left, right, D, p1, p2, paths=8):
    C, S = R.vectorised_volumes(left, right, D, p1, p2)
    if paths == 8:
        S = S + vectorised_diagonals(C, p1, p2)
    assert C.max() <= 6375 and S.max() <= 65535 and S.max() <= paths * (6375 + p2), (C.max(), S.max())
    return C, S


def _run(volumes, select, left, right, paths, kw):
    p = params(paths, **kw)
    _, S = volumes(left, right, p["num_disparities"], p["p1"], p["p2"], paths)
    d16 = select(S, p["uniqueness"], p["disp12_max_diff"])
    return d16, R.depth_of(d16, p["baseline"], p["focal"], p["max_depth"])


def literal(left, right, paths=8, **kw):
    return _run(literal_volumes, R.literal_select, left, right, paths, kw)


def vectorised(left, right, paths=8, **kw):
    return _run(vectorised_volumes, R.vectorised_select, left, right, paths, kw)


def flat_scene(seed):
    """The scene of the usefulness condition: 40 x 120 noise at true disparity 6 with a flat grey patch in the middle, where only the
    paths carry the answer in from the textured surroundings; independent noise of +-16 on both images."""
    rng = np.random.default_rng(seed)
    wide = rng.integers(0, 256, (40, 126), dtype=np.uint8)
    wide[10:30, 40:80] = 128
    left = np.clip(wide[:, :120].astype(np.int64) + rng.integers(-16, 17, (40, 120)), 0, 255).astype(np.uint8)
    right = np.clip(wide[:, 6:].astype(np.int64) + rng.integers(-16, 17, (40, 120)), 0, 255).astype(np.uint8)
    return left, right
