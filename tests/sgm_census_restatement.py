"""Two independent statements of the stereo matcher's census cost (include/dcmt.h, steps 1c and 2c; dcmt_sgm_cost_dev with
DCMT_SGM_COST_CENSUS), built on tests/sgm_restatement.py, tests/sgm_paths_restatement.py and tests/sgm_guided_restatement.py: the
paths, the guide's penalty, the selection (*_select) and the depth (depth_of) are theirs.

literal     the code of every pixel bit by bit on Python ints, every clamp spelled out, the Hamming distance as a count of differing
            bits, the block cost as 25 terms per (y, x, d); then the guide and the paths of sgm_guided_restatement.literal_volumes.
vectorised  the 24 comparisons as shifted slices of an edge-padded image, the codes as int64 words, the popcount from a table of
            bytes, the block cost as 25 shifted slices of an edge-padded H volume; then the penalty as one broadcast and the paths as
            scans over all lines of a direction.

Both return (C, S) -- C with the penalty in it where there is a guide, as the workspace holds it -- and both assert C <= 6000 (+ the
cap) and S <= 65535.  The two forms order the bits of a code differently: only the popcount of an XOR is ever used."""
import numpy as np

import sgm_guided_restatement as G
import sgm_paths_restatement as P
import sgm_restatement as R

SCALE = 10                                      # part of the definition: C = 10 * the sum of the Hamming distances
C_BOUND = SCALE * 25 * 24                       # 6000 <= 6375: every bound of the statement holds as written
WINDOW = [(dy, dx) for dy in (-2, -1, 0, 1, 2) for dx in (-2, -1, 0, 1, 2) if (dy, dx) != (0, 0)]
COSTS = ("absdiff", "census")


# ---- steps 1c and 2c, one pixel at a time -------------------------------------------------------------------------------------------------
def literal_codes(image):
    """[rows][cols] Python ints: bit k is set iff the k-th neighbour of WINDOW, clamped into the image, is strictly darker."""
    rows, cols = image.shape
    I = image.astype(int).tolist()
    clamp = lambda v, hi: 0 if v < 0 else hi if v > hi else v
    codes = [[0] * cols for _ in range(rows)]
    for y in range(rows):
        for x in range(cols):
            code = 0
            for k, (dy, dx) in enumerate(WINDOW):
                if I[clamp(y + dy, rows - 1)][clamp(x + dx, cols - 1)] < I[y][x]:
                    code |= 1 << k
            codes[y][x] = code
    return codes


def literal_cost(left, right, D):
    """C int64 [rows][cols][D] without a guide."""
    rows, cols = left.shape
    KL, KR = literal_codes(left), literal_codes(right)
    clamp = lambda v, hi: 0 if v < 0 else hi if v > hi else v
    C = [[[0] * D for _ in range(cols)] for _ in range(rows)]
    for y in range(rows):
        for x in range(cols):
            for d in range(D):
                total = 0
                for dy in (-2, -1, 0, 1, 2):
                    yy = clamp(y + dy, rows - 1)
                    for dx in (-2, -1, 0, 1, 2):
                        xx = clamp(x + dx, cols - 1)
                        total += bin(KL[yy][xx] ^ KR[yy][max(xx - d, 0)]).count("1")
                C[y][x][d] = SCALE * total
    C = np.array(C, dtype=np.int64)
    assert 0 <= C.min() and C.max() <= C_BOUND, (C.min(), C.max())
    return C


def literal_volumes(left, right, guide, D, p1, p2, paths=4, guide_weight=G.GUIDE_WEIGHT, guide_cap=G.GUIDE_CAP, bf=G.BF, C=None):
    """(C', S) int64 [rows][cols][D].  C: literal_cost(left, right, D) if the caller has it already."""
    if C is None:
        C = literal_cost(left, right, D)
    Cg, S = G.literal_volumes(left, right, guide, D, p1, p2, paths, guide_weight, guide_cap, bf, C=C)
    cap = guide_cap if guide is not None else 0
    assert Cg.max() <= C_BOUND + cap and S.max() <= 65535 and S.max() <= paths * (C_BOUND + p2 + cap), (Cg.max(), S.max())
    return Cg, S


# ---- the same, planes at a time -----------------------------------------------------------------------------------------------------------
_BYTE_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], dtype=np.int32)


def vectorised_codes(image):
    """int64 [rows][cols]; the bits in the order of the slices, which is not literal_codes' order."""
    rows, cols = image.shape
    pad = np.pad(image.astype(np.int32), 2, mode="edge")
    centre = pad[2:2 + rows, 2:2 + cols]
    code = np.zeros((rows, cols), np.int64)
    bit = 23
    for i in range(5):
        for j in range(5):
            if (i, j) == (2, 2):
                continue
            code |= (pad[i:i + rows, j:j + cols] < centre).astype(np.int64) << bit
            bit -= 1
    assert bit == -1
    return code


def popcount24(words):
    w = words.astype(np.int64)
    return _BYTE_POPCOUNT[w & 0xFF] + _BYTE_POPCOUNT[(w >> 8) & 0xFF] + _BYTE_POPCOUNT[(w >> 16) & 0xFF]


def vectorised_cost(left, right, D):
    rows, cols = left.shape
    KL, KR = vectorised_codes(left), vectorised_codes(right)
    xr = np.maximum(np.arange(cols)[:, None] - np.arange(D)[None, :], 0)            # [cols][D]: the right column of (x, d)
    H = popcount24(KL[:, :, None] ^ KR[:, xr])                                      # [rows][cols][D], 0..24
    pad = np.pad(H, ((2, 2), (2, 2), (0, 0)), mode="edge")
    C = (SCALE * sum(pad[i:i + rows, j:j + cols] for i in range(5) for j in range(5))).astype(np.int32)
    assert 0 <= C.min() and C.max() <= C_BOUND, (C.min(), C.max())
    return C


def vectorised_volumes(left, right, guide, D, p1, p2, paths=4, guide_weight=G.GUIDE_WEIGHT, guide_cap=G.GUIDE_CAP, bf=G.BF):
    C = vectorised_cost(left, right, D)
    cap = 0
    if guide is not None:
        h = G.vectorised_hints(guide, bf, D)
        penalty = np.minimum(guide_weight * np.abs(np.arange(D)[None, None, :] - h[..., None]), guide_cap)
        C = C + np.where((h >= 0)[..., None], penalty, 0).astype(C.dtype)
        cap = guide_cap
    T = C.transpose(1, 0, 2)
    S = (P.scan_lines(C, p1, p2) + P.scan_lines(C[:, ::-1], p1, p2)[:, ::-1]
         + P.scan_lines(T, p1, p2).transpose(1, 0, 2) + P.scan_lines(T[:, ::-1], p1, p2)[:, ::-1].transpose(1, 0, 2))
    if paths == 8:
        S = S + P.vectorised_diagonals(C, p1, p2)
    assert C.max() <= C_BOUND + cap and S.max() <= 65535 and S.max() <= paths * (C_BOUND + p2 + cap), (C.max(), S.max())
    return C, S


def _run(volumes, select, left, right, guide, paths, guide_weight, guide_cap, kw):
    p = G.params(paths, guide_weight, guide_cap, guided=guide is not None, **kw)
    _, S = volumes(left, right, guide, p["num_disparities"], p["p1"], p["p2"], paths, guide_weight, guide_cap, G.bf_of(p["baseline"], p["focal"]))
    d16 = select(S, p["uniqueness"], p["disp12_max_diff"])
    return d16, R.depth_of(d16, p["baseline"], p["focal"], p["max_depth"])


def literal(left, right, guide=None, paths=4, guide_weight=G.GUIDE_WEIGHT, guide_cap=G.GUIDE_CAP, **kw):
    return _run(literal_volumes, R.literal_select, left, right, guide, paths, guide_weight, guide_cap, kw)


def vectorised(left, right, guide=None, paths=4, guide_weight=G.GUIDE_WEIGHT, guide_cap=G.GUIDE_CAP, **kw):
    return _run(vectorised_volumes, R.vectorised_select, left, right, guide, paths, guide_weight, guide_cap, kw)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def constant_pair(rows, cols, value=93):
    """Every code is 0, C is 0 everywhere, and the lowest-d rule of step 4 decides."""
    return np.full((rows, cols), value, np.uint8), np.full((rows, cols), value, np.uint8)


def quantised_pair(rows, cols, seed, shift=3):
    """shifted_pair on four grey levels: most neighbours equal the centre, so a strict and a non-strict comparison differ on most
    bits."""
    left, right = R.shifted_pair(rows, cols, seed, shift=min(shift, cols - 1)) if cols >= 2 else R.random_pair(rows, cols, seed)
    return (left // 64 * 64).astype(np.uint8), (right // 64 * 64).astype(np.uint8)


# the exposures of the usefulness table: what the right camera makes of the grey value v the left one sees
EXPOSURES = {
    "as generated": lambda v: v,
    "0.6 v + 40": lambda v: np.floor(0.6 * v.astype(np.float64) + 40).astype(np.uint8),
    "v // 2": lambda v: v // 2,
    "max(v - 60, 0)": lambda v: np.maximum(v.astype(np.int32) - 60, 0).astype(np.uint8),
    "gamma 1.8": lambda v: np.floor(255 * (v.astype(np.float64) / 255) ** 1.8).astype(np.uint8),
}


def found(d16, truth):
    """The pixels that are valid with the true integer disparity."""
    return int(((d16 >= 0) & ((d16 >> 4) == truth)).sum())
