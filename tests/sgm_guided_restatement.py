"""Two independent statements of the guided stereo matcher's volumes (include/dcmt.h, steps 2b and 3; dcmt_sgm_guided_dev), built on
tests/sgm_restatement.py and tests/sgm_paths_restatement.py: the block cost C, the selection (*_select) and the depth (depth_of) are
theirs.

literal     the hint rule spelled out on the bits of every guide value (sign, exponent, mantissa), the quotient and the sum rounded
            to f32 one at a time, the penalty and every path on Python ints, pixel by pixel.
vectorised  the hints of a whole plane with numpy's f32 arithmetic, the penalty as one broadcast, the axis paths as scans over all
            lines of a direction at once, the diagonals as sgm_paths_restatement extracts them.

Both return (C', S): the cost volume with the penalty in it, as the workspace holds it.  Both assert S <= 65535 and
S <= paths * (6375 + p2 + guide_cap).  guide=None, guide_weight=0 or guide_cap=0 is the unguided matcher."""
import struct

import numpy as np

import sgm_paths_restatement as P
import sgm_restatement as R

f32 = np.float32
GUIDE_WEIGHT, GUIDE_CAP = 100, 1000
MAX_GUIDE_WEIGHT = 10000
MAX_P2 = {4: 10000, 8: 1800}                    # with a guide: the limit on p2 + guide_cap


def params(paths=4, guide_weight=GUIDE_WEIGHT, guide_cap=GUIDE_CAP, guided=True, **kw):
    p = P.params(paths, **kw)
    if guided:
        assert 0 <= guide_weight <= MAX_GUIDE_WEIGHT and guide_cap >= 0 and p["p2"] + guide_cap <= MAX_P2[paths], (paths, p["p2"], guide_weight, guide_cap)
        assert np.isfinite(p["baseline"]) and p["baseline"] > 0 and np.isfinite(p["focal"]) and p["focal"] > 0
    return p


def bf_of(baseline=R.DEFAULTS["baseline"], focal=R.DEFAULTS["focal"]):
    """baseline * focal, one rounded f32 product (depth_of's)."""
    with np.errstate(over="ignore"):
        return f32(f32(baseline) * f32(focal))


BF = bf_of()


# ---- step 2b, one value at a time --------------------------------------------------------------------------------------------------------
def _round_f32(v):
    """A Python float rounded to f32 (to +-inf beyond its range), as a Python float.  A quotient or a sum of two f32 values computed in
    f64 and rounded again is the correctly rounded f32 result: f64 carries more than twice f32's digits."""
    with np.errstate(over="ignore"):
        return float(f32(v))


def literal_hint(bits, bf, D):
    """The hint of a guide value given as the 32 bits of its f32, or -1."""
    sign, exponent, mantissa = bits >> 31, (bits >> 23) & 0xFF, bits & 0x7FFFFF
    if sign == 1:                                   # negatives, -0.0, -inf, NaNs with the sign set
        return -1
    if exponent == 0xFF:                            # +inf, NaN
        return -1
    if exponent == 0 and mantissa == 0:             # +0.0
        return -1
    z = struct.unpack("<f", struct.pack("<I", bits))[0]          # finite and > 0, a denormal included
    bf = float(bf)
    q = float("inf") if bf == float("inf") else _round_f32(bf / z)
    t = _round_f32(q + 0.5)
    if not t < float(D):
        return -1
    h = int(t)
    assert 0 <= h <= D - 1
    return h


def literal_hints(guide, bf, D):
    bits = np.ascontiguousarray(guide, dtype=f32).view(np.uint32)
    return [[literal_hint(int(b), bf, D) for b in row] for row in bits]


def literal_volumes(left, right, guide, D, p1, p2, paths=4, guide_weight=GUIDE_WEIGHT, guide_cap=GUIDE_CAP, bf=BF, C=None):
    """(C', S) int64 [rows][cols][D].  C: the unguided block cost if the caller has it already."""
    if C is None:
        C = R.literal_volumes(left, right, D, 0, 0)[0]
    rows, cols = left.shape
    cost = C.tolist()
    if guide is not None:
        hints = literal_hints(guide, bf, D)
        for y in range(rows):
            for x in range(cols):
                h = hints[y][x]
                if h < 0:
                    continue
                for d in range(D):
                    penalty = guide_weight * abs(d - h)
                    cost[y][x][d] += guide_cap if penalty > guide_cap else penalty
    cap = guide_cap if guide is not None else 0
    S = [[[0] * D for _ in range(cols)] for _ in range(rows)]
    directions = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (-1, -1), (1, -1), (-1, 1)] if paths == 8 else [])
    for dy, dx in directions:
        for y0 in range(rows):
            for x0 in range(cols):
                if 0 <= y0 - dy < rows and 0 <= x0 - dx < cols:
                    continue                                    # not the first pixel of a path
                y, x, prev = y0, x0, None
                while 0 <= y < rows and 0 <= x < cols:
                    c = cost[y][x]
                    if prev is None:
                        cur = list(c)
                    else:
                        m = min(prev)
                        cur = []
                        for d in range(D):
                            best = min(prev[d], m + p2)
                            if d >= 1:
                                best = min(best, prev[d - 1] + p1)
                            if d <= D - 2:
                                best = min(best, prev[d + 1] + p1)
                            cur.append(c[d] + best - m)
                    for d in range(D):
                        assert c[d] <= cur[d] <= c[d] + p2
                        S[y][x][d] += cur[d]
                    prev = cur
                    y, x = y + dy, x + dx
    Cg, S = np.array(cost, dtype=np.int64), np.array(S, dtype=np.int64)
    assert Cg.max() <= 6375 + cap and S.max() <= 65535 and S.max() <= paths * (6375 + p2 + cap), (Cg.max(), S.max())
    return Cg, S


# ---- the same, planes at a time ----------------------------------------------------------------------------------------------------------
def vectorised_hints(guide, bf, D):
    """int64 [rows][cols], -1 where there is no hint."""
    z = np.ascontiguousarray(guide, dtype=f32)
    bits = z.view(np.uint32)
    positive_finite = (bits.view(np.int32) > 0) & (bits < np.uint32(0x7F800000))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        q = (f32(bf) / np.where(positive_finite, z, f32(1))).astype(f32)
        t = (q + f32(0.5)).astype(f32)
    has = positive_finite & (t < f32(D))
    return np.where(has, np.where(has, t, f32(0)).astype(np.int64), -1)


def vectorised_volumes(left, right, guide, D, p1, p2, paths=4, guide_weight=GUIDE_WEIGHT, guide_cap=GUIDE_CAP, bf=BF):
    C = R.vectorised_volumes(left, right, D, 0, 0)[0]
    cap = 0
    if guide is not None:
        h = vectorised_hints(guide, bf, D)
        penalty = np.minimum(guide_weight * np.abs(np.arange(D)[None, None, :] - h[..., None]), guide_cap)
        C = C + np.where((h >= 0)[..., None], penalty, 0).astype(C.dtype)
        cap = guide_cap
    T = C.transpose(1, 0, 2)
    S = (P.scan_lines(C, p1, p2) + P.scan_lines(C[:, ::-1], p1, p2)[:, ::-1]
         + P.scan_lines(T, p1, p2).transpose(1, 0, 2) + P.scan_lines(T[:, ::-1], p1, p2)[:, ::-1].transpose(1, 0, 2))
    if paths == 8:
        S = S + P.vectorised_diagonals(C, p1, p2)
    assert C.max() <= 6375 + cap and S.max() <= 65535 and S.max() <= paths * (6375 + p2 + cap), (C.max(), S.max())
    return C, S


def _run(volumes, select, left, right, guide, paths, guide_weight, guide_cap, kw):
    p = params(paths, guide_weight, guide_cap, guided=guide is not None, **kw)
    _, S = volumes(left, right, guide, p["num_disparities"], p["p1"], p["p2"], paths, guide_weight, guide_cap, bf_of(p["baseline"], p["focal"]))
    d16 = select(S, p["uniqueness"], p["disp12_max_diff"])
    return d16, R.depth_of(d16, p["baseline"], p["focal"], p["max_depth"])


def literal(left, right, guide=None, paths=4, guide_weight=GUIDE_WEIGHT, guide_cap=GUIDE_CAP, **kw):
    return _run(literal_volumes, R.literal_select, left, right, guide, paths, guide_weight, guide_cap, kw)


def vectorised(left, right, guide=None, paths=4, guide_weight=GUIDE_WEIGHT, guide_cap=GUIDE_CAP, **kw):
    return _run(vectorised_volumes, R.vectorised_select, left, right, guide, paths, guide_weight, guide_cap, kw)


# ---- guides ------------------------------------------------------------------------------------------------------------------------------
def depth_for(disparity, bf=BF):
    """An f32 depth whose hint is `disparity` (> 0): bf / disparity lands within rounding of it, far from the next half."""
    return f32(f32(bf) / f32(disparity))


FAR = f32(1e30)                                     # q underflows towards 0: the hint 0


def boundary_depths(D, bf=BF):
    """(inside, outside): two adjacent f32 depths, the first with t = q + 0.5f just below D (hint D - 1), the second, one ulp nearer,
    with t >= D (no hint)."""
    z = f32(f32(bf) / f32(D - 0.5))
    for _ in range(64):                             # move off the boundary to the inside, then walk down to it
        z = np.nextafter(z, f32(np.inf))
    for _ in range(256):
        nearer = np.nextafter(z, f32(0))
        if vectorised_hints(np.array([[nearer]], f32), bf, D)[0, 0] < 0:
            assert vectorised_hints(np.array([[z]], f32), bf, D)[0, 0] == D - 1
            return f32(z), f32(nearer)
        z = nearer
    raise AssertionError("no boundary found")


HOSTILE_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000,
                0x00000001, 0x007FFFFF, 0x80000001, 0x00800000, 0x7F7FFFFF)
# NaN, -NaN, a signalling NaN, +inf, -inf, -1.0, -0.0, +0.0, the least and the greatest denormal, a negative denormal, the least
# normal number, the greatest finite number


def hostile_plane(rows, cols, D, bf=BF):
    """Every hostile pattern, 1e30 and 1e-30, the two depths of boundary_depths and a few ordinary hints, repeated over the plane."""
    inside, outside = boundary_depths(D, bf)
    values = [np.array([b], np.uint32).view(f32)[0] for b in HOSTILE_BITS]
    values += [f32(1e30), f32(1e-30), inside, outside, depth_for(1, bf), depth_for(D - 1, bf), f32(-5.0)]
    flat = np.array([values[i % len(values)] for i in range(rows * cols)], dtype=f32)
    return flat.reshape(rows, cols)


def guide_kinds(rows, cols, D, bf=BF, shift=3, seed=0):
    """{name: f32 [rows][cols]}: the guides every test of the guided matcher runs, in one order."""
    rng = np.random.default_rng(seed + 31 * rows + cols)
    kinds = {"zero": np.zeros((rows, cols), f32)}
    sparse = np.zeros((rows, cols), f32)
    sparse[min(2, rows - 1)::4, min(3, cols - 1)::8] = depth_for(shift, bf)       # right for shifted_pair
    kinds["sparse"] = sparse
    with np.errstate(divide="ignore"):
        kinds["dense"] = (f32(bf) / rng.uniform(0.0, D + 4.0, (rows, cols)).astype(f32)).astype(f32)      # every pixel, some beyond the range
    ends = np.where((np.arange(rows)[:, None] + np.arange(cols)[None, :]) % 2 == 0, FAR, depth_for(D - 1, bf)).astype(f32)
    kinds["ends"] = ends                                                            # hints exactly 0 and D - 1
    kinds["middle"] = np.where((np.arange(rows)[:, None] + np.arange(cols)[None, :]) % 2 == 0, depth_for(63, bf), depth_for(64, bf)).astype(f32)
    border = np.zeros((rows, cols), f32)
    border[0, :] = border[-1, :] = depth_for(shift, bf)
    border[:, 0] = border[:, -1] = depth_for(min(5, D - 1), bf)
    kinds["border"] = border
    kinds["hostile"] = hostile_plane(rows, cols, D, bf)
    return kinds


def flat_grid_guide(disparity, bf=BF):
    """The guide of the usefulness experiments on sgm_paths_restatement.flat_scene: a return on every 4th row and 8th column."""
    guide = np.zeros((40, 120), f32)
    guide[2::4, 3::8] = f32(bf) / f32(disparity)
    return guide
