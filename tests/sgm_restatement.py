"""Two independent numpy statements of the stereo matcher include/dcmt.h defines (dcmt_sgm_dev), and the inputs its tests share.

literal     per pixel and per path, plain Python loops over lists of ints, every clamp and every absent neighbour spelled out: meant
            for tiny frames.
vectorised  whole planes at a time: the block cost as 25 shifted slices of an edge-padded AD volume, a path as one scan along an
            axis, the right disparity as one gather.

Both come in two steps, because the volumes depend on (D, p1, p2) alone and the selection on the rest: *_volumes -> (C, S)
[rows][cols][D] (int64 from the literal form, int32 from the vectorised one), *_select -> disp16 int16 [rows][cols].  literal() /
vectorised() chain them and return (disp16, depth).  Both assert S.max() <= 65535: the device keeps S in uint16.  Nothing here is fitted to the library: tests/test_sgm.py holds the two against each
other without a GPU."""
import numpy as np

f32 = np.float32
DEFAULTS = dict(num_disparities=64, p1=200, p2=800, uniqueness=10, disp12_max_diff=1, baseline=0.54, focal=9.597910e+02, max_depth=100.0)
INVALID = -16
S_BOUND = 4 * (25 * 255 + 10000)            # 65500


def params(**kw):
    assert set(kw) <= set(DEFAULTS), kw
    p = dict(DEFAULTS)
    p.update(kw)
    D = p["num_disparities"]
    assert D % 16 == 0 and 16 <= D <= 128 and 0 <= p["p1"] <= p["p2"] <= 10000 and 0 <= p["uniqueness"] <= 100
    return p


# ---- the statement, pixel by pixel ---------------------------------------------------------------------------------------------------
def literal_volumes(left, right, D, p1, p2):
    rows, cols = left.shape
    L, R = left.astype(int).tolist(), right.astype(int).tolist()
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
                        total += abs(L[yy][xx] - R[yy][max(xx - d, 0)])
                C[y][x][d] = total
    S = [[[0] * D for _ in range(cols)] for _ in range(rows)]
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        if dx:
            starts = [(y, 0 if dx > 0 else cols - 1) for y in range(rows)]
        else:
            starts = [(0 if dy > 0 else rows - 1, x) for x in range(cols)]
        for y, x in starts:
            prev = None
            while 0 <= y < rows and 0 <= x < cols:
                c = C[y][x]
                if prev is None:
                    cur = list(c)
                else:
                    m = min(prev)
                    cur = []
                    for d in range(D):
                        candidates = [prev[d], m + p2]
                        if d - 1 >= 0:
                            candidates.append(prev[d - 1] + p1)
                        if d + 1 < D:
                            candidates.append(prev[d + 1] + p1)
                        cur.append(c[d] + min(candidates) - m)
                for d in range(D):
                    assert c[d] <= cur[d] <= c[d] + p2
                    S[y][x][d] += cur[d]
                prev = cur
                y, x = y + dy, x + dx
    C, S = np.array(C, dtype=np.int64), np.array(S, dtype=np.int64)
    assert C.max() <= 6375 and S.max() <= 65535 and S.max() <= S_BOUND, (C.max(), S.max())
    return C, S


def literal_select(S, uniqueness, disp12_max_diff):
    rows, cols, D = S.shape
    S = S.tolist()
    out = np.empty((rows, cols), np.int16)
    for y in range(rows):
        for x in range(cols):
            s = S[y][x]
            best = min(s)
            d = s.index(best)                                  # the lowest d of the least S
            ok = True
            for k in range(D):
                if abs(k - d) > 1 and s[k] * (100 - uniqueness) < best * 100:
                    ok = False
            if x - d < 0:
                ok = False
            if ok and disp12_max_diff >= 0:
                xp, right_best, right_d = x - d, None, None
                for k in range(D):
                    if xp + k < cols and (right_best is None or S[y][xp + k][k] < right_best):
                        right_best, right_d = S[y][xp + k][k], k
                if abs(right_d - d) > disp12_max_diff:
                    ok = False
            if not ok:
                out[y, x] = INVALID
                continue
            frac = 0
            if 0 < d < D - 1:
                a, b = s[d - 1], s[d + 1]
                den = max(a + b - 2 * best, 1)
                frac = ((a - b) * 16 + den) // (2 * den)       # Python's //: the floor
                assert abs(a - b) <= den and frac == ((a - b + den) * 16 + den) // (2 * den) - 8 and -8 <= frac <= 8
            out[y, x] = 16 * d + frac
    return out


# ---- the same, planes at a time -----------------------------------------------------------------------------------------------------
def vectorised_volumes(left, right, D, p1, p2):
    rows, cols = left.shape
    L, R = left.astype(np.int32), right.astype(np.int32)             # int32 throughout: S * 100 < 2^23, an absent entry is 2^28
    xr = np.maximum(np.arange(cols)[:, None] - np.arange(D)[None, :], 0)            # [cols][D]: the right column of (x, d)
    ad = np.abs(L[:, :, None] - R[:, xr])                                           # [rows][cols][D]
    pad = np.pad(ad, ((2, 2), (2, 2), (0, 0)), mode="edge")
    C = sum(pad[i:i + rows, j:j + cols] for i in range(5) for j in range(5))

    def scan(A):                                                                     # the path along axis 0, first index first
        out = np.empty_like(A)
        out[0] = A[0]
        absent = np.full(A.shape[1:-1] + (1,), 1 << 28, np.int32)
        for i in range(1, A.shape[0]):
            prev = out[i - 1]
            m = prev.min(axis=-1, keepdims=True)
            below = np.concatenate([absent, prev[..., :-1]], axis=-1) + p1
            above = np.concatenate([prev[..., 1:], absent], axis=-1) + p1
            out[i] = A[i] + np.minimum(np.minimum(prev, m + p2), np.minimum(below, above)) - m
        return out

    T = C.transpose(1, 0, 2)
    S = scan(C) + scan(C[::-1])[::-1] + scan(T).transpose(1, 0, 2) + scan(T[::-1])[::-1].transpose(1, 0, 2)
    assert C.max() <= 6375 and S.max() <= 65535 and S.max() <= S_BOUND, (C.max(), S.max())
    return C, S


def vectorised_select(S, uniqueness, disp12_max_diff):
    rows, cols, D = S.shape
    k = np.arange(D)
    d = S.argmin(axis=-1)                                                            # the first of equal minima
    best = np.take_along_axis(S, d[..., None], -1)[..., 0]
    far = np.abs(k[None, None, :] - d[..., None]) > 1
    ok = ~(far & (S * (100 - uniqueness) < best[..., None] * 100)).any(axis=-1)
    x = np.arange(cols)[None, :]
    ok &= x - d >= 0
    if disp12_max_diff >= 0:
        xs = np.arange(cols)[:, None] + k[None, :]                                   # [x'][k]: the left column of (x', k)
        along = np.where((xs < cols)[None], S[:, np.minimum(xs, cols - 1), k[None, :]], 1 << 28)
        right_d = along.argmin(axis=-1)                                              # [rows][x']
        at = np.clip(x - d, 0, cols - 1)
        ok &= np.abs(np.take_along_axis(right_d, at, 1) - d) <= disp12_max_diff
    a = np.take_along_axis(S, np.clip(d - 1, 0, D - 1)[..., None], -1)[..., 0]
    b = np.take_along_axis(S, np.clip(d + 1, 0, D - 1)[..., None], -1)[..., 0]
    den = np.maximum(a + b - 2 * best, 1)
    frac = np.where((d == 0) | (d == D - 1), 0, np.floor_divide((a - b) * 16 + den, 2 * den))
    return np.where(ok, 16 * d + frac, INVALID).astype(np.int16)


def depth_of(disp16, baseline=DEFAULTS["baseline"], focal=DEFAULTS["focal"], max_depth=DEFAULTS["max_depth"]):
    """Step 9's depth plane: one rounded product, one rounded quotient, the clamp; 0 where disp16 <= 0."""
    bf = f32(baseline) * f32(focal)
    assert bf.dtype == f32
    disparity = np.where(disp16 > 0, disp16, 16).astype(f32) / f32(16.0)
    q = (bf / disparity).astype(f32)
    return np.where(disp16 > 0, np.minimum(q, f32(max_depth)), f32(0)).astype(f32)


def _run(volumes, select, left, right, kw):
    p = params(**kw)
    _, S = volumes(left, right, p["num_disparities"], p["p1"], p["p2"])
    d16 = select(S, p["uniqueness"], p["disp12_max_diff"])
    return d16, depth_of(d16, p["baseline"], p["focal"], p["max_depth"])


def literal(left, right, **kw):
    return _run(literal_volumes, literal_select, left, right, kw)


def vectorised(left, right, **kw):
    return _run(vectorised_volumes, vectorised_select, left, right, kw)


def batch(fn, lefts, rights, **kw):
    outs = [fn(l, r, **kw) for l, r in zip(lefts, rights)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def random_pair(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (rows, cols), dtype=np.uint8), rng.integers(0, 256, (rows, cols), dtype=np.uint8)


def shifted_pair(rows, cols, seed, shift=3, half=False):
    """Noise, the right image the left one moved `shift` columns: a pair with an answer, so that most pixels are valid.  half: the
    right image is the floor-mean of the left one moved `shift` and `shift + 1` columns -- the answer lies half a pixel between the
    two, so the sub-pixel fraction takes many values."""
    rng = np.random.default_rng(seed)
    wide = rng.integers(0, 256, (rows, cols + shift + (1 if half else 0)), dtype=np.uint8)
    left = np.ascontiguousarray(wide[:, :cols])
    if not half:
        return left, np.ascontiguousarray(wide[:, shift:])
    both = wide[:, shift:shift + cols].astype(np.uint16) + wide[:, shift + 1:shift + 1 + cols]
    return left, (both // 2).astype(np.uint8)


def stripes_pair(rows, cols, right_value=0):
    """Vertical stripes 0 / 255 of period 2 against a constant image."""
    left = np.tile(np.where(np.arange(cols) % 2 == 0, 0, 255).astype(np.uint8), (rows, 1))
    return left, np.full((rows, cols), right_value, np.uint8)


def comb_pair(rows, cols, D):
    """All 255 against a comb: 255 in every D-th column, 0 elsewhere.  For every x exactly one d in [0, D) meets a tooth, so one
    narrow band of disparities is cheap and every other one costs the full 25 * 255 on every pixel of every path: with a large p2 the
    paths saturate at C + p2 and S comes close to 4 * (6375 + p2) -- what separates a uint16 volume from an int16 one."""
    right = np.where(np.arange(cols) % D == D - 1, 255, 0).astype(np.uint8)
    return np.full((rows, cols), 255, np.uint8), np.tile(right, (rows, 1))


def box_scene(rows, cols, D, seed):
    """A scene with a known answer: uniform noise, a background at disparity 5 and a centred box at min(12, D - 3); the right image
    is the left one forward-warped, far first, over noise.  Returns (left, right, truth [rows][cols] in pixels)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    left = np.ascontiguousarray(rng.integers(0, 256, (rows, cols + 2 * D)).astype(np.uint8)[:, D:D + cols])
    right = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    truth = np.full((rows, cols), 5, np.int64)
    truth[rows // 4: 3 * rows // 4, cols // 3: 2 * cols // 3] = min(12, D - 3)
    for disparity in sorted(set(truth.ravel().tolist())):           # far (small disparity) first, near over it
        ys, xs = np.nonzero(truth == disparity)
        keep = xs - disparity >= 0
        right[ys[keep], xs[keep] - disparity] = left[ys[keep], xs[keep]]
    return left, right, truth


def staircase_disparities(D):
    """The disparities at which the kernels change what they do, those that exist for D: both ends of the range, and the two sides
    of the step from a lane's first disparity register to its second (d = 63 | 64)."""
    return sorted({d for d in (0, 1, 62, 63, 64, 65, D - 2, D - 1) if 0 <= d < D})


def staircase_scene(rows, cols, D, seed, disparities=None):
    """A scene with known answers across the disparity range: uniform noise in vertical bands of rising true disparity (by default
    staircase_disparities(D)).  Band k of n starts at column k w + d_k, w = (cols - d_max) / n: every pixel of it has x >= d, and of
    its w + d_(k+1) - d_k columns the next, nearer band hides all but w in the right image.  The right image is the left one
    forward-warped, far first, over noise.  Returns (left, right, truth [rows][cols] in pixels)."""
    ds = sorted(set(staircase_disparities(D) if disparities is None else [int(d) for d in disparities]))
    assert ds and 0 <= ds[0] and ds[-1] < D
    rng = np.random.Generator(np.random.PCG64(seed))
    left = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    right = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    truth = np.empty((rows, cols), np.int64)
    w = max((cols - ds[-1]) // len(ds), 1)
    truth[:] = ds[0]
    for k, d in enumerate(ds[1:], 1):                               # (a band that starts beyond the frame does not exist in it)
        truth[:, min(k * w + d, cols):] = d
    for disparity in sorted(set(truth.ravel().tolist())):           # far (small disparity) first, near over it
        ys, xs = np.nonzero(truth == disparity)
        keep = xs - disparity >= 0
        right[ys[keep], xs[keep] - disparity] = left[ys[keep], xs[keep]]
    return left, right, truth


# ---- pairs whose answer is a chosen disparity --------------------------------------------------------------------------------------------
# per D: the ends of the range and, at two disparities a lane, both sides of the step between a lane's two registers
TARGET_SHIFTS = {16: (1, 14, 15), 48: (31, 46, 47), 128: (1, 62, 63, 64, 65, 126, 127)}
TARGET_ROWS, TARGET_MARGIN = 8, 72              # frames of 8 x (D + 72): a pixel with x < d is invalid by definition


def target_pair(D, shift, half):
    return shifted_pair(TARGET_ROWS, D + TARGET_MARGIN, 1000 + 10 * D + shift + (500 if half else 0), shift, half)


def target_pairs(D):
    """[(shift, half)] in the order every test batches them."""
    return [(shift, half) for shift in TARGET_SHIFTS[D] for half in (False, True)]


def assert_targets_found(D, disp16_of):
    """The conditions on target_pair, on the restatement's results alone (disp16_of: {(shift, half): disp16 at the default
    parameters}): the exact pair has its shift as the integer disparity of at least 500 valid pixels, the half pair shift or
    shift + 1 on at least 200, and the half pairs of one D show at least 12 of the 16 sub-pixel fractions."""
    fractions = set()
    for (shift, half), d16 in disp16_of.items():
        valid, whole = d16 >= 0, d16 >> 4
        if half:
            n = int((valid & ((whole == shift) | (whole == shift + 1))).sum())
            fractions |= set((d16[valid] & 15).tolist())
        else:
            n = int((valid & (whole == shift)).sum())
        assert n >= (200 if half else 500), f"D {D} shift {shift} half {half}: {n} pixels found"
    assert len(fractions) >= 12, (D, sorted(fractions))


STAIR_ROWS, STAIR_BAND = 8, 16


def staircase_cols(D):
    """The frame width at which every band of the default staircase shows STAIR_BAND columns in the right image."""
    return D - 1 + STAIR_BAND * len(staircase_disparities(D))


def assert_staircase_found(D, disp16, truth):
    """Every band of the default staircase at STAIR_ROWS x staircase_cols(D): of the 128 pixels the right image shows of it, at
    least 50 are valid with the band's disparity as their integer part."""
    for d in staircase_disparities(D):
        n = int(((disp16 >= 0) & ((disp16 >> 4) == d) & (truth == d)).sum())
        assert n >= 50, f"D {D}: the band at {d} is found on {n} pixels"
