"""get_initial_error (DC_stereo_lidar/main_sl.cpp:618-712) restated twice, and the planes and images its tests share.

literal()     the reference's loops statement by statement (:636-682 and the count of :696): np.float32 for its three f32 operations
              (the product, the quotient, the difference), Python ints for everything else.
vectorised()  an independent numpy form: whole-plane arithmetic, one pass per tap, its own integer square root.

Both close the reference's two undefined conversions the way include/dcmt.h states it: a t that is NaN or outside int's range is
"not inside", and 0 < trunc(t) < cols is decided on the float before any conversion (target()).  Both return (err uint8 [rows][cols],
stats uint64 [4] = valid, matches, nonzero, sum_err).
"""
import math

import numpy as np

f32 = np.float32
BASELINE, FOCAL, WINDOW = 0.54, 9.597910e+02, 2            # :632, :634, :638
STATS = ("valid", "matches", "nonzero", "sum_err")


def target(t, cols):
    """pixel_reprojected of :649 where it passes :656, else None.  t: the f32 (float)j - disparity."""
    t = float(t)
    if math.isnan(t) or math.isinf(t) or abs(t) >= 2.0 ** 31:
        return None                                         # (int)t is undefined in the reference: not inside
    pr = math.trunc(t)                                      # toward zero, exact
    return pr if 0 < pr < cols else None


def literal(depth, left, right, baseline=BASELINE, focal=FOCAL, window=WINDOW):
    depth = np.asarray(depth, dtype=f32)
    rows, cols = depth.shape
    assert left.shape == right.shape == (rows, cols) and left.dtype == right.dtype == np.uint8
    err = np.zeros((rows, cols), np.uint8)                  # :641
    matches = row_cols = 0
    with np.errstate(all="ignore"):
        bf = f32(baseline) * f32(focal)                     # one rounded product
        for i in range(rows):
            for j in range(cols):
                d = depth[i, j]
                if not d > 0:                               # :646 (false for NaN)
                    continue
                disparity = bf / d                          # :648, one rounded quotient
                t = f32(j) - disparity                      # :649
                pr = target(t, cols)
                ssd = 0
                if pr is not None:                          # :656
                    row_cols += 1
                    for k in range(-window, window):
                        for p in range(-window, window):
                            if i + p > 0 and i + p < rows and j + k > 0 and j + k < cols and pr + k > 0 and pr + k < cols:
                                lv, rv = int(left[i + p, j + k]), int(right[i + p, pr + k])
                                ssd += (lv - rv) * (lv - rv)
                                matches += 1
                err[i, j] = min(255, math.isqrt(ssd))       # :676-678: float e = sqrt(int), clamp, cast (test_photo_error.py: the same)
    counts = sum(1 for v in err.flat if v > 0)              # :696
    return err, np.array([row_cols, matches, counts, int(err.astype(np.int64).sum())], np.uint64)


def vectorised(depth, left, right, baseline=BASELINE, focal=FOCAL, window=WINDOW):
    depth = np.asarray(depth, dtype=f32)
    rows, cols = depth.shape
    I, J = np.meshgrid(np.arange(rows, dtype=np.int64), np.arange(cols, dtype=np.int64), indexing="ij")
    with np.errstate(all="ignore"):
        positive = depth > 0
        disparity = np.divide(f32(baseline) * f32(focal), depth, dtype=f32)
        t = np.subtract(J.astype(f32), disparity, dtype=f32)
        whole = np.trunc(t.astype(np.float64))
        inside = positive & np.isfinite(t) & (whole >= 1) & (whole <= cols - 1)
    pr = np.where(inside, whole, 0).astype(np.int64)
    L, R = left.astype(np.int64), right.astype(np.int64)
    ssd = np.zeros((rows, cols), np.int64)
    matches = 0
    for p in range(-window, window):
        for k in range(-window, window):
            r, cl, cr = I + p, J + k, pr + k
            keep = inside & (r > 0) & (r < rows) & (cl > 0) & (cl < cols) & (cr > 0) & (cr < cols)
            rc = np.clip(r, 0, rows - 1)
            diff = L[rc, np.clip(cl, 0, cols - 1)] - R[rc, np.clip(cr, 0, cols - 1)]
            ssd += np.where(keep, diff * diff, 0)
            matches += int(keep.sum())
    root = np.floor(np.sqrt(ssd.astype(np.float64))).astype(np.int64)       # then made exact in integers, whatever the f64 root did
    root -= root * root > ssd
    root += (root + 1) * (root + 1) <= ssd
    err = np.minimum(root, 255).astype(np.uint8)
    return err, np.array([int(inside.sum()), matches, int((err > 0).sum()), int(err.astype(np.int64).sum())], np.uint64)


def batch(fn, depth, left, right, **kw):
    """fn over [b][rows][cols]: (err [b][rows][cols], stats [b][4])."""
    out = [fn(depth[f], left[f], right[f], **kw) for f in range(depth.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- depth planes ---------------------------------------------------------------------------------------------------------------
def random_depth(rows, cols, seed):
    """Depths in [1.5, 80] with 30 % zeros."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(1.5, 80.0, (rows, cols)).astype(f32)
    d[rng.random((rows, cols)) < 0.3] = 0
    return d


def constant_depth(rows, cols, value=12.0):
    return np.full((rows, cols), value, f32)


def depth_for_disparity(disp, bf):
    """An f32 depth d with f32(bf / d) == disp exactly, or None: the quotient's neighbours, a few ulps either way."""
    disp, bf = f32(disp), f32(bf)
    if not disp > 0:
        return None
    d0 = f32(bf / disp)
    for direction in (f32(np.inf), f32(0)):
        d = d0
        for _ in range(64):
            if d > 0 and np.isfinite(d) and f32(bf / d) == disp:
                return d
            d = np.nextafter(d, direction)
    return None


SPECIAL_VALUES = {"1e-38": f32(1e-38), "1e-30": f32(1e-30), "1e30": f32(1e30), "-1": f32(-1), "-0.0": f32(-0.0), "nan": f32(np.nan),
                  "+inf": f32(np.inf), "-inf": f32(-np.inf)}
T_TARGETS = ("t=-0.5", "t=0.5", "t=1", "t=cols-1", "t<left", "t=-inf")


def adversarial_depth(rows, cols, seed, baseline=BASELINE, focal=FOCAL):
    """A random plane with, at known pixels, depths that put t = (float)j - disparity on -0.5, 0.5, 1 and cols - 1, beyond the row's left
    end (t = -3) and on -inf, and the values of SPECIAL_VALUES.  Returns (plane, placed): placed maps a label to its (i, j); a label is
    missing where the plane has no room for it (a t target needs a column j with an f32 depth that hits it exactly).
    t = cols itself cannot be reached from a plane: with baseline * focal > 0 (anything else is refused) and depth > 0 the disparity is
    >= 0 and t <= (float)j <= cols - 1 for every column below 2^24; test_photo_error.py puts it to target() directly."""
    d = random_depth(rows, cols, seed)
    with np.errstate(all="ignore"):
        bf = f32(baseline) * f32(focal)
    placed, used, n = {}, set(), 0

    def put(label, i, j, v):
        if (i, j) in used:
            return False
        d[i, j] = v
        used.add((i, j))
        placed[label] = (i, j)
        return True

    for label, want in (("t=-0.5", -0.5), ("t=0.5", 0.5), ("t=1", 1.0), ("t<left", -3.0)):
        for j in range(cols):
            v = depth_for_disparity(j - want, bf)
            if v is not None and put(label, n % rows, j, v):
                n += 1
                break
    if put("t=cols-1", n % rows, cols - 1, f32(np.inf)):      # disparity 0: t = cols - 1, valid where cols > 1
        n += 1
    for label, v in SPECIAL_VALUES.items():
        for step in range(rows * cols):
            k = (7 * n + 3 + step) % (rows * cols)
            if put(label, k // cols, k % cols, v):
                n += 1
                break
    if "1e-38" in placed:
        placed["t=-inf"] = placed["1e-38"]                    # bf / 1e-38 overflows: the disparity is +inf, t is -inf
    return d, placed


# ---- images ---------------------------------------------------------------------------------------------------------------------
def random_pair(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (rows, cols), dtype=np.uint8), rng.integers(0, 256, (rows, cols), dtype=np.uint8)


def extremes_pair(rows, cols):
    """All 0 against all 255: every valid pixel with a kept tap clamps to 255."""
    return np.zeros((rows, cols), np.uint8), np.full((rows, cols), 255, np.uint8)


def ramp_pair(rows, cols):
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return ((3 * j + 5 * i) % 256).astype(np.uint8), ((3 * j + 7 * i + 11) % 256).astype(np.uint8)


IMAGES = {"random": lambda r, c: random_pair(r, c, 1000 + 31 * r + c), "extremes": extremes_pair, "ramp": ramp_pair}
