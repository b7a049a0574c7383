"""The bilateral finish (include/dcmt.h: dcmt_bilateral5_dev, DCMT_BLUR_BILATERAL_CLONE) restated in numpy,
whole planes at a time.  The statement follows the documented definition of cv::bilateralFilter for CV_32FC1 with d = 5 and
BORDER_DEFAULT; OpenCV is never executed and its interpolated exp table is not restated.

  taps     the 13 offsets (dy, dx) with dy*dy + dx*dx <= 4, row-major; BORDER_REFLECT_101 on both axes
  weights  ws(dy, dx) = (float)exp(-(dy*dy + dx*dx) / (2 sigma_space^2)) evaluated in double;
           wc = exp(gc * d * d), d = v(tap) - v(centre), gc = -0.5f / sigma_color^2
  output   y = c + (sum ws wc d) / (sum ws wc), the sums in tap order; the centre tap adds d = 0, w = 1

restatement_f32: every operation in f32, rounded once, in that order (numpy's f32 exp stands for the device's).
restatement_f64: the same expression in f64 on the f32 inputs, with the f32 ws and gc -- the yardstick of the device tests.
naive_f32: sum(w v) / sum(w) in f32, the form the statement does NOT use (shown to be an order of magnitude worse)."""
import numpy as np

f32 = np.float32
SIGMA_COLOR, SIGMA_SPACE = 1.5, 2.0          # the cascade's literals (LO/img_completion.cpp:174)
TAPS = [(dy, dx) for dy in range(-2, 3) for dx in range(-2, 3) if dy * dy + dx * dx <= 4]
assert len(TAPS) == 13 and TAPS[6] == (0, 0)


def reflect101(p, n):
    """BORDER_REFLECT_101 of index array p into [0, n); 0 for n == 1, repeated reflection for n == 2."""
    p = np.array(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * n - 2 - p, p)
    return p


def constants(sigma_color=SIGMA_COLOR, sigma_space=SIGMA_SPACE):
    """(gc, {d2: ws}): gc in f32 arithmetic, ws from f64, rounded to f32."""
    sc = f32(sigma_color)
    gc = f32(-0.5) / (sc * sc)
    gs = -0.5 / (float(f32(sigma_space)) * float(f32(sigma_space)))
    return gc, {d2: f32(np.exp(d2 * gs)) for d2 in (0, 1, 2, 4)}


def shifted(x, dy, dx):
    rows, cols = x.shape
    return x[reflect101(np.arange(rows) + dy, rows)][:, reflect101(np.arange(cols) + dx, cols)]


def restatement_f32(x, sigma_color=SIGMA_COLOR, sigma_space=SIGMA_SPACE):
    x = np.ascontiguousarray(x, dtype=f32)
    gc, ws = constants(sigma_color, sigma_space)
    num, den = np.zeros_like(x), np.zeros_like(x)
    with np.errstate(under="ignore"):
        for dy, dx in TAPS:
            d = shifted(x, dy, dx) - x
            w = ws[dy * dy + dx * dx] * np.exp(gc * (d * d))
            assert d.dtype == f32 and w.dtype == f32
            num = num + w * d
            den = den + w
    return x + num / den


def restatement_f64(x, sigma_color=SIGMA_COLOR, sigma_space=SIGMA_SPACE):
    x = np.ascontiguousarray(x, dtype=f32).astype(np.float64)
    gc, ws = constants(sigma_color, sigma_space)
    gc = float(gc)
    num, den = np.zeros_like(x), np.zeros_like(x)
    for dy, dx in TAPS:
        d = shifted(x, dy, dx) - x
        w = float(ws[dy * dy + dx * dx]) * np.exp(gc * (d * d))
        num = num + w * d
        den = den + w
    return x + num / den


def naive_f32(x, sigma_color=SIGMA_COLOR, sigma_space=SIGMA_SPACE):
    x = np.ascontiguousarray(x, dtype=f32)
    gc, ws = constants(sigma_color, sigma_space)
    num, den = np.zeros_like(x), np.zeros_like(x)
    with np.errstate(under="ignore"):
        for dy, dx in TAPS:
            v = shifted(x, dy, dx)
            d = v - x
            w = ws[dy * dy + dx * dx] * np.exp(gc * (d * d))
            num = num + w * v
            den = den + w
    return num / den


def invert(x, max_depth=100.0, thr=0.1):
    """The cascade's final invert (LO :191-202, the project's threshold rule) in f32."""
    x = np.ascontiguousarray(x, dtype=f32)
    return np.where(x >= f32(thr), f32(max_depth) - x, x).astype(f32)
