"""The cascade without its extrapolation (DCMT_FLAG_NO_EXTRAPOLATE, include/dcmt.h), restated twice from what the oracle already
exports.  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

With X5 the plane after stage 5 (the 7x7 fill), thr = valid_thresh (0.1f by default) and "valid" x >= thr:
    X9  = medianBlur5(X5)
    X10 = gaussian: X9 >= thr ? GaussianBlur5(X9) : X9;   none: X9
    X11 = X10 >= thr ? max_depth - X10 : X10
(a) restatement_oracle: X5 from oracle/dcmt_oracle.c (stop_after = 5), then its median5 and gaussian5, select and invert here.
(b) restatement_numpy: everything from oracle/np_restatement.py's whole-array functions.
Both take labels (the label-masked stage of interpolate_with_superpixels, which forces the Gaussian), a k0 preset, and the two
numeric parameters max_depth and valid_thresh (defaults: the reference's 100 and 0.1f)."""
import numpy as np

from oracle import np_restatement as N
from oracle import oracle as O

f32 = np.float32
THR = f32(0.1)
MAX_DEPTH = f32(100.0)


def _finish(x5, stop_after, blur, median5, gaussian5, max_depth=MAX_DEPTH, valid_thresh=THR):
    assert stop_after in (9, 10, 11), "stages 6..8 do not exist without the extrapolation"
    thr = f32(valid_thresh)
    x = median5(x5)
    if stop_after == 9:
        return x
    if blur == "gaussian":
        x = np.where(x >= thr, gaussian5(x), x).astype(f32)
    if stop_after == 10:
        return x
    return np.where(x >= thr, f32(max_depth) - x, x).astype(f32)


def x5_oracle(sparse, k0="as_compiled", labels=None, n_labels=0, max_depth=MAX_DEPTH, valid_thresh=THR):
    p = O.default_params(k0=k0, stop_after=5, max_depth=max_depth, valid_thresh=valid_thresh)
    if labels is None:
        return O.img_completion(sparse, p)
    return O.interpolate_with_superpixels(sparse, labels, n_labels, p)


def restatement_oracle(sparse, k0="as_compiled", blur="gaussian", stop_after=11, labels=None, n_labels=0,
                       max_depth=MAX_DEPTH, valid_thresh=THR):
    """(a)"""
    blur = "gaussian" if labels is not None else blur
    return _finish(x5_oracle(sparse, k0, labels, n_labels, max_depth, valid_thresh), stop_after, blur, O.median5, O.gaussian5,
                   max_depth, valid_thresh)


def restatement_numpy(sparse, k0="as_compiled", blur="gaussian", stop_after=11, labels=None, n_labels=0,
                      max_depth=MAX_DEPTH, valid_thresh=THR):
    """(b)"""
    k = N.K0_DIAMOND if k0 == "diamond" else N.K0_AS_COMPILED if k0 == "as_compiled" else np.asarray(k0, np.uint8).reshape(5, 5)
    if labels is None:
        x5 = N.img_completion(sparse, k0=k, stop_after=5, max_depth=max_depth, valid_thresh=valid_thresh)
    else:
        x5 = N.interpolate_with_superpixels(sparse, labels, n_labels, k0=k, stop_after=5, max_depth=max_depth, valid_thresh=valid_thresh)
        blur = "gaussian"
    # N.fill, N.dilate, N.erode and N.invert are what stop_after = 5 runs; the finish below uses N's median, Gaussian and invert
    x = N.median5(x5)
    if stop_after == 9:
        return x
    if blur == "gaussian":
        x = np.where(N._valid(x, valid_thresh), N.gaussian5(x), x).astype(f32)
    if stop_after == 10:
        return x
    return N.invert(x, max_depth, valid_thresh)


# ---- the adversarial planes of the issue -------------------------------------------------------------------------------------
def random_plane(rows, cols, seed, density=0.004):
    """Sparse enough that H3..H5 leave holes on all but the smallest shapes: one measurement per 250 pixels, three at least."""
    g = np.random.Generator(np.random.PCG64(seed))
    n = max(3, int(rows * cols * density))
    x = np.zeros(rows * cols, f32)
    x[g.choice(rows * cols, n, replace=False)] = g.uniform(1.0, 90.0, n).astype(f32)
    return x.reshape(rows, cols)


def adversarial_planes(rows=33, cols=70, max_depth=MAX_DEPTH, valid_thresh=THR):
    """name -> plane; "threshold" and "far" are built around the given (max_depth, valid_thresh)"""
    THR, MAX_DEPTH = f32(valid_thresh), f32(max_depth)
    g = np.random.Generator(np.random.PCG64(77))
    out = {}
    out["all zero"] = np.zeros((rows, cols), f32)
    out["fully valid"] = g.uniform(2.0, 80.0, (rows, cols)).astype(f32)
    c = np.zeros((rows, cols), f32)
    c[0, 0], c[0, -1], c[-1, 0], c[-1, -1] = 10.0, 20.0, 30.0, 40.0
    out["corners"] = c
    e = np.zeros((rows, cols), f32)
    e[:, 0] = g.uniform(5.0, 50.0, rows).astype(f32)
    e[:, -1] = g.uniform(5.0, 50.0, rows).astype(f32)
    e[rows // 3: rows // 3 + 5, 0] = 0.0                       # holes in the edge columns themselves
    e[2 * rows // 3:, -1] = 0.0
    out["edge columns"] = e
    t = np.zeros((rows, cols), f32)
    below = np.nextafter(THR, f32(0.0))
    t[4::6, 3::7] = THR
    t[5::6, 5::7] = below
    t[2, 2:12] = [THR, below] * 5
    out["threshold"] = t
    # isolated depths in max_depth - 10 thr .. max_depth - thr / 2 (99.0 .. 99.95 m at the defaults): inverted they are thr / 2 .. 10 thr,
    # either side of thr, and blurred with the empty pixels around them some fall below it
    far = np.zeros((rows, cols), f32)
    ys, xs = np.mgrid[3:rows - 3:7, 3:cols - 3:9]
    far[ys, xs] = np.linspace(MAX_DEPTH - f32(10) * THR, MAX_DEPTH - THR / f32(2), ys.size, dtype=f32).reshape(ys.shape)
    out["far"] = far
    for v in out.values():
        v.setflags(write=False)
    return out


def uninverted_pixels(sparse, k0="as_compiled", max_depth=MAX_DEPTH, valid_thresh=THR):
    """Pixels whose median is valid but whose blurred value fell below thr: they are not inverted (X11 = X10 < thr)."""
    x9 = restatement_oracle(sparse, k0, "gaussian", 9, max_depth=max_depth, valid_thresh=valid_thresh)
    x10 = restatement_oracle(sparse, k0, "gaussian", 10, max_depth=max_depth, valid_thresh=valid_thresh)
    return (x9 >= f32(valid_thresh)) & (x10 < f32(valid_thresh))
