"""The Gaussian that ignores holes (DCMT_BLUR_GAUSSIAN_VALID, dcmt_gaussian5_valid*; include/dcmt.h has the definition), restated
twice in different styles, and the cascade finishes built on it.  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

With G5 = oracle/np_restatement.py::gaussian5, thr = valid_thresh and v(x) = x >= thr (NaN is not valid):
    num = G5(v(X) ? X : 0)       den = G5(v(X) ? 1 : 0)       GV(X) = v(X) ? num / den : X
(a) gv_arrays: whole arrays, from gaussian5 itself.
(b) gv_loop:   a literal loop over every pixel's 25 reflect-101 taps: five row passes c*k0 + (l1 + r1)*k1 + (l2 + r2)*k2, then the same
               pass down their results, every operation rounded to f32."""
import numpy as np

from oracle import np_restatement as N
import no_extrapolate_restatement as NE

f32 = np.float32
THR = f32(0.1)
MAX_DEPTH = f32(100.0)
K0, K1, K2 = f32(0.375), f32(0.25), f32(0.0625)


def valid(x, valid_thresh=THR):
    with np.errstate(invalid="ignore"):
        return np.asarray(x, f32) >= f32(valid_thresh)


def num_den(x, valid_thresh=THR):
    x = np.asarray(x, f32)
    v = valid(x, valid_thresh)
    return N.gaussian5(np.where(v, x, f32(0)).astype(f32)), N.gaussian5(v.astype(f32))


def gv_arrays(x, valid_thresh=THR):
    """(a)"""
    x = np.asarray(x, f32)
    num, den = num_den(x, valid_thresh)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (num / den).astype(f32)
    return np.where(valid(x, valid_thresh), q, x).astype(f32)


def _reflect101(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def _pass(c, l1, r1, l2, r2):
    acc = f32(c * K0)
    acc = f32(acc + f32(f32(l1 + r1) * K1))
    return f32(acc + f32(f32(l2 + r2) * K2))


def gv_loop(x, valid_thresh=THR):
    """(b)"""
    x = np.asarray(x, f32)
    thr = f32(valid_thresh)
    R, C = x.shape
    out = x.copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for r in range(R):
            for c in range(C):
                if not x[r, c] >= thr:
                    continue
                hv, hm = [], []
                for dr in (-2, -1, 0, 1, 2):
                    rr = _reflect101(r + dr, R)
                    tv, tm = [], []
                    for dc in (-2, -1, 0, 1, 2):
                        t = x[rr, _reflect101(c + dc, C)]
                        ok = bool(t >= thr)
                        tv.append(t if ok else f32(0))
                        tm.append(f32(1) if ok else f32(0))
                    hv.append(_pass(tv[2], tv[1], tv[3], tv[0], tv[4]))
                    hm.append(_pass(tm[2], tm[1], tm[3], tm[0], tm[4]))
                num = _pass(hv[2], hv[1], hv[3], hv[0], hv[4])
                den = _pass(hm[2], hm[1], hm[3], hm[0], hm[4])
                out[r, c] = f32(num / den)
    return out


def holes_plane(rows, cols, seed, holes=0.4, lo=1.0, hi=90.0):
    """A dense plane with `holes` of its pixels invalid: zeros mostly, and every other kind of invalid value among them."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.uniform(lo, hi, (rows, cols)).astype(f32)
    h = g.random((rows, cols)) < holes
    kinds = g.integers(0, 8, (rows, cols))
    below = np.nextafter(THR, f32(0))
    x[h] = 0.0
    x[h & (kinds == 1)] = -0.0
    x[h & (kinds == 2)] = -3.5
    x[h & (kinds == 3)] = below
    return x


def nan_plane(rows, cols, seed):
    x = holes_plane(rows, cols, seed)
    g = np.random.Generator(np.random.PCG64(seed + 1000))
    x[g.random((rows, cols)) < 0.05] = np.nan
    return x


# ---- the cascade's finishes ----------------------------------------------------------------------------------------------------
def finish(x9, stop_after, max_depth=MAX_DEPTH, valid_thresh=THR):
    assert stop_after in (10, 11)
    x = gv_arrays(x9, valid_thresh)
    return x if stop_after == 10 else N.invert(x, max_depth, valid_thresh)


def no_extrapolate(sparse, k0="as_compiled", stop_after=11, labels=None, n_labels=0, max_depth=MAX_DEPTH, valid_thresh=THR):
    """complete(extrapolate=False, blur_type="gaussian_valid")"""
    x9 = NE.restatement_numpy(sparse, k0, "none", 9, labels, n_labels, max_depth, valid_thresh)
    return x9 if stop_after == 9 else finish(x9, stop_after, max_depth, valid_thresh)


def extrapolating(sparse, k0="as_compiled", stop_after=11, max_fill_iters=64, max_depth=MAX_DEPTH, valid_thresh=THR):
    """complete(blur_type="gaussian_valid"); returns (plane, info)"""
    k = N.K0_DIAMOND if k0 == "diamond" else N.K0_AS_COMPILED if k0 == "as_compiled" else np.asarray(k0, np.uint8).reshape(5, 5)
    info = {}
    x9 = N.img_completion(sparse, k0=k, stop_after=9, max_fill_iters=max_fill_iters, info=info, max_depth=max_depth, valid_thresh=valid_thresh)
    return (x9 if stop_after == 9 else finish(x9, stop_after, max_depth, valid_thresh)), info
