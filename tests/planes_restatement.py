"""Two independent CPU restatements of the per-superpixel plane fit (include/dcmt.h: dcmt_superpixel_planes_dev), and the scenes the
tests run them and the device on.

literal_planes(depth, labels, n_labels, **params)   the definition pixel by pixel and label by label: the return test on the bit
                                pattern, the moments as Python ints, the centred terms and the determinant as Python ints (exact
                                at any size), the solve on np.float64 scalars in the header's order (numpy never contracts), the
                                refit pass, the paint.  Returns (out f32 [rows][cols], fits FIT_DTYPE [n_labels]).
closed_planes(...)              the same definition vectorised: the return test on values, np.add.at / np.minimum.at into int64
                                tables, the exact terms as object arrays of Python ints, the solve and the paint as array
                                expressions.  Same returns.
float(int) and ndarray.astype(float64) of Python ints round to nearest, ties to even: dcmt.h's f64(i).
params: valid_thresh 0.1, max_depth 100, min_points 3, min_extent 2, refit_tol 0, keep_returns True.
Scenes: facet_scene, outlier_scene (exact affine inverse depth per label, with the f64 truth), sparse_depth (anything, with NaN, inf,
-0.0 and out-of-range values among it), and the adversarial label planes of contours_restatement."""
import numpy as np

from contours_restatement import PLANES, checkerboard, noise, out_of_range, plane_cases, rows_own_label, voronoi  # noqa: F401

f32, f64, i32 = np.float32, np.float64, np.int32
W32 = f32(65536.0)
W64 = f64(65536.0)
NONE, CONSTANT, PLANE = 0, 1, 2
FIT_DTYPE = np.dtype([("a", "<f8"), ("b", "<f8"), ("c", "<f8"), ("seen", "<u4"), ("used", "<u4"), ("wmin", "<u4"), ("wmax", "<u4"),
                      ("kind", "<u4"), ("reserved", "<u4")])
DEFAULTS = dict(valid_thresh=0.1, max_depth=100.0, min_points=3, min_extent=2, refit_tol=0.0, keep_returns=True)


def _params(kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def _bits(x):
    return int(np.array(x, f32).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------- literal
def _fit_literal(m, min_points, min_extent):
    """m: dict of Python ints -> (a, b, c, kind) as np.float64 / int."""
    n = m["n"]
    if n == 0:
        return f64(0.0), f64(0.0), f64(0.0), NONE
    F = lambda i: f64(float(i))                               # noqa: E731  f64(i): nearest, ties to even
    wbar = F(m["sw"]) / F(n)
    if n < min_points or m["umax"] - m["umin"] + 1 < min_extent or m["vmax"] - m["vmin"] + 1 < min_extent:
        return f64(0.0), f64(0.0), wbar, CONSTANT
    cuu = n * m["suu"] - m["su"] * m["su"]
    cuv = n * m["suv"] - m["su"] * m["sv"]
    cvv = n * m["svv"] - m["sv"] * m["sv"]
    cuw = n * m["suw"] - m["su"] * m["sw"]
    cvw = n * m["svw"] - m["sv"] * m["sw"]
    det = cuu * cvv - cuv * cuv
    if det <= 0:
        return f64(0.0), f64(0.0), wbar, CONSTANT
    a = (F(cuw) * F(cvv) - F(cvw) * F(cuv)) / F(det)
    b = (F(cvw) * F(cuu) - F(cuw) * F(cuv)) / F(det)
    c = (wbar - a * (F(m["su"]) / F(n))) - b * (F(m["sv"]) / F(n))
    return a, b, c, PLANE


def _empty():
    return dict(n=0, su=0, sv=0, suu=0, suv=0, svv=0, sw=0, suw=0, svw=0, umin=2 ** 32 - 1, umax=0, vmin=2 ** 32 - 1, vmax=0, wmin=2 ** 32 - 1, wmax=0)


def _add(m, u, v, w):
    m["n"] += 1
    m["su"] += u
    m["sv"] += v
    m["suu"] += u * u
    m["suv"] += u * v
    m["svv"] += v * v
    m["sw"] += w
    m["suw"] += u * w
    m["svw"] += v * w
    m["umin"], m["umax"] = min(m["umin"], u), max(m["umax"], u)
    m["vmin"], m["vmax"] = min(m["vmin"], v), max(m["vmax"], v)
    m["wmin"], m["wmax"] = min(m["wmin"], w), max(m["wmax"], w)


def literal_planes(depth, labels, n_labels, **kw):
    p = _params(kw)
    depth, labels = np.asarray(depth, f32), np.asarray(labels, i32)
    rows, cols = depth.shape
    lo, hi = _bits(p["valid_thresh"]), _bits(p["max_depth"])
    zb = depth.view(np.uint32).tolist()
    lab = labels.tolist()
    returns = []                                              # (u, v, label, w)
    for v in range(rows):
        for u in range(cols):
            k = lab[v][u]
            if 0 <= k < n_labels and lo <= zb[v][u] <= hi:
                returns.append((u, v, k, int(np.rint(W32 / depth[v, u]))))
    mom = [_empty() for _ in range(n_labels)]
    for u, v, k, w in returns:
        _add(mom[k], u, v, w)
    fits = np.zeros(n_labels, FIT_DTYPE)
    for k in range(n_labels):
        a, b, c, kind = _fit_literal(mom[k], p["min_points"], p["min_extent"])
        if kind != NONE:
            fits[k] = (a, b, c, mom[k]["n"], mom[k]["n"], mom[k]["wmin"], mom[k]["wmax"], kind, 0)
    tol = f64(f32(p["refit_tol"]))
    if tol > 0:
        mom2 = [_empty() for _ in range(n_labels)]
        for u, v, k, w in returns:
            if fits[k]["kind"] != PLANE:
                continue
            what = (fits[k]["a"] * f64(u) + fits[k]["b"] * f64(v)) + fits[k]["c"]
            if abs(f64(w) - what) <= tol * what:
                _add(mom2[k], u, v, w)
        for k in range(n_labels):
            if fits[k]["kind"] != PLANE:
                continue
            a, b, c, kind = _fit_literal(mom2[k], p["min_points"], p["min_extent"])
            if kind == PLANE:
                fits[k]["a"], fits[k]["b"], fits[k]["c"] = a, b, c
                fits[k]["used"], fits[k]["wmin"], fits[k]["wmax"] = mom2[k]["n"], mom2[k]["wmin"], mom2[k]["wmax"]
    out = np.zeros((rows, cols), f32)
    for v in range(rows):
        for u in range(cols):
            k = lab[v][u]
            if not 0 <= k < n_labels or fits[k]["kind"] == NONE:
                continue
            if p["keep_returns"] and lo <= zb[v][u] <= hi:
                out[v, u] = depth[v, u]
                continue
            what = (fits[k]["a"] * f64(u) + fits[k]["b"] * f64(v)) + fits[k]["c"]
            wmin, wmax = f64(fits[k]["wmin"]), f64(fits[k]["wmax"])
            what = wmin if what < wmin else (wmax if what > wmax else what)
            out[v, u] = f32(W64 / what)
    return out, fits


# ------------------------------------------------------------------------------------------------------------------- vectorised
def _table(n_labels, k, u, v, w):
    """Moments of the returns (k, u, v, w: int64 arrays) per label, as a dict of int64 arrays."""
    t = {name: np.zeros(n_labels, np.int64) for name in ("n", "su", "sv", "suu", "suv", "svv", "sw", "suw", "svw", "umax", "vmax", "wmax")}
    for name in ("umin", "vmin", "wmin"):
        t[name] = np.full(n_labels, 2 ** 32 - 1, np.int64)
    for name, x in (("n", np.ones_like(u)), ("su", u), ("sv", v), ("suu", u * u), ("suv", u * v), ("svv", v * v), ("sw", w), ("suw", u * w), ("svw", v * w)):
        np.add.at(t[name], k, x)
    for name, x in (("umin", u), ("vmin", v), ("wmin", w)):
        np.minimum.at(t[name], k, x)
    for name, x in (("umax", u), ("vmax", v), ("wmax", w)):
        np.maximum.at(t[name], k, x)
    return t


def _fit_closed(t, min_points, min_extent):
    """-> (a, b, c, kind) arrays."""
    O = {name: t[name].astype(object) for name in ("n", "su", "sv", "suu", "suv", "svv", "sw", "suw", "svw")}
    n = O["n"]
    cuu, cuv, cvv = n * O["suu"] - O["su"] * O["su"], n * O["suv"] - O["su"] * O["sv"], n * O["svv"] - O["sv"] * O["sv"]
    cuw, cvw = n * O["suw"] - O["su"] * O["sw"], n * O["svw"] - O["sv"] * O["sw"]
    det = cuu * cvv - cuv * cuv
    F = lambda x: x.astype(f64)                               # noqa: E731
    some = t["n"] > 0
    plane = some & (t["n"] >= min_points) & (t["umax"] - t["umin"] + 1 >= min_extent) & (t["vmax"] - t["vmin"] + 1 >= min_extent) & np.array(det > 0, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        nd = F(n)
        wbar = F(O["sw"]) / nd
        a = (F(cuw) * F(cvv) - F(cvw) * F(cuv)) / F(det)
        b = (F(cvw) * F(cuu) - F(cuw) * F(cuv)) / F(det)
        c = (wbar - a * (F(O["su"]) / nd)) - b * (F(O["sv"]) / nd)
    a, b = np.where(plane, a, 0.0), np.where(plane, b, 0.0)
    c = np.where(plane, c, np.where(some, wbar, 0.0))
    return a, b, c, np.where(plane, PLANE, np.where(some, CONSTANT, NONE))


def closed_planes(depth, labels, n_labels, **kw):
    p = _params(kw)
    depth, labels = np.asarray(depth, f32), np.asarray(labels, i32)
    with np.errstate(invalid="ignore"):
        ret = np.isfinite(depth) & (depth >= f32(p["valid_thresh"])) & (depth <= f32(p["max_depth"])) & (labels >= 0) & (labels < n_labels)
    vv, uu = np.nonzero(ret)
    vv, uu = vv.astype(np.int64), uu.astype(np.int64)
    k = labels[ret].astype(np.int64)
    w = np.rint(W32 / depth[ret]).astype(np.int64)
    t = _table(n_labels, k, uu, vv, w)
    a, b, c, kind = _fit_closed(t, p["min_points"], p["min_extent"])
    used, wmin, wmax = t["n"].copy(), t["wmin"].copy(), t["wmax"].copy()
    tol = f64(f32(p["refit_tol"]))
    if tol > 0:
        what = (a[k] * uu.astype(f64) + b[k] * vv.astype(f64)) + c[k]
        sel = (kind[k] == PLANE) & (np.abs(w.astype(f64) - what) <= tol * what)
        t2 = _table(n_labels, k[sel], uu[sel], vv[sel], w[sel])
        a2, b2, c2, kind2 = _fit_closed(t2, p["min_points"], p["min_extent"])
        new = (kind == PLANE) & (kind2 == PLANE)
        a, b, c = np.where(new, a2, a), np.where(new, b2, b), np.where(new, c2, c)
        used, wmin, wmax = np.where(new, t2["n"], used), np.where(new, t2["wmin"], wmin), np.where(new, t2["wmax"], wmax)
    fits = np.zeros(n_labels, FIT_DTYPE)
    some = kind != NONE
    fits["a"], fits["b"], fits["c"], fits["kind"] = a, b, c, kind
    fits["seen"], fits["used"] = t["n"], np.where(some, used, 0)
    fits["wmin"], fits["wmax"] = np.where(some, wmin, 0), np.where(some, wmax, 0)
    rows, cols = depth.shape
    inside = (labels >= 0) & (labels < n_labels)
    L = np.where(inside, labels, 0).astype(np.int64)
    painted = inside & some[L]
    V, U = np.mgrid[0:rows, 0:cols]
    what = (a[L] * U.astype(f64) + b[L] * V.astype(f64)) + c[L]
    what = np.minimum(np.maximum(what, wmin[L].astype(f64)), wmax[L].astype(f64))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(painted, (W64 / what).astype(f32), f32(0.0)).astype(f32)
    if p["keep_returns"]:
        out[ret] = depth[ret]
    return out, fits


# ---------------------------------------------------------------------------------------------------------------- the scenes
def _grid(n_facets, rows, cols):
    """(gy, gx) with gy * gx == n_facets whose blocks are nearest to square."""
    pairs = [(gy, n_facets // gy) for gy in range(1, n_facets + 1) if n_facets % gy == 0]
    return min(pairs, key=lambda g: abs(np.log((cols / g[1]) / (rows / g[0]))))


def facet_scene(rows, cols, n_facets, density, seed):
    """Labels from a grid of n_facets blocks whose borders are jittered by up to two pixels per row and per column; every label has an
    exact affine inverse depth q(u, v) inside [1/80, 1/3] over its block; returns (f32(1 / q)) at `density` of the pixels.  Returns
    (depth f32, labels int32, n_labels, truth f64 [rows][cols] = 1 / q of every pixel's own facet)."""
    g = np.random.Generator(np.random.PCG64(seed))
    gy, gx = _grid(n_facets, rows, cols)
    V, U = np.mgrid[0:rows, 0:cols]
    jx, jy = g.integers(-2, 3, rows)[:, None], g.integers(-2, 3, cols)[None, :]
    bx = np.clip((U - jx) * gx // cols, 0, gx - 1)
    by = np.clip((V - jy) * gy // rows, 0, gy - 1)
    labels = (by * gx + bx).astype(i32)
    hw, hh = cols / gx / 2 + 2, rows / gy / 2 + 2             # half a block and its jitter
    q0 = g.uniform(1 / 40, 1 / 6, n_facets)
    room = 0.8 * np.minimum(q0 - 1 / 80, 1 / 3 - q0)
    share = g.uniform(0.1, 0.9, n_facets)
    qa = g.choice([-1.0, 1.0], n_facets) * room * share / hw
    qb = g.choice([-1.0, 1.0], n_facets) * room * (1 - share) / hh
    uc, vc = (np.arange(n_facets) % gx + 0.5) * cols / gx, (np.arange(n_facets) // gx + 0.5) * rows / gy
    q = q0[labels] + qa[labels] * (U - uc[labels]) + qb[labels] * (V - vc[labels])
    assert q.min() >= 1 / 80 and q.max() <= 1 / 3
    truth = 1.0 / q
    depth = np.where(g.random((rows, cols)) < density, truth, 0.0).astype(f32)
    return depth, labels, n_facets, truth


def outlier_scene(rows, cols, n_facets, density, seed, facet=0, share=0.2, factor=1.5):
    """facet_scene with `share` of the returns of `facet` moved to `factor` times their depth.  Returns (depth, labels, n_labels,
    truth, facet)."""
    depth, labels, n, truth = facet_scene(rows, cols, n_facets, density, seed)
    g = np.random.Generator(np.random.PCG64(seed + 7919))
    idx = np.flatnonzero((labels == facet) & (depth > 0))
    moved = g.choice(idx, max(1, int(round(share * len(idx)))), replace=False)
    depth = depth.copy()
    depth.flat[moved] = (depth.flat[moved] * f32(factor)).astype(f32)
    return depth, labels, n, truth, facet


SPECIALS = (np.nan, np.inf, -np.inf, -0.0, -5.0, 0.05, 0.0999, 100.5, 1e30, 1e-40)


def sparse_depth(rows, cols, density, seed):
    """Anything a depth plane may hold: returns between 0.1 and 100 m at `density` of the pixels (a slanted surface with noise, and the
    exact bounds 0.1 and 100), zeros elsewhere, and every one of SPECIALS on a few pixels (no returns, any of them)."""
    g = np.random.Generator(np.random.PCG64(seed))
    V, U = np.mgrid[0:rows, 0:cols]
    q = 0.02 + 0.2 * U / max(cols, 2) + 0.1 * V / max(rows, 2) + g.uniform(0, 0.01, (rows, cols))
    depth = np.where(g.random((rows, cols)) < density, 1.0 / q, 0.0).astype(f32)
    flat = depth.reshape(-1)
    spots = g.permutation(flat.size)
    for i, s in enumerate((f32(0.1), f32(100.0)) + SPECIALS):
        for j in range(2):
            if 2 * i + j < flat.size // 3:
                flat[spots[2 * i + j]] = f32(s)
    return depth


def block_labels(rows, cols, step):
    """Square blocks of `step` pixels, numbered row-major: (labels, n_labels)."""
    V, U = np.mgrid[0:rows, 0:cols]
    nx = (cols + step - 1) // step
    return (V // step * nx + U // step).astype(i32), nx * ((rows + step - 1) // step)


def pixel_labels(rows, cols):
    """Every pixel its own label."""
    return np.arange(rows * cols, dtype=i32).reshape(rows, cols), rows * cols
