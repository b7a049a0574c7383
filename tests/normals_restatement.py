"""Two independent CPU restatements of the surface normals and the flying-pixel filter of a depth plane (include/dcmt.h:
dcmt_depth_normals_dev), neither shaped like the kernel, the f64 evaluation of the same formula, and the planes the tests run them
and the device on.

literal(depth, **params)      the definition pixel by pixel on numpy f32 scalars, one rounding per operation: validity from the bit
                              pattern, the neighbours by index, Python's own control flow for the four cases of a gradient.  `watch`
                              is called with (name, value) for every intermediate (the bounds claim of dcmt.h is checked through it).
vectorised(depth, **params)   whole planes: validity from the values, w on a plane padded with zeros, the four differences as shifted
                              views, the cases as np.where.
Both return (normals f32 [rows][cols][4] = nx ny nz dist, out f32 [rows][cols], removed, valid pixels with no normal).
exact(w, **intrinsics)        the statement in f64 on a plane of INVERSE depths, no rounding to f32 anywhere: (normals, dist).
params: min_plane_dist 0.4, valid_thresh 0.1, max_depth 100 and the intrinsics fx fy cx cy (the library's defaults)."""
import numpy as np

f32, f64, u32 = np.float32, np.float64, np.uint32
DEFAULTS = dict(min_plane_dist=0.4, valid_thresh=0.1, max_depth=100.0, fx=9.597910e+02, fy=9.569251e+02, cx=6.960217e+02, cy=2.241806e+02)
SPECIALS = (np.nan, np.inf, -np.inf, -0.0, -5.0, 0.05, 0.0999, 100.5, 1e30, 1e-40)
KITTI = dict(fx=721.5, fy=721.5, cx=608.0, cy=176.0)
ONE = f32(1.0)


def _params(kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def _bits(x):
    return int(np.array(x, f32).view(u32))


# ------------------------------------------------------------------------------------------------------------------- literal
def _gradient(w, nxt, prv, note):
    """dcmt.h's GRADIENT of one axis: nxt / prv the w of the next / previous pixel or None.  None where there is neither."""
    F = note("F", nxt - w) if nxt is not None else None
    B = note("B", w - prv) if prv is not None else None
    if F is not None and B is not None:
        return F if abs(F) <= abs(B) else B
    return F if F is not None else B


def literal(depth, watch=None, **kw):
    p = _params(kw)
    depth = np.ascontiguousarray(depth, f32)
    rows, cols = depth.shape
    lo, hi = _bits(p["valid_thresh"]), _bits(p["max_depth"])
    fx, fy, cx, cy = (f32(f64(p[k])) for k in ("fx", "fy", "cx", "cy"))
    dmin = f32(p["min_plane_dist"])

    def note(name, v):
        if watch is not None:
            watch(name, v)
        return v

    with np.errstate(all="ignore"):
        dmin2 = note("dmin2", dmin * dmin)
        zb = depth.view(u32).tolist()
        w = [[note("w", ONE / depth[y, x]) if lo <= zb[y][x] <= hi else None for x in range(cols)] for y in range(rows)]
        normals = np.zeros((rows, cols, 4), f32)
        out = depth.copy()
        removed = none = 0
        for y in range(rows):
            for x in range(cols):
                wc = w[y][x]
                if wc is None:
                    continue
                gx = _gradient(wc, w[y][x + 1] if x + 1 < cols else None, w[y][x - 1] if x > 0 else None, note)
                gy = _gradient(wc, w[y + 1][x] if y + 1 < rows else None, w[y - 1][x] if y > 0 else None, note)
                if gx is None or gy is None:
                    none += 1
                    continue
                a, b = note("a", fx * gx), note("b", fy * gy)
                dx, dy = note("dx", f32(x) - cx), note("dy", f32(y) - cy)
                c = note("c", note("c1", wc - note("px", gx * dx)) - note("py", gy * dy))
                len2 = note("len2", note("ab", note("aa", a * a) + note("bb", b * b)) + note("cc", c * c))
                dist = note("dist", ONE / note("len", np.sqrt(len2)))
                normals[y, x] = (note("nx", -a * dist), note("ny", -b * dist), note("nz", -c * dist), dist)
                if note("rem", len2 * dmin2) > ONE:
                    out[y, x] = 0
                    removed += 1
    return normals, out, removed, none


# ------------------------------------------------------------------------------------------------------------------- vectorised
def _axis_gradient(W, V, axis):
    """The gradient of the padded plane W (validity V) along `axis` for the inner pixels, and where it exists."""
    inner = (slice(1, -1), slice(1, -1))
    nxt = (slice(2, None), slice(1, -1)) if axis == 0 else (slice(1, -1), slice(2, None))
    prv = (slice(None, -2), slice(1, -1)) if axis == 0 else (slice(1, -1), slice(None, -2))
    F, B = (W[nxt] - W[inner]).astype(f32), (W[inner] - W[prv]).astype(f32)
    hf, hb = V[nxt], V[prv]
    return np.where(hf & (~hb | (np.abs(F) <= np.abs(B))), F, B).astype(f32), hf | hb


def vectorised(depth, **kw):
    p = _params(kw)
    depth = np.ascontiguousarray(depth, f32)
    rows, cols = depth.shape
    fx, fy, cx, cy = (f32(f64(p[k])) for k in ("fx", "fy", "cx", "cy"))
    dmin = f32(p["min_plane_dist"])
    with np.errstate(all="ignore"):
        valid = np.isfinite(depth) & (depth >= f32(p["valid_thresh"])) & (depth <= f32(p["max_depth"]))
        W = np.zeros((rows + 2, cols + 2), f32)
        V = np.zeros((rows + 2, cols + 2), bool)
        W[1:-1, 1:-1] = np.where(valid, ONE / np.where(valid, depth, ONE), f32(0))
        V[1:-1, 1:-1] = valid
        gx, okx = _axis_gradient(W, V, 1)
        gy, oky = _axis_gradient(W, V, 0)
        has = valid & okx & oky
        w = W[1:-1, 1:-1]
        a, b = fx * gx, fy * gy
        dx = (np.arange(cols, dtype=f32) - cx)[None, :]
        dy = (np.arange(rows, dtype=f32) - cy)[:, None]
        c = (w - gx * dx) - gy * dy
        len2 = (a * a + b * b) + c * c
        dist = ONE / np.sqrt(np.where(has, len2, ONE))
        rec = np.stack([-a * dist, -b * dist, -c * dist, dist], -1).astype(f32)
        normals = np.where(has[..., None], rec, f32(0)).astype(f32)
        gone = has & (len2 * (dmin * dmin) > ONE)
    out = depth.copy()
    out[gone] = 0
    return normals, out, int(gone.sum()), int((valid & ~has).sum())


# ------------------------------------------------------------------------------------------------------------------- f64
def exact(w, fx, fy, cx, cy):
    """The statement evaluated in f64 on a dense plane of inverse depths w [rows][cols] (f64, all valid): (unit normals [rows][cols][3],
    plane distances [rows][cols]) of the pixels that have both gradients."""
    w = np.asarray(w, f64)
    rows, cols = w.shape

    def grad(axis):
        d = np.diff(w, axis=axis)
        nan = np.full((1, cols) if axis == 0 else (rows, 1), np.nan)
        F, B = np.concatenate([d, nan], axis), np.concatenate([nan, d], axis)
        return np.where(np.isnan(B) | (~np.isnan(F) & (np.abs(F) <= np.abs(B))), F, B)

    gx, gy = grad(1), grad(0)
    V, U = np.mgrid[0:rows, 0:cols].astype(f64)
    n = np.stack([fx * gx, fy * gy, w - gx * (U - cx) - gy * (V - cy)], -1)
    ln = np.sqrt((n * n).sum(-1))
    return -n / ln[..., None], 1.0 / ln


def plane_inverse_depth(normal, dist, rows, cols, fx, fy, cx, cy):
    """The exactly affine inverse depth (f64) a pinhole camera sees of the plane m . P = dist, m a unit vector: w = m . ray / dist."""
    m = np.asarray(normal, f64)
    V, U = np.mgrid[0:rows, 0:cols].astype(f64)
    return (m[0] * (U - cx) / fx + m[1] * (V - cy) / fy + m[2]) / dist


# ------------------------------------------------------------------------------------------------------------------- planes
def holey_plane(rows, cols, seed, holes=0.4, specials=True):
    """Anything a depth plane may hold: a slanted background between 12 and 60 m with patches of foreground at 3 to 8 m, noise that
    makes steep local planes (so that pixels are removed), `holes` of the pixels zero, and with `specials` the exact bounds 0.1 and
    100, values one ulp inside and outside them and every one of SPECIALS on a few pixels."""
    g = np.random.Generator(np.random.PCG64(seed))
    V, U = np.mgrid[0:rows, 0:cols]
    q = 1.0 / 60 + (1.0 / 12 - 1.0 / 60) * (U / max(cols, 2) * 0.5 + V / max(rows, 2) * 0.5) + g.uniform(0, 0.0005, (rows, cols))
    near = ((U // 9 + V // 7) % 3 == 0)
    q = np.where(near, 1.0 / g.uniform(3, 8, (rows, cols)), q)
    depth = np.where(g.random((rows, cols)) < 1.0 - holes, 1.0 / q, 0.0).astype(f32)
    if not specials:
        return depth
    flat = depth.reshape(-1)
    spots = g.permutation(flat.size)
    lo, hi = f32(0.1), f32(100.0)
    edge = (lo, hi, np.nextafter(lo, f32(0)), np.nextafter(lo, f32(1)), np.nextafter(hi, f32(0)), np.nextafter(hi, f32(1000)))
    for i, s in enumerate(edge + SPECIALS):
        for j in range(2):
            if 2 * i + j < flat.size // 3:
                flat[spots[2 * i + j]] = f32(s)
    return depth


def smooth_plane(rows, cols, seed):
    """A dense plane without holes: a ground-like slant in inverse depth with a gentle ripple."""
    g = np.random.Generator(np.random.PCG64(seed))
    V, U = np.mgrid[0:rows, 0:cols].astype(f64)
    q = 0.02 + 0.0004 * V + 0.00005 * U + 0.0002 * np.sin(U / 7.0) * np.cos(V / 5.0) + g.uniform(0, 1e-6, (rows, cols))
    return (1.0 / q).astype(f32)


def tie_planes(rows, cols):
    """Two planes on which F and B tie: `lin`, whose w is meant to be (64 + x + 2 y) / 1024, exactly linear on both axes (F == B) --
    z = fdiv(1024, k) gives back w = k / 1024 exactly at most pixels, not at all: linear_ties says where; and `peak`, whose w
    alternates 0.5 and 0.25 like a chessboard: F == -B at every inner pixel, on both axes."""
    V, U = np.mgrid[0:rows, 0:cols]
    lin = (f32(1024.0) / (64 + U + 2 * V).astype(f32)).astype(f32)
    peak = np.where((U + V) % 2 == 0, f32(2.0), f32(4.0)).astype(f32)
    return lin, peak


def linear_ties(lin):
    """The inner pixels of tie_planes' `lin` at which F == B != 0 holds exactly on both axes, as a mask."""
    w = (ONE / lin).astype(f32)
    m = np.zeros(lin.shape, bool)
    fx, bx = w[1:-1, 2:] - w[1:-1, 1:-1], w[1:-1, 1:-1] - w[1:-1, :-2]
    fy, by = w[2:, 1:-1] - w[1:-1, 1:-1], w[1:-1, 1:-1] - w[:-2, 1:-1]
    m[1:-1, 1:-1] = (fx == bx) & (fy == by) & (fx != 0) & (fy != 0)
    return m
