"""Two independent CPU restatements of the distance to the nearest LiDAR return and of the trust mask (include/dcmt.h:
dcmt_support_distance_dev and its payload form), and the planes the tests run them and the device on.

literal_dist2(plane, **params)   the definition: the list of the frame's returns, and for every pixel the minimum over that list of
                                 (y - y')^2 + (x - x')^2 in integers; then the cap.  Neither pass of the device's scheme appears.
edt_dist2(plane, **params)       scipy.ndimage.distance_transform_edt on the mask of returns and rint(d * d): exact for these sizes
                                 (d * d is within a few ulp of an integer below 2^24).
Both take the return test from the bit pattern, on an f32 plane [rows][cols] (metres) or a uint16 one (the KITTI payload, metres =
f32(value) * f32(scale), rounded once, as dcmt_complete_u16_dev ingests it), and return (the uint16 plane: D2 where D2 <= R^2, 65535
elsewhere; the number of pixels beyond R).
select(dist2, dense, fallback)   the trust mask on the bits: dense where dist2 != 65535, elsewhere fallback or +0.0.
params: max_radius 9, valid_thresh 0.1, max_depth 100, and for the payload scale 1 / 256."""
import numpy as np
from scipy import ndimage

f32, u16, u32 = np.float32, np.uint16, np.uint32
BEYOND = 65535
DEFAULTS = dict(max_radius=9, valid_thresh=0.1, max_depth=100.0, scale=1.0 / 256.0)
SPECIALS = (np.nan, np.inf, -np.inf, -0.0, -5.0, 0.05, 0.0999, 100.5, 1e30, 1e-40)


def _params(kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def returns_mask(plane, **kw):
    """The return test on the bit pattern: lo <= bits <= hi, the bits of the two positive bounds; NaN, +-inf, negatives and -0.0 have
    bits above any positive finite float's."""
    p = _params(kw)
    plane = np.asarray(plane)
    if plane.dtype == u16:
        z = (plane.astype(f32) * f32(p["scale"])).astype(f32)
    else:
        assert plane.dtype == f32
        z = plane
    zb = np.ascontiguousarray(z).view(u32)
    lo, hi = (int(np.array(p[k], f32).view(u32)) for k in ("valid_thresh", "max_depth"))
    return (zb >= lo) & (zb <= hi)


def _cap(d2, R):
    far = d2 > R * R
    return np.where(far, BEYOND, d2).astype(u16), int(far.sum())


# ------------------------------------------------------------------------------------------------------------------- literal
def literal_dist2(plane, **kw):
    p = _params(kw)
    ret = returns_mask(plane, **kw)
    rows, cols = ret.shape
    ys, xs = (a.astype(np.int64) for a in np.nonzero(ret))
    d2 = np.full((rows, cols), 1 << 40, np.int64)             # "infinite": a frame without returns
    X = np.arange(cols, dtype=np.int64)
    for y in range(rows):
        best = d2[y]
        for i in range(0, len(ys), 4096):                       # the minimum over the list of returns, a slab of the list at a time
            cand = (y - ys[i:i + 4096, None]) ** 2 + (X[None, :] - xs[i:i + 4096, None]) ** 2
            np.minimum(best, cand.min(axis=0), out=best)
    return _cap(d2, int(p["max_radius"]))


# ------------------------------------------------------------------------------------------------------------------- scipy
def edt_dist2(plane, **kw):
    p = _params(kw)
    ret = returns_mask(plane, **kw)
    if not ret.any():
        return _cap(np.full(ret.shape, 1 << 40, np.int64), int(p["max_radius"]))
    d = ndimage.distance_transform_edt(~ret)
    return _cap(np.rint(d * d).astype(np.int64), int(p["max_radius"]))


def select(dist2, dense, fallback=None):
    """The trust mask, on the bits."""
    d = np.ascontiguousarray(dense, f32).view(u32)
    fb = np.zeros_like(d) if fallback is None else np.ascontiguousarray(fallback, f32).view(u32)
    return np.where(dist2 != BEYOND, d, fb).view(f32)


# ------------------------------------------------------------------------------------------------------------------- planes
def sparse_plane(rows, cols, density, seed, specials=True):
    """Anything a sparse plane may hold: returns between 0.5 and 80 m at `density` of the pixels, in clumps with empty stretches
    between them (so that distances of every size occur), zeros elsewhere, and with `specials` the exact bounds 0.1 and 100, values one
    ulp inside and outside them and every one of SPECIALS on a few pixels."""
    g = np.random.Generator(np.random.PCG64(seed))
    V, U = np.mgrid[0:rows, 0:cols]
    clump = ((U // 23 + V // 11 + seed) % 3 != 0)
    depth = np.where((g.random((rows, cols)) < density) & clump, g.uniform(0.5, 80.0, (rows, cols)), 0.0).astype(f32)
    if not specials:
        return depth
    flat = depth.reshape(-1)
    spots = g.permutation(flat.size)
    lo, hi = f32(0.1), f32(100.0)
    edge = (lo, hi, np.nextafter(lo, f32(0)), np.nextafter(lo, f32(1)), np.nextafter(hi, f32(0)), np.nextafter(hi, f32(1000)))
    for i, s in enumerate(edge + SPECIALS):
        if i < flat.size // 3:
            flat[spots[i]] = f32(s)
    return depth


def payload_plane(rows, cols, density, seed):
    """sparse_plane as the KITTI payload: uint16 round(metres * 256), with 0, 1, 25, 26 (on either side of 0.1 m), 25600, 25601 (of
    100 m) and 65535 on a few pixels."""
    z = sparse_plane(rows, cols, density, seed, specials=False)
    v = np.rint(z.astype(np.float64) * 256.0).astype(u16)
    flat = v.reshape(-1)
    spots = np.random.Generator(np.random.PCG64(seed + 1)).permutation(flat.size)
    for i, s in enumerate((0, 1, 25, 26, 25600, 25601, 65535)):
        if i < flat.size // 3:
            flat[spots[i]] = s
    return v


def dense_planes(rows, cols, seed):
    """(dense, fallback): f32 planes with values everywhere and, on every fifth pixel, NaNs with payloads, infinities, -0.0 and a
    denormal in turn, whose bits a select must keep."""
    g = np.random.Generator(np.random.PCG64(seed))
    out = []
    for k in range(2):
        a = g.uniform(0.5, 90.0, (rows, cols)).astype(f32)
        b = a.view(u32).reshape(-1)
        odd = np.array((0x7fc00001, 0xffc12345, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001), u32) + u32(2 * k)
        b[k::5] = np.resize(odd, len(b[k::5]))
        out.append(a)
    return out[0], out[1]
