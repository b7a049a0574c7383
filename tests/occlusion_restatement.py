"""Two independent CPU restatements of the occlusion filter of projected LiDAR returns (include/dcmt.h: dcmt_sparse_occlusion_dev and
its payload form), and the planes and the scene the tests run them and the device on.

literal_occlusion(plane, **params)   the definition pixel by pixel: the return test on the bit pattern, the code of every return, and
                                for every return a double loop over its clipped window, all on Python ints.
shifted_occlusion(plane, **params)   the same definition vectorised: the return test on values, the codes as one array expression, the
                                window maximum as the maximum of (2 ry + 1)(2 rx + 1) shifted views of a zero-padded code plane.
Both take an f32 plane [rows][cols] (metres) or a uint16 one (the KITTI payload, metres = f32(value) * f32(scale), rounded once, as
dcmt_complete_u16_dev ingests it) and return (the filtered plane, the number of pixels changed).
params: rx 3, ry 6, tol_code 655, valid_thresh 0.1, max_depth 100, and for the payload scale 1 / 256.
Scenes: sparse_plane (anything a plane may hold), payload_plane, with_ties, lidar_scene (the issue's boxes in front of a wall)."""
import numpy as np

f32, f64, u16, u32 = np.float32, np.float64, np.uint16, np.uint32
W32 = f32(65536.0)
DEFAULTS = dict(rx=3, ry=6, tol_code=655, valid_thresh=0.1, max_depth=100.0, scale=1.0 / 256.0)
SPECIALS = (np.nan, np.inf, -np.inf, -0.0, -5.0, 0.05, 0.0999, 100.5, 1e30, 1e-40)


def _params(kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def _bits(x):
    return int(np.array(x, f32).view(u32))


def metres(plane, scale=DEFAULTS["scale"]):
    """The f32 depths of a plane: itself, or the ingest of a payload."""
    plane = np.asarray(plane)
    if plane.dtype == u16:
        return (plane.astype(f32) * f32(scale)).astype(f32)
    assert plane.dtype == f32
    return plane


# ------------------------------------------------------------------------------------------------------------------- literal
def literal_codes(plane, **kw):
    """The code of every pixel as a list of lists of Python ints (0: no return)."""
    p = _params(kw)
    z = metres(plane, p["scale"])
    lo, hi = _bits(p["valid_thresh"]), _bits(p["max_depth"])
    zb = z.view(u32).tolist()
    rows, cols = z.shape
    return [[int(np.rint(W32 / z[y, x])) if lo <= zb[y][x] <= hi else 0 for x in range(cols)] for y in range(rows)]


def literal_occlusion(plane, **kw):
    p = _params(kw)
    plane = np.asarray(plane)
    rows, cols = plane.shape
    rx, ry, tol = int(p["rx"]), int(p["ry"]), int(p["tol_code"])
    w = literal_codes(plane, **kw)
    out = plane.copy()
    removed = 0
    for y in range(rows):
        for x in range(cols):
            if w[y][x] == 0:
                continue
            m = 0
            for yy in range(max(0, y - ry), min(rows - 1, y + ry) + 1):
                for xx in range(max(0, x - rx), min(cols - 1, x + rx) + 1):
                    m = max(m, w[yy][xx])
            if m - w[y][x] > tol:
                out[y, x] = 0
                removed += 1
    return out, removed


# ------------------------------------------------------------------------------------------------------------------- vectorised
def shifted_codes(plane, **kw):
    """The code of every pixel as an int64 array (0: no return), the return test on values."""
    p = _params(kw)
    z = metres(plane, p["scale"])
    with np.errstate(all="ignore"):
        ret = np.isfinite(z) & (z >= f32(p["valid_thresh"])) & (z <= f32(p["max_depth"]))
        w = np.rint(W32 / np.where(ret, z, f32(1.0)))
    return np.where(ret, w, 0).astype(np.int64)


def shifted_occlusion(plane, **kw):
    p = _params(kw)
    plane = np.asarray(plane)
    rows, cols = plane.shape
    rx, ry, tol = int(p["rx"]), int(p["ry"]), int(p["tol_code"])
    w = shifted_codes(plane, **kw)
    pad = np.zeros((rows + 2 * ry, cols + 2 * rx), np.int64)
    pad[ry:ry + rows, rx:rx + cols] = w
    m = np.zeros_like(w)
    for dy in range(2 * ry + 1):
        for dx in range(2 * rx + 1):
            m = np.maximum(m, pad[dy:dy + rows, dx:dx + cols])
    occluded = (w > 0) & (m - w > tol)
    out = plane.copy()
    out[occluded] = 0
    return out, int(occluded.sum())


# ------------------------------------------------------------------------------------------------------------------- planes
def sparse_plane(rows, cols, density, seed, specials=True):
    """Anything a depth plane may hold: returns at `density` of the pixels, a slanted background between 12 and 60 m with patches of
    foreground at 3 to 8 m over it (so that returns are removed), zeros elsewhere, and with `specials` the exact bounds 0.1 and 100,
    values one ulp inside and outside them and every one of SPECIALS on a few pixels."""
    g = np.random.Generator(np.random.PCG64(seed))
    V, U = np.mgrid[0:rows, 0:cols]
    q = 1.0 / 60 + (1.0 / 12 - 1.0 / 60) * (U / max(cols, 2) * 0.5 + V / max(rows, 2) * 0.5) + g.uniform(0, 0.002, (rows, cols))
    near = ((U // 9 + V // 7) % 3 == 0)
    q = np.where(near, 1.0 / g.uniform(3, 8, (rows, cols)), q)
    depth = np.where(g.random((rows, cols)) < density, 1.0 / q, 0.0).astype(f32)
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


def payload_plane(rows, cols, density, seed):
    """sparse_plane as the KITTI payload: uint16 round(metres * 256), with 0, 1, 25, 26 (on either side of 0.1 m), 25600, 25601 (of
    100 m) and 65535 on a few pixels."""
    z = sparse_plane(rows, cols, density, seed)
    with np.errstate(all="ignore"):
        v = np.where(np.isfinite(z) & (z > 0) & (z < 255), np.rint(z.astype(f64) * 256.0), 0).astype(u16)
    flat = v.reshape(-1)
    spots = np.random.Generator(np.random.PCG64(seed + 1)).permutation(flat.size)
    for i, s in enumerate((0, 1, 25, 26, 25600, 25601, 65535)):
        if i < flat.size // 3:
            flat[spots[i]] = s
    return v


def with_ties(rows, cols, tol_code=DEFAULTS["tol_code"]):
    """A plane of pairs of horizontal neighbours whose codes differ by exactly tol_code (the far one is kept), by tol_code + 1 (it is
    removed) and by tol_code - 1, far apart from each other: (plane, the pixels that must go, the pixels of ties that must stay)."""
    z = np.zeros((rows, cols), f32)
    go, stay = [], []
    y, k = 0, 0
    while y < rows:
        x = 0
        while x + 1 < cols:
            far = 1000 + 37 * k
            d = (tol_code, tol_code + 1, tol_code - 1)[k % 3]
            near = far + d
            z[y, x], z[y, x + 1] = W32 / f32(far), W32 / f32(near)
            if d < 0 or near > (1 << 20):
                z[y, x] = z[y, x + 1] = 0
            elif int(np.rint(W32 / z[y, x])) == far and int(np.rint(W32 / z[y, x + 1])) == near:    # the codes are hit exactly
                (go if d > tol_code else stay).append((y, x))
            else:
                z[y, x] = z[y, x + 1] = 0
            k += 1
            x += 20
        y += 40
    return z, go, stay


# ------------------------------------------------------------------------------------------------------------------- the scene
F, CX, CY, ROWS, COLS = 721.5, 608.0, 176.0, 352, 1216
GROUND_Y, WALL_Z = 1.65, 40.0
BOXES = ((6.0, -1.0, 1.0, -0.2, 1.65), (12.0, 2.5, 4.5, 0.0, 1.65), (9.0, -5.0, -3.5, 0.2, 1.65))      # z; x range; y range


def _cast(o, d, boxes):
    """The distance along z (camera depth) of the first surface each ray o + t d hits, inf where none: o [3], d [n][3]."""
    with np.errstate(all="ignore"):
        t = np.where(d[:, 1] > 0, (GROUND_Y - o[1]) / d[:, 1], np.inf)
        t = np.minimum(t, np.where(d[:, 2] > 0, (WALL_Z - o[2]) / d[:, 2], np.inf))
        for z, x0, x1, y0, y1 in (BOXES if boxes else ()):
            tb = np.where(d[:, 2] > 0, (z - o[2]) / d[:, 2], np.inf)
            x, y = o[0] + tb * d[:, 0], o[1] + tb * d[:, 1]
            t = np.minimum(t, np.where((tb > 0) & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1), tb, np.inf))
    return t


def lidar_scene(boxes=True, lidar=(0.06, -0.08, -0.27)):
    """The scene of the issue in camera coordinates (x right, y down, z forward): ground at y = 1.65, a wall at z = 40 and, with
    boxes, three fronto-parallel boxes; a LiDAR at `lidar` casts rays at azimuth -45 .. 45 deg in steps of 0.17 and elevation
    -24.8 .. 2 deg in steps of 0.42; the hits are projected with f = 721.5, cx = 608, cy = 176 into 352 x 1216, the nearest hit wins
    a pixel.  Returns (the sparse f32 plane, the mask of its see-through returns: those whose depth exceeds 1.15 * the scene depth
    rendered from the camera at that pixel + 0.3 m)."""
    o = np.array(lidar, f64)
    az = np.deg2rad(np.arange(-45.0, 45.0 + 1e-9, 0.17))
    el = np.deg2rad(np.arange(-24.8, 2.0 + 1e-9, 0.42))
    A, E = np.meshgrid(az, el)
    d = np.stack([np.sin(A) * np.cos(E), -np.sin(E), np.cos(A) * np.cos(E)], -1).reshape(-1, 3)
    t = _cast(o, d, boxes)
    hit = np.isfinite(t)
    p = o + t[hit, None] * d[hit]
    p = p[p[:, 2] > 0.1]
    u = np.floor(F * p[:, 0] / p[:, 2] + CX + 0.5).astype(np.int64)
    v = np.floor(F * p[:, 1] / p[:, 2] + CY + 0.5).astype(np.int64)
    inside = (u >= 0) & (u < COLS) & (v >= 0) & (v < ROWS)
    u, v, z = u[inside], v[inside], p[inside, 2]
    sparse = np.full((ROWS, COLS), np.inf)
    np.minimum.at(sparse, (v, u), z)
    sparse = np.where(np.isfinite(sparse), sparse, 0.0).astype(f32)
    V, U = np.mgrid[0:ROWS, 0:COLS]
    rays = np.stack([(U - CX) / F, (V - CY) / F, np.ones(U.shape)], -1).reshape(-1, 3)
    scene = _cast(np.zeros(3), rays, boxes).reshape(ROWS, COLS)            # rays with d_z = 1: t is the depth
    see_through = (sparse > 0) & (sparse.astype(f64) > 1.15 * scene + 0.3)
    return sparse, see_through
