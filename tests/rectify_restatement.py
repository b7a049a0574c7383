"""The undistort-and-rectify map and the fixed-point bilinear remap of include/dcmt.h ("in front of the stereo calls"), restated in
numpy: what dcmt_rectify_map_dev and dcmt_rectify_dev are compared with, bit for bit.  The definition is the header's own -- stated,
never compared with an executing OpenCV.  Every f64 operation below is one numpy operation, in the header's order."""
import numpy as np

from depth_completion_mt_amd import api

OUTSIDE = np.int32(-2**31)
FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")

# a KITTI-magnitude record: the numbers of a 2011_09_26-style calib_cam_to_cam.txt (K_02, D_02, R_rect_02, P_rect_02), an unrectified
# 512 x 1392 sensor and a 375 x 1242 rectified view
KITTI_K = np.array([[9.597910e+02, 0.0, 6.960217e+02], [0.0, 9.569251e+02, 2.241806e+02], [0.0, 0.0, 1.0]])
KITTI_D = np.array([-3.691481e-01, 1.968681e-01, 1.353473e-03, 5.677587e-04, -6.770705e-02])
KITTI_R = np.array([[9.998817e-01, 1.511453e-02, -2.841595e-03], [-1.511724e-02, 9.998853e-01, -9.338510e-04],
                    [2.827154e-03, 9.766976e-04, 9.999955e-01]])
KITTI_P = np.array([[7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01], [0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01],
                    [0.0, 0.0, 1.0, 2.745884e-03]])
KITTI_SRC = (512, 1392)
KITTI_DST = (375, 1242)


def record(K, D, R, P) -> np.ndarray:
    """One dcmt_rectify_calib as a structured scalar array [1], without make_rectify_calib's refusals (a test may want a bad one)."""
    out = np.zeros(1, api.RECTIFY_CALIB_DTYPE)
    K, D, R, P = (np.asarray(a, dtype=np.float64) for a in (K, D, R, P))
    out["fx"], out["fy"], out["cx"], out["cy"] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    out["k1"], out["k2"], out["p1"], out["p2"], out["k3"] = D
    out["R"] = R.reshape(9)
    out["fxp"], out["fyp"], out["cxp"], out["cyp"] = P[0, 0], P[1, 1], P[0, 2], P[1, 2]
    return out


def record_ok(rec) -> bool:
    v = np.frombuffer(np.ascontiguousarray(rec).tobytes(), dtype=np.float64)
    return bool(np.isfinite(v).all() and rec["fxp"] != 0 and rec["fyp"] != 0)


def _coords(rec, rows: int, cols: int, ft):
    """mx * 32 and my * 32 of every destination pixel in float type ft, the header's order of operations."""
    g = lambda name: ft(rec[name])
    R = [ft(v) for v in np.asarray(rec["R"], dtype=np.float64).reshape(9)]
    two, one = ft(2), ft(1)
    u = np.arange(cols, dtype=ft)[None, :] + np.zeros((rows, 1), ft)
    v = np.arange(rows, dtype=ft)[:, None] + np.zeros((1, cols), ft)
    x = (u - g("cxp")) / g("fxp")
    y = (v - g("cyp")) / g("fyp")
    X = (R[0] * x + R[3] * y) + R[6]
    Y = (R[1] * x + R[4] * y) + R[7]
    W = (R[2] * x + R[5] * y) + R[8]
    xn, yn = X / W, Y / W
    x2, y2 = xn * xn, yn * yn
    r2 = x2 + y2
    xy2 = (two * xn) * yn
    kr = one + ((g("k3") * r2 + g("k2")) * r2 + g("k1")) * r2
    xd = (xn * kr + g("p1") * xy2) + g("p2") * (r2 + two * x2)
    yd = (yn * kr + g("p1") * (r2 + two * y2)) + g("p2") * xy2
    mx = g("fx") * xd + g("cx")
    my = g("fy") * yd + g("cy")
    return mx * ft(32), my * ft(32)


def rectify_map(rec, rows: int, cols: int) -> np.ndarray:
    """int32 [rows][cols][2] = (sx, sy) of one record (a structured scalar or an array of one)."""
    rec = np.asarray(rec).reshape(-1)[0]
    out = np.full((rows, cols, 2), OUTSIDE, np.int32)
    if not record_ok(rec):
        return out
    with np.errstate(all="ignore"):
        tx, ty = _coords(rec, rows, cols, np.float64)
        inside = np.isfinite(tx) & np.isfinite(ty) & (np.abs(tx) < 2.0**30) & (np.abs(ty) < 2.0**30)
        sx = np.rint(np.where(inside, tx, 0.0)).astype(np.int32)          # np.rint: ties to even
        sy = np.rint(np.where(inside, ty, 0.0)).astype(np.int32)
    out[..., 0] = np.where(inside, sx, OUTSIDE)
    out[..., 1] = np.where(inside, sy, OUTSIDE)
    return out


def rectify_maps(table, rows: int, cols: int) -> np.ndarray:
    return np.stack([rectify_map(table[i], rows, cols) for i in range(len(table))])


def coords_longdouble(rec, rows: int, cols: int):
    """(32 * mx, 32 * my) evaluated in np.longdouble: the yardstick of the map's accuracy."""
    rec = np.asarray(rec).reshape(-1)[0]
    return _coords(rec, rows, cols, np.longdouble)


def _sample(src, y, x):
    """p(y, x) per pixel of the destination: src [rows][cols][ch] int64, zero outside; y, x int64 arrays."""
    r, c = src.shape[:2]
    ok = (y >= 0) & (y < r) & (x >= 0) & (x < c)
    v = src[np.clip(y, 0, r - 1), np.clip(x, 0, c - 1)]
    return np.where(ok[..., None], v, 0)


def remap(src: np.ndarray, m: np.ndarray) -> np.ndarray:
    """One frame: src uint8 [src_rows][src_cols] or [..][3] through map m int32 [rows][cols][2] (any contents)."""
    grey = src.ndim == 2
    s = src.astype(np.int64).reshape(src.shape[0], src.shape[1], -1)
    sx, sy = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    ix, ax, iy, ay = sx >> 5, (sx & 31)[..., None], sy >> 5, (sy & 31)[..., None]
    top = (32 - ax) * _sample(s, iy, ix) + ax * _sample(s, iy, ix + 1)
    bot = (32 - ax) * _sample(s, iy + 1, ix) + ax * _sample(s, iy + 1, ix + 1)
    out = (((32 - ay) * top + ay * bot + 512) >> 10).astype(np.uint8)
    return out[..., 0] if grey else out


def rectify(src: np.ndarray, maps: np.ndarray, index=None) -> np.ndarray:
    """A batch: src uint8 [b][r][c] or [b][r][c][3], maps [n_maps][rows][cols][2]; frame f uses map index[f] (an index outside
    0 .. n_maps - 1: a zero frame), or f % n_maps without one."""
    n = len(maps)
    out = np.zeros((len(src),) + maps.shape[1:3] + src.shape[3:], np.uint8)
    for f in range(len(src)):
        i = f % n if index is None else int(index[f])
        if 0 <= i < n:
            out[f] = remap(src[f], maps[i])
    return out


def bilinear_f64(src: np.ndarray, m: np.ndarray) -> np.ndarray:
    """The real-valued bilinear sample at (sx / 32, sy / 32), zero outside the source: what the integer form rounds half up."""
    s = src.astype(np.int64).reshape(src.shape[0], src.shape[1], -1)
    sx, sy = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    ix, iy = sx >> 5, sy >> 5
    fx, fy = ((sx & 31) / 32.0)[..., None], ((sy & 31) / 32.0)[..., None]
    top = (1 - fx) * _sample(s, iy, ix) + fx * _sample(s, iy, ix + 1)
    bot = (1 - fx) * _sample(s, iy + 1, ix) + fx * _sample(s, iy + 1, ix + 1)
    out = (1 - fy) * top + fy * bot
    return out[..., 0] if src.ndim == 2 else out


def noise(shape, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def roll_record(deg: float, K, P) -> np.ndarray:
    """A rotation about the optical axis, no distortion."""
    a = np.deg2rad(deg)
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return record(K, np.zeros(5), R, P)
