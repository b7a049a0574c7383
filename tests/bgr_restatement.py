"""numpy restatement of the 8-bit BGR -> Lab and BGR -> grey conversions (dcmt_bgr_convert*), and of the
documented f64 conversions they approximate.  A helper of test_bgr_convert.py and test_gpu_bgr_convert.py: no test in here.

Pixel bytes are B, G, R.  Integer-only per pixel:
    grey  Y = (B * 3735 + G * 19235 + R * 9798 + 16384) >> 15
    Lab   R' = gamma[R] ...;  fX = cbrt[D(R' * C00 + G' * C01 + B' * C02, 12)], fY, fZ with rows 1, 2 of C;
          L = D(296 * fY - 1336934, 15);  a = D(500 * (fX - fY) + 128 * 32768, 15);  b = D(200 * (fY - fZ) + 128 * 32768, 15)
    with D(v, n) = (v + (1 << (n - 1))) >> n, an arithmetic shift."""
from __future__ import annotations

import hashlib

import numpy as np

M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], dtype=np.float64)
W = np.array([0.950456, 1.0, 1.088754], dtype=np.float64)


def _lin(v):
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


def _f(t):
    return np.where(t < 0.008856, 7.787 * t + 16.0 / 116.0, np.cbrt(t))


def gamma_table() -> np.ndarray:
    return np.floor(2040.0 * _lin(np.arange(256, dtype=np.float64) / 255.0) + 0.5).astype(np.uint16)


def cbrt_table() -> np.ndarray:
    return np.floor(32768.0 * _f(np.arange(3072, dtype=np.float64) / 2040.0) + 0.5).astype(np.uint16)


def coefficients() -> np.ndarray:
    return np.rint(4096.0 * M / W[:, None]).astype(np.int32)


GAMMA, CBRT, C = gamma_table(), cbrt_table(), coefficients()


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _d(v, n):
    return (v + (1 << (n - 1))) >> n


def lab_indices(bgr: np.ndarray) -> np.ndarray:
    """The three cbrt indices of every pixel, int32 [..., 3] (X, Y, Z)."""
    lin = GAMMA.astype(np.int32)[np.asarray(bgr, dtype=np.uint8)]                 # [..., 3] as B', G', R'
    b, g, r = lin[..., 0], lin[..., 1], lin[..., 2]
    return np.stack([_d(r * C[k, 0] + g * C[k, 1] + b * C[k, 2], 12) for k in range(3)], axis=-1)


def bgr_to_lab_wide(bgr: np.ndarray, indices: np.ndarray | None = None) -> np.ndarray:
    """L, a, b as int32 [..., 3], before they are stored as bytes (indices: lab_indices(bgr) where the caller has them)."""
    f = CBRT.astype(np.int32)[lab_indices(bgr) if indices is None else indices]
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    return np.stack([_d(296 * fy - 1336934, 15), _d(500 * (fx - fy) + 128 * 32768, 15), _d(200 * (fy - fz) + 128 * 32768, 15)], axis=-1)


def bgr_to_lab(bgr: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] B, G, R -> uint8 [..., 3] L, a, b."""
    wide = bgr_to_lab_wide(bgr)
    assert wide.min() >= 0 and wide.max() <= 255            # no saturation is ever needed (test_bgr_convert.py proves it over the cube)
    return wide.astype(np.uint8)


def bgr_to_gray(bgr: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] B, G, R -> uint8 [...]."""
    p = np.asarray(bgr, dtype=np.uint8).astype(np.int32)
    return ((p[..., 0] * 3735 + p[..., 1] * 19235 + p[..., 2] * 9798 + 16384) >> 15).astype(np.uint8)


def colour_cube(first: int = 0, count: int = 1 << 24) -> np.ndarray:
    """Pixels k = first .. first + count - 1 of the cube: B = k & 255, G = (k >> 8) & 255, R = k >> 16; uint8 [count][3]."""
    k = np.arange(first, first + count, dtype=np.uint32)
    return np.stack([k & 255, (k >> 8) & 255, k >> 16], axis=-1).astype(np.uint8)


def documented_lab(bgr: np.ndarray) -> np.ndarray:
    """The documented 8-bit conversion: CIE L*a*b* of the sRGB pixel in f64 (D65), L * 255 / 100, a + 128, b + 128, rounded to
    nearest; int32 [..., 3], not clamped."""
    lin = _lin(np.arange(256, dtype=np.float64) / 255.0)[np.asarray(bgr, dtype=np.uint8)]
    rgb = lin[..., ::-1]
    xyz = [(rgb * (M[k] / W[k])).sum(axis=-1) for k in range(3)]
    fx, fy, fz = _f(xyz[0]), _f(xyz[1]), _f(xyz[2])
    L = np.where(xyz[1] > 0.008856, 116.0 * fy - 16.0, 903.3 * xyz[1])
    return np.stack([np.rint(L * 255.0 / 100.0), np.rint(500.0 * (fx - fy) + 128.0), np.rint(200.0 * (fy - fz) + 128.0)], axis=-1).astype(np.int32)


def documented_gray(bgr: np.ndarray) -> np.ndarray:
    p = np.asarray(bgr, dtype=np.uint8).astype(np.float64)
    return np.rint(0.114 * p[..., 0] + 0.587 * p[..., 1] + 0.299 * p[..., 2]).astype(np.int32)


_cube = None
_deviation = None
_SLICE = 1 << 20


def cube_reference():
    """The restatement over the whole colour cube, computed once per process in slices of 2^20 pixels: a dict with the Lab bytes
    "lab" [2^24][3], the grey bytes "gray" [2^24] (both read-only), the extrema "lo" / "hi" of L, a, b before they are stored
    (int32 [3] each) and the largest cbrt index "max_index"."""
    global _cube
    if _cube is None:
        n = 1 << 24
        lab, gray = np.empty((n, 3), np.uint8), np.empty(n, np.uint8)
        lo, hi, max_index = np.full(3, 1 << 30), np.full(3, -(1 << 30)), 0
        for first in range(0, n, _SLICE):
            px = colour_cube(first, _SLICE)
            idx = lab_indices(px)
            max_index = max(max_index, int(idx.max()))
            wide = bgr_to_lab_wide(px, idx)
            lo, hi = np.minimum(lo, wide.min(axis=0)), np.maximum(hi, wide.max(axis=0))
            lab[first:first + _SLICE] = wide.astype(np.uint8)
            gray[first:first + _SLICE] = bgr_to_gray(px)
        lab.flags.writeable = False
        gray.flags.writeable = False
        _cube = {"lab": lab, "gray": gray, "lo": lo, "hi": hi, "max_index": max_index}
    return _cube


def cube_deviation():
    """|restatement - documented f64 conversion| over the whole cube as histograms: "lab" int64 [3][16] (L, a, b; entry d = colours
    that are off by d levels, 15 = 15 or more) and "gray" int64 [16]."""
    global _deviation
    if _deviation is None:
        cube = cube_reference()
        lab_hist, gray_hist = np.zeros((3, 16), np.int64), np.zeros(16, np.int64)
        for first in range(0, 1 << 24, _SLICE):
            px = colour_cube(first, _SLICE)
            d = np.minimum(np.abs(documented_lab(px) - cube["lab"][first:first + _SLICE].astype(np.int32)), 15)
            for k in range(3):
                lab_hist[k] += np.bincount(d[:, k], minlength=16)
            g = np.abs(documented_gray(px) - cube["gray"][first:first + _SLICE].astype(np.int32))
            gray_hist += np.bincount(np.minimum(g, 15), minlength=16)
        _deviation = {"lab": lab_hist, "gray": gray_hist}
    return _deviation
