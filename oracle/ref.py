"""ctypes binding of oracle/_ref/libdcmt_ref.so: the reference's own sources, compiled by oracle/refbuild/build_ref.py
against stand-in OpenCV / Eigen headers.  Same calling shapes as oracle/oracle.py.

TEST INFRASTRUCTURE, NOT PRODUCT CODE.  The library is never built on import: where it is absent, available() is False
and tests fall back to the recorded tests/golden/reference_cases.npz.  The reference's fill loop has no iteration cap, so
never hand img_completion / interpolate_with_superpixels a frame the oracle reports as not converging.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(_HERE, "_ref", "libdcmt_ref.so")

_lib = None


def available() -> bool:
    return os.path.exists(LIB)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        L = ctypes.CDLL(LIB)
        fp = ctypes.POINTER(ctypes.c_float)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        i32p = ctypes.POINTER(ctypes.c_int32)
        i = ctypes.c_int
        L.ref_abi_version.restype = i
        assert L.ref_abi_version() == 1
        L.ref_img_completion.argtypes = [fp, fp, i, i, ctypes.c_char_p]
        L.ref_slic.argtypes = [u8p, i, i, i, i, i32p, ctypes.POINTER(ctypes.c_double), i]
        L.ref_slic.restype = i
        L.ref_interpolate_with_superpixels.argtypes = [fp, i32p, i, fp, i, i, i]
        L.ref_standin_primitive.argtypes = [i, fp, fp, i, i, u8p, i, i]
        L.ref_stereo.argtypes = [fp, u8p, u8p, fp, fp, i, i]
        for n in ("ref_evaluate_lo", "ref_evaluate_lc", "ref_evaluate_sl"):
            getattr(L, n).argtypes = [fp, fp, i, i, fp]
        for n in ("ref_img_completion", "ref_interpolate_with_superpixels", "ref_standin_primitive", "ref_stereo",
                  "ref_evaluate_lo", "ref_evaluate_lc", "ref_evaluate_sl"):
            getattr(L, n).restype = None
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _u8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _c32(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.ndim == 2 and a.size > 0
    return a


def img_completion(sparse, blur: str = "gaussian") -> np.ndarray:
    """The reference's img_completion on one frame; blur is its blur_type string ("gaussian", anything else = no blur;
    "bilateral" aborts in the stand-in)."""
    assert blur != "bilateral"
    src = _c32(sparse)
    dst = np.empty_like(src)
    lib().ref_img_completion(_fp(src), _fp(dst), src.shape[0], src.shape[1], blur.encode())
    return dst


def slic(lab_image, step: int, nc: int, return_centers: bool = False):
    """Slic::generate_superpixels: (labels int32 [rows][cols], n_centers[, centers float64 [n][5]])."""
    img = np.ascontiguousarray(lab_image, dtype=np.uint8)
    assert img.ndim == 3 and img.shape[2] == 3 and step >= 6 and nc >= 1      # below 6 its gradient probe leaves the image
    rows, cols = img.shape[:2]
    labels = np.empty((rows, cols), dtype=np.int32)
    cap = max(1, (cols // step + 1) * (rows // step + 1))
    centers = np.full((cap, 5), -12345.0, dtype=np.float64)
    n = lib().ref_slic(_u8(img), rows, cols, int(step), int(nc), labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                       centers.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cap)
    assert 0 <= n <= cap
    return (labels, n, centers[:n].copy()) if return_centers else (labels, n)


def interpolate_with_superpixels(sparse, labels, n_labels: int, use_superpixel: int = 1) -> np.ndarray:
    src = _c32(sparse)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    assert lab.shape == src.shape
    dst = np.empty_like(src)
    lib().ref_interpolate_with_superpixels(_fp(src), lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(n_labels), _fp(dst),
                                           src.shape[0], src.shape[1], int(use_superpixel))
    return dst


def stereo(depth, left, right):
    """The reference's stereo sequence with its hard-coded constants: (depth before the sweeps, depth after them)."""
    d = _c32(depth)
    l = np.ascontiguousarray(left, dtype=np.uint8)
    r = np.ascontiguousarray(right, dtype=np.uint8)
    assert l.shape == d.shape == r.shape
    pre, post = np.empty_like(d), np.empty_like(d)
    lib().ref_stereo(_fp(d), _u8(l), _u8(r), _fp(pre), _fp(post), d.shape[0], d.shape[1])
    return pre, post


def _evaluate(name, gt, pred, n):
    g, p = _c32(gt), _c32(pred)
    assert g.shape == p.shape
    out = np.zeros(n, dtype=np.float32)
    getattr(lib(), name)(_fp(g), _fp(p), g.shape[0], g.shape[1], _fp(out))
    return out


def evaluate_lo(gt, pred) -> np.float32:
    """lidar-only evaluate_performance: the signed mean error it calls mse."""
    return _evaluate("ref_evaluate_lo", gt, pred, 1)[0]


def evaluate_lc(gt, pred):
    """lidar-camera evaluate_performance: (mse = the RMSE, mae)."""
    o = _evaluate("ref_evaluate_lc", gt, pred, 2)
    return o[0], o[1]


def evaluate_sl(gt, pred):
    """stereo-lidar evaluate_performances: (mae, rmse)."""
    o = _evaluate("ref_evaluate_sl", gt, pred, 2)
    return o[0], o[1]


EVALUATE = {"lidar_only": evaluate_lo, "lidar_camera": evaluate_lc, "stereo_lidar": evaluate_sl}


def _primitive(what, a, element=None):
    src = _c32(a)
    dst = np.empty_like(src)
    el = np.ascontiguousarray(element if element is not None else np.ones((1, 1)), dtype=np.uint8)
    lib().ref_standin_primitive(what, _fp(src), _fp(dst), src.shape[0], src.shape[1], _u8(el), el.shape[0], el.shape[1])
    return dst


def standin_dilate(a, element):
    return _primitive(0, a, element)


def standin_erode(a, element):
    return _primitive(1, a, element)


def standin_median5(a):
    return _primitive(2, a)


def standin_gaussian5(a):
    return _primitive(3, a)
