"""Python host side of the C ABI: mirrors the reference's two entry points.

    img_completion(sparse, extr=False, blur_type="gaussian") -> dense
        reference: src/DC_lidar_only/img_completion.cpp:17-20
    interpolate_with_superpixels(labels, sparse, blur_type="gaussian", use_superpixel=1) -> dense
        reference: src/DC_lidar_camera/img_completion_lc.cpp:34-38

    evaluate_performance(gt, pred, preset) -> what the reference's evaluate_performance(s) returns
        reference: src/DC_lidar_only/main.cpp:16, src/DC_lidar_camera/main_lc.cpp:85, src/DC_stereo_lidar/main_sl.cpp:1031
    to_color_image(r_img) -> the BGR JET image the reference's toColorImage makes
        reference: src/DC_lidar_only/main.cpp:6-14
    bgr_to_lab(img) / bgr_to_gray(img) -> the 8-bit Lab / grey image cv::cvtColor makes of a camera frame
        reference: src/DC_lidar_camera/main_lc.cpp:183, src/DC_stereo_lidar/main_sl.cpp:439, :1167, :1171
    reproject_pc_colors(depth, bgr) / reproject_pc(depth) -> the ordered point cloud of a dense plane
        reference: src/DC_stereo_lidar/main_sl.cpp:924-965, :887-922
    unrectify_sol(depth_pre_optim, out_shape, R_rect) -> the plane forward-warped into the un-rectified camera's frame
        reference: src/DC_stereo_lidar/main_sl.cpp:967-1028 (its data, not its drawing and printing)
    get_initial_error(depth, left, right) -> (the photometric error map, its four counts)
        reference: src/DC_stereo_lidar/main_sl.cpp:618-712 (its data, not its drawing and printing)
    stereo_sgm(left, right) -> the int16 disparity map of a rectified grey pair, in sixteenths of a pixel (-16: none)
        reference: src/DC_stereo_lidar/main_sl.cpp:1293-1339 (cv::StereoSGBM's role and output convention; the matcher is dcmt.h's)
    filter_speckles(disp16) -> the map with its small components set to -16 (cv::filterSpeckles for CV_16S), and how many pixels changed
        reference: src/DC_stereo_lidar/main_sl.cpp:1301-1302 (speckleWindowSize, speckleRange: what StereoSGBM applies to its output)

numpy arrays go through the host entry point (dcmt_complete_f32: H2D, kernels, D2H, exact
hole-closure loop); torch CUDA tensors go through the device entry point on torch's current
stream (dcmt_complete_f32_dev: asynchronous).  PyTorch is only the owner of device memory
here.  All arithmetic happens in csrc/ (HIP); there is no CPU path.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

from . import _lib as L


EVAL_FIELDS = ("n", "sum_err", "sum_abs", "sum_sq", "n_inv", "sum_inv_abs", "sum_inv_sq")     # dcmt_eval_frame, in order
# the three reference functions: (mask mode, threshold).  LO main.cpp:19 `int tolerance = 0` over gt only; LC main_lc.cpp:88
# `int tolerance = 0.1` (truncates to 0) over gt and pred; SL main_sl.cpp:1036 `int tolerance = 2` over gt and pred
EVAL_PRESETS = {"lidar_only": ("gt", 0.0), "lidar_camera": ("both", 0.0), "stereo_lidar": ("both", 2.0)}


def _eval_mode(mode) -> int:
    if mode == "gt" or (not isinstance(mode, str) and mode == L.EVAL_GT):
        return L.EVAL_GT
    if mode == "both" or (not isinstance(mode, str) and mode == L.EVAL_BOTH):
        return L.EVAL_BOTH
    raise ValueError("mode must be 'gt' (mask gt > thresh) or 'both' (gt > thresh and pred > thresh)")


class DcmtError(RuntimeError):
    def __init__(self, status: int, what: str = ""):
        super().__init__(f"{what}: {L.strerror(status)} (status {status})")
        self.status = status


def _check(st: int, what: str) -> None:
    if st != L.OK:
        raise DcmtError(st, what)


def _rule(twin: str, nearest: bool) -> str:
    """The entry point of a scatter call under either collision rule: the reference's (the last wins) or nearest wins."""
    return L.nearest_name(twin) if nearest else twin


def _is_dev(t, dtype=None) -> bool:
    """A contiguous CUDA tensor (of that dtype)."""
    return t.is_cuda and t.is_contiguous() and (dtype is None or t.dtype == dtype)


def _brc(t, trailing: int = 0):
    """(batch, rows, cols) of a [batch][rows][cols] or [rows][cols] tensor, `trailing` more dimensions behind them."""
    shp = tuple(t.shape)[:t.dim() - trailing]
    b, r, c = shp if len(shp) == 3 else (1,) + shp
    return b, r, c


def _stream(stream, t) -> ctypes.c_void_p:
    """The hipStream_t a *_dev call enqueues on: the one given (as int), by default torch's current stream on t's device."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream(t.device).cuda_stream
    return ctypes.c_void_p(stream)


def _on_stream(stream, t):
    """What a wrapper creates its default outputs under: torch's current stream is the stream the call enqueues on, so the
    caching allocator ties the block to that stream and a fill is ordered in front of the kernels."""
    if stream is None:
        return contextlib.nullcontext()
    import torch
    return torch.cuda.stream(torch.cuda.ExternalStream(stream, device=t.device) if stream else torch.cuda.default_stream(t.device))


def _frame_f32(a) -> np.ndarray:
    """One host frame as the single-frame entry points take it: f32 [rows][cols] with unit column stride, any row stride."""
    a = np.asarray(a, dtype=np.float32)
    assert a.ndim == 2
    return a if a.strides[1] == 4 else np.ascontiguousarray(a)


def make_params(k0="as_compiled", blur_type: str = "gaussian", stop_after: int = L.STAGE_FINAL,
                max_fill_iters: int = 64, spec_fill_iters: int = 1, verbose: bool = False,
                max_depth: float = 100.0, valid_thresh: float = 0.1, force_staged: bool = False, force_fused: bool = False,
                normalize=None, extrapolate: bool = True) -> L.Params:
    """normalize=(lo, hi): min-max normalise every frame first, as cv::normalize(src, dst, lo, hi, NORM_MINMAX)
    in front of the path does in the stereo-lidar executables (SL/main_sl.cpp:370, :523).
    extrapolate=False: DCMT_FLAG_NO_EXTRAPOLATE -- no column extension and no large fills (stages 6..8 do not exist: stop_after 6..8
    is refused); the median, the blur and the final invert run on the plane the 7x7 fill left, so nothing is invented far from a
    measurement (include/dcmt.h has the definition)."""
    p = L.Params()
    L.lib().dcmt_default_params(ctypes.byref(p))
    if isinstance(k0, str):
        if k0 == "diamond":
            L.lib().dcmt_k0_diamond(p.k0)
        elif k0 != "as_compiled":
            raise ValueError("k0 must be 'as_compiled', 'diamond' or a 5x5 array")
    else:
        arr = np.asarray(k0, dtype=np.uint8).reshape(25)
        for i in range(25):
            p.k0[i] = int(arr[i])
    # the reference compares strings: "bilateral" / "gaussian" / anything else = no blur; "bilateral_clone" is this project's opt-in:
    # what the reference's in-place bilateral call computes when it is given a copy (DCMT_BLUR_BILATERAL_CLONE)
    # "gaussian_valid" is another: the Gaussian that takes its weights from the valid taps only (DCMT_BLUR_GAUSSIAN_VALID), the finish
    # for extrapolate=False, where the plain Gaussian averages the region's border pixels with the holes beside them
    p.blur = {"gaussian": L.BLUR_GAUSSIAN, "bilateral": L.BLUR_BILATERAL, "bilateral_clone": L.BLUR_BILATERAL_CLONE,
              "gaussian_valid": L.BLUR_GAUSSIAN_VALID}.get(blur_type, L.BLUR_NONE)
    p.stop_after = int(stop_after)
    p.max_fill_iters = int(max_fill_iters)
    p.spec_fill_iters = int(spec_fill_iters)
    p.verbose = int(verbose)
    p.max_depth = float(max_depth)
    p.valid_thresh = float(valid_thresh)
    p.flags = (L.FLAG_FORCE_STAGED if force_staged else 0) | (L.FLAG_FORCE_FUSED if force_fused else 0)
    if normalize is not None:
        p.flags |= L.FLAG_NORMALIZE
        p.norm_lo, p.norm_hi = float(normalize[0]), float(normalize[1])
    if not extrapolate:
        p.flags |= L.FLAG_NO_EXTRAPOLATE
    return p


# one record of a cloud (dcmt_cloud_point): 16 bytes, the layout PCL's PointXYZRGB has in a binary .pcd
CLOUD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])


def make_cloud_params(fx: float | None = None, fy: float | None = None, cx: float | None = None, cy: float | None = None) -> L.CloudParams:
    """dcmt_cloud_params: the reference's intrinsics (SL/main_sl.cpp:927-930) unless given."""
    p = L.CloudParams()
    L.lib().dcmt_default_cloud_params(ctypes.byref(p))
    for k, v in (("fx", fx), ("fy", fy), ("cx", cx), ("cy", cy)):
        if v is not None:
            setattr(p, k, float(v))
    return p


def make_reproject_params(M=None, K=None, fx: float | None = None, fy: float | None = None, cx: float | None = None,
                          cy: float | None = None) -> L.ReprojectParams:
    """dcmt_reproject_params: the reference's intrinsics and camera_mat (SL/main_sl.cpp:969-976) and M = identity unless given.
    M: 4x4 (the matrix that is APPLIED: pass the inverse of R_rect; its 4th row is ignored), K: 3x3, both row-major, rounded to f32."""
    p = L.ReprojectParams()
    L.lib().dcmt_default_reproject_params(ctypes.byref(p))
    for k, v in (("fx", fx), ("fy", fy), ("cx", cx), ("cy", cy)):
        if v is not None:
            setattr(p, k, float(v))
    if M is not None:
        p.M[:] = np.asarray(M, dtype=np.float32).reshape(16).tolist()
    if K is not None:
        p.K[:] = np.asarray(K, dtype=np.float32).reshape(9).tolist()
    return p


# ---- per-frame calibration tables of the *_calib_dev calls (include/dcmt.h): structured arrays of exactly the C layouts ----------
PROJECT_CALIB_DTYPE = np.dtype([("T", "<f4", (12,)), ("P", "<f4", (12,))])                                   # dcmt_project_calib, 96 B
PHOTO_STATS = ("valid", "matches", "nonzero", "sum_err")           # the four uint64 words of dcmt_photo_error_dev's statistics, in order


def make_photo_error_params(baseline: float | None = None, focal: float | None = None, window: int | None = None) -> L.PhotoErrorParams:
    """dcmt_photo_error_params: the reference's constants (SL/main_sl.cpp:632, :634, :638: 0.54, 959.791, 2) unless overridden."""
    p = L.PhotoErrorParams()
    L.lib().dcmt_default_photo_error_params(ctypes.byref(p))
    if baseline is not None:
        p.baseline = float(baseline)
    if focal is not None:
        p.focal = float(focal)
    if window is not None:
        p.window = int(window)
    return p


def make_sgm_params(num_disparities: int | None = None, p1: int | None = None, p2: int | None = None, uniqueness: int | None = None,
                    disp12_max_diff: int | None = None, baseline: float | None = None, focal: float | None = None,
                    max_depth: float | None = None, for_depth: bool = True) -> L.SgmParams:
    """dcmt_sgm_params: the reference's matcher (SL/main_sl.cpp:1306: 64 disparities) and this library's penalties unless overridden.
    Raises ValueError on what dcmt_sgm_dev refuses of them: num_disparities not a multiple of 16 in 16..128, p1 < 0, p1 > p2,
    p2 > 10000, uniqueness outside 0..100 and, for a call that writes the depth plane (for_depth, as the C call tests them only with a
    d_depth), a baseline, focal or max_depth that is not finite and > 0."""
    p = L.SgmParams()
    L.lib().dcmt_default_sgm_params(ctypes.byref(p))
    for name, v in (("num_disparities", num_disparities), ("p1", p1), ("p2", p2), ("uniqueness", uniqueness), ("disp12_max_diff", disp12_max_diff)):
        if v is not None:
            if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
                raise ValueError(f"{name} = {v!r} is not an int32")
            setattr(p, name, int(v))
    for name, v in (("baseline", baseline), ("focal", focal), ("max_depth", max_depth)):
        if v is not None:
            setattr(p, name, float(v))
    if p.num_disparities % 16 != 0 or not 16 <= p.num_disparities <= 128:
        raise ValueError(f"num_disparities = {p.num_disparities}: a multiple of 16 in 16..128")
    if not 0 <= p.p1 <= p.p2 <= 10000:
        raise ValueError(f"p1 = {p.p1}, p2 = {p.p2}: 0 <= p1 <= p2 <= 10000")
    if not 0 <= p.uniqueness <= 100:
        raise ValueError(f"uniqueness = {p.uniqueness}: 0..100")
    for name in ("baseline", "focal", "max_depth") if for_depth else ():
        v = getattr(p, name)
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{name} = {v!r}: finite and > 0")
    return p


def make_speckle_params(max_size: int | None = None, max_diff: int | None = None, new_val: int | None = None) -> L.SpeckleParams:
    """dcmt_speckle_params: the reference's speckle window and range (SL/main_sl.cpp:1301-1302: 200 pixels, 2 disparities = 32
    sixteenths) and dcmt_sgm_dev's "none" (-16) unless overridden.  Raises ValueError on what dcmt_filter_speckles_dev refuses of
    them: max_size < 0, max_diff outside 0..65535, new_val outside int16."""
    p = L.SpeckleParams()
    L.lib().dcmt_default_speckle_params(ctypes.byref(p))
    for name, v in (("max_size", max_size), ("max_diff", max_diff), ("new_val", new_val)):
        if v is not None:
            if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
                raise ValueError(f"{name} = {v!r} is not an int32")
            setattr(p, name, int(v))
    if p.max_size < 0:
        raise ValueError(f"max_size = {p.max_size}: >= 0")
    if not 0 <= p.max_diff <= 65535:
        raise ValueError(f"max_diff = {p.max_diff}: 0..65535")
    if not -32768 <= p.new_val <= 32767:
        raise ValueError(f"new_val = {p.new_val}: an int16")
    return p


def _speckle_kw(speckle_window, speckle_range) -> dict | None:
    """StereoSGBM's speckleWindowSize / speckleRange (whole disparities) as the fields of make_speckle_params; None: no filter."""
    if speckle_window is None and speckle_range is None:
        return None
    kw = {}
    if speckle_window is not None:
        kw["max_size"] = speckle_window
    if speckle_range is not None:
        if int(speckle_range) != speckle_range:
            raise ValueError(f"speckle_range = {speckle_range!r}: whole disparities")
        kw["max_diff"] = 16 * int(speckle_range)
    return kw if make_speckle_params(**kw).max_size > 0 else None


PLANE_FIT_DTYPE = np.dtype([("a", "<f8"), ("b", "<f8"), ("c", "<f8"), ("seen", "<u4"), ("used", "<u4"), ("wmin", "<u4"), ("wmax", "<u4"),
                            ("kind", "<u4"), ("reserved", "<u4")])     # dcmt_plane_fit, 48 bytes
PLANES_MAX_PIXELS = 1 << 21         # rows * cols of a frame dcmt_superpixel_planes_dev takes (include/dcmt.h: the bounds of its sums)


def make_planes_params(valid_thresh: float | None = None, max_depth: float | None = None, min_points: int | None = None,
                       min_extent: int | None = None, refit_tol: float | None = None, keep_returns: bool | None = None) -> L.PlanesParams:
    """dcmt_planes_params: valid_thresh 0.1, max_depth 100, min_points 3, min_extent 2, refit_tol 0 (no refit), keep_returns True unless
    overridden.  Raises ValueError on what dcmt_superpixel_planes_dev refuses of them: valid_thresh not finite or < 0.0625, max_depth
    not finite, < valid_thresh or > 16384, min_points < 3, min_extent < 1, refit_tol outside [0, 1), keep_returns no bool."""
    p = L.PlanesParams()
    L.lib().dcmt_default_planes_params(ctypes.byref(p))
    for name, v in (("valid_thresh", valid_thresh), ("max_depth", max_depth), ("refit_tol", refit_tol)):
        if v is not None:
            if not np.isfinite(np.float32(v)):
                raise ValueError(f"{name} = {v!r}: a finite float")
            setattr(p, name, float(v))
    for name, v in (("min_points", min_points), ("min_extent", min_extent)):
        if v is not None:
            if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
                raise ValueError(f"{name} = {v!r} is not an int32")
            setattr(p, name, int(v))
    if keep_returns is not None:
        if keep_returns not in (0, 1, False, True):
            raise ValueError(f"keep_returns = {keep_returns!r}: a bool")
        p.keep_returns = int(keep_returns)
    if not p.valid_thresh >= 0.0625:
        raise ValueError(f"valid_thresh = {p.valid_thresh}: >= 0.0625 (the codes stay at or below 2^20)")
    if not p.valid_thresh <= p.max_depth <= 16384.0:
        raise ValueError(f"max_depth = {p.max_depth}: valid_thresh .. 16384")
    if p.min_points < 3:
        raise ValueError(f"min_points = {p.min_points}: >= 3")
    if p.min_extent < 1:
        raise ValueError(f"min_extent = {p.min_extent}: >= 1")
    if not 0.0 <= p.refit_tol < 1.0:
        raise ValueError(f"refit_tol = {p.refit_tol}: in [0, 1)")
    return p


def superpixel_planes_max_labels(max_rows: int, max_cols: int, max_batch: int, batch: int = 1) -> int:
    """The largest n_labels superpixel_planes_dev takes for `batch` frames on a Context(device, max_rows, max_cols, max_batch):
    96 bytes of moments a label and frame in one of the context's scratch planes (dcmt_superpixel_planes_max_labels)."""
    return int(L.lib().dcmt_superpixel_planes_max_labels(int(max_rows), int(max_cols), int(max_batch), int(batch)))


def make_occlusion_params(rx: int | None = None, ry: int | None = None, inv_depth_tol: float | None = None, valid_thresh: float | None = None,
                          max_depth: float | None = None, tol_code: int | None = None) -> L.OcclusionParams:
    """dcmt_occlusion_params: rx 3, ry 6, tol_code 655 (0.01 / m), valid_thresh 0.1, max_depth 100 unless overridden.  The tolerance is
    given in inverse metres (inv_depth_tol, converted as round(65536 * tol)) or in codes (tol_code), not both.  Raises ValueError on
    what dcmt_sparse_occlusion_dev refuses of them: rx outside 0..8, ry outside 0..16, a tolerance outside 0..2^20 codes,
    valid_thresh not finite or < 0.0625, max_depth not finite, < valid_thresh or > 16384."""
    p = L.OcclusionParams()
    L.lib().dcmt_default_occlusion_params(ctypes.byref(p))
    if inv_depth_tol is not None:
        if tol_code is not None:
            raise ValueError("inv_depth_tol and tol_code: one of them")
        if not np.isfinite(np.float64(inv_depth_tol)):
            raise ValueError(f"inv_depth_tol = {inv_depth_tol!r}: a finite float")
        tol_code = int(round(65536.0 * float(inv_depth_tol)))
    for name, v in (("rx", rx), ("ry", ry), ("tol_code", tol_code)):
        if v is not None:
            if int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
                raise ValueError(f"{name} = {v!r} is not an int32")
            setattr(p, name, int(v))
    for name, v in (("valid_thresh", valid_thresh), ("max_depth", max_depth)):
        if v is not None:
            if not np.isfinite(np.float32(v)):
                raise ValueError(f"{name} = {v!r}: a finite float")
            setattr(p, name, float(v))
    if not 0 <= p.rx <= 8:
        raise ValueError(f"rx = {p.rx}: 0 .. 8")
    if not 0 <= p.ry <= 16:
        raise ValueError(f"ry = {p.ry}: 0 .. 16")
    if not 0 <= p.tol_code <= 1 << 20:
        raise ValueError(f"tol_code = {p.tol_code}: 0 .. 2^20 (inv_depth_tol 0 .. 16)")
    if not p.valid_thresh >= 0.0625:
        raise ValueError(f"valid_thresh = {p.valid_thresh}: >= 0.0625 (the codes stay at or below 2^20)")
    if not p.valid_thresh <= p.max_depth <= 16384.0:
        raise ValueError(f"max_depth = {p.max_depth}: valid_thresh .. 16384")
    return p


def make_support_params(max_radius: int | None = None, valid_thresh: float | None = None, max_depth: float | None = None) -> L.SupportParams:
    """dcmt_support_params: max_radius 9, valid_thresh 0.1, max_depth 100 unless overridden.  Raises ValueError on what
    dcmt_support_distance_dev refuses of them: max_radius outside 1..255, valid_thresh not finite or < 0.0625, max_depth not finite,
    < valid_thresh or > 16384."""
    p = L.SupportParams()
    L.lib().dcmt_default_support_params(ctypes.byref(p))
    if max_radius is not None:
        if isinstance(max_radius, bool) or int(max_radius) != max_radius or not -2 ** 31 <= int(max_radius) < 2 ** 31:
            raise ValueError(f"max_radius = {max_radius!r} is not an int32")
        p.max_radius = int(max_radius)
    for name, v in (("valid_thresh", valid_thresh), ("max_depth", max_depth)):
        if v is not None:
            if not np.isfinite(np.float32(v)):
                raise ValueError(f"{name} = {v!r}: a finite float")
            setattr(p, name, float(v))
    if not 1 <= p.max_radius <= 255:
        raise ValueError(f"max_radius = {p.max_radius}: 1 .. 255 (255^2 stays below the marker 65535)")
    if not p.valid_thresh >= 0.0625:
        raise ValueError(f"valid_thresh = {p.valid_thresh}: >= 0.0625")
    if not p.valid_thresh <= p.max_depth <= 16384.0:
        raise ValueError(f"max_depth = {p.max_depth}: valid_thresh .. 16384")
    return p


def make_normals_params(min_plane_dist: float | None = None, valid_thresh: float | None = None, max_depth: float | None = None) -> L.NormalsParams:
    """dcmt_normals_params: min_plane_dist 0.4, valid_thresh 0.1, max_depth 100 unless overridden.  Raises ValueError on what
    dcmt_depth_normals_dev refuses of them: min_plane_dist not finite or outside 0..1024, valid_thresh not finite or < 0.0625,
    max_depth not finite, < valid_thresh or > 16384."""
    p = L.NormalsParams()
    L.lib().dcmt_default_normals_params(ctypes.byref(p))
    for name, v in (("min_plane_dist", min_plane_dist), ("valid_thresh", valid_thresh), ("max_depth", max_depth)):
        if v is not None:
            if not np.isfinite(np.float32(v)):
                raise ValueError(f"{name} = {v!r}: a finite float")
            setattr(p, name, float(v))
    if not 0.0 <= p.min_plane_dist <= 1024.0:
        raise ValueError(f"min_plane_dist = {p.min_plane_dist}: 0 .. 1024")
    if not p.valid_thresh >= 0.0625:
        raise ValueError(f"valid_thresh = {p.valid_thresh}: >= 0.0625")
    if not p.valid_thresh <= p.max_depth <= 16384.0:
        raise ValueError(f"max_depth = {p.max_depth}: valid_thresh .. 16384")
    return p


def _normals_intrinsics_or_raise(fx, fy, cx, cy) -> None:
    """The bounds dcmt_depth_normals_dev puts on a dcmt_cloud_params record (scalars or arrays): fx, fy finite with
    2^-10 <= |.| <= 2^20, |cx|, |cy| <= 2^20."""
    for name, v, lo in (("fx", fx, 2.0 ** -10), ("fy", fy, 2.0 ** -10), ("cx", cx, 0.0), ("cy", cy, 0.0)):
        a = np.abs(np.atleast_1d(np.asarray(v, dtype=np.float64)))
        bad = ~(np.isfinite(a) & (a >= lo) & (a <= 2.0 ** 20))
        if bad.any():
            raise ValueError(f"{name} = {np.atleast_1d(v)[int(np.argwhere(bad)[0][0])]!r} in record {int(np.argwhere(bad)[0][0])}: finite, "
                             f"{'2^-10 <= ' if lo else ''}|{name}| <= 2^20")


JOINT_TABLES_DTYPE = np.dtype([("w_space", "<u2", (128,)), ("w_guide", "<u2", (768,))])                         # dcmt_joint_tables, 1792 B


def make_joint_params(radius: int | None = None, fill: bool | None = None, smooth: bool | None = None, min_weight: int | None = None,
                      valid_thresh: float | None = None, max_depth: float | None = None) -> L.JointParams:
    """dcmt_joint_params: radius 6, fill alone, min_weight 1, valid_thresh 0.1, max_depth 100 unless overridden.  Raises ValueError on
    what dcmt_joint_bilateral_dev refuses of them: radius outside 1..9, neither fill nor smooth, min_weight outside 1..2^32 - 1,
    valid_thresh not finite or < 0.0625, max_depth not finite, < valid_thresh or > 16384."""
    p = L.JointParams()
    L.lib().dcmt_default_joint_params(ctypes.byref(p))
    if radius is not None:
        if isinstance(radius, bool) or int(radius) != radius or not -2 ** 31 <= int(radius) < 2 ** 31:
            raise ValueError(f"radius = {radius!r} is not an int32")
        p.radius = int(radius)
    for flag, bit in ((fill, L.JOINT_FILL), (smooth, L.JOINT_SMOOTH)):
        if flag is not None:
            p.flags = (p.flags | bit) if flag else (p.flags & ~bit)
    if min_weight is not None:
        if isinstance(min_weight, bool) or int(min_weight) != min_weight or not 1 <= int(min_weight) < 2 ** 32:
            raise ValueError(f"min_weight = {min_weight!r}: 1 .. 2^32 - 1")
        p.min_weight = int(min_weight)
    for name, v in (("valid_thresh", valid_thresh), ("max_depth", max_depth)):
        if v is not None:
            if not np.isfinite(np.float32(v)):
                raise ValueError(f"{name} = {v!r}: a finite float")
            setattr(p, name, float(v))
    if not 1 <= p.radius <= 9:
        raise ValueError(f"radius = {p.radius}: 1 .. 9 (253 taps of weight 255 * 255 stay below 2^24)")
    if p.flags == 0:
        raise ValueError("neither fill nor smooth: nothing to do")
    if not p.valid_thresh >= 0.0625:
        raise ValueError(f"valid_thresh = {p.valid_thresh}: >= 0.0625")
    if not p.valid_thresh <= p.max_depth <= 16384.0:
        raise ValueError(f"max_depth = {p.max_depth}: valid_thresh .. 16384")
    return p


def make_joint_tables(radius: int = 6, sigma_space: float = 3.0, sigma_guide: float = 10.0) -> np.ndarray:
    """The weight tables of the joint bilateral filter (dcmt_make_joint_tables, as include/dcmt.h states them): one JOINT_TABLES_DTYPE
    record, w_space[d2] = rne(255 exp(-d2 / (2 sigma_space^2))) for d2 <= radius^2 and 0 beyond, w_guide[s] = rne(255 exp(-s^2 /
    (2 sigma_guide^2))), in f64.  Raises ValueError on a radius outside 1..9 and on a sigma that is not finite or not > 0.  Upload it
    once with calib_to_device; any other table of that layout is as good an input (the device uses min(entry, 255))."""
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= 9:
        raise ValueError(f"radius = {radius!r}: 1 .. 9")
    for name, v in (("sigma_space", sigma_space), ("sigma_guide", sigma_guide)):
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{name} = {v!r}: finite and > 0")
    t = L.JointTables()
    _check(L.lib().dcmt_make_joint_tables(int(radius), float(sigma_space), float(sigma_guide), ctypes.byref(t)), "dcmt_make_joint_tables")
    return np.frombuffer(bytes(t), dtype=JOINT_TABLES_DTYPE).copy()


SGM_MAX_P2_EIGHT_PATHS = 1800      # S <= 8 * (6375 + p2) must fit uint16 (include/dcmt.h, step 3)


def _check_sgm_paths(paths, p: L.SgmParams) -> int:
    """The `paths` keyword of sgm_dev / sgm / stereo_sgm: 4 or 8, and with 8 the tighter limit on p2.  Raises ValueError on what
    dcmt_sgm_paths_dev refuses of them, before any call."""
    if isinstance(paths, bool) or int(paths) != paths or int(paths) not in (4, 8):
        raise ValueError(f"paths = {paths!r}: 4 or 8")
    if int(paths) == 8 and p.p2 > SGM_MAX_P2_EIGHT_PATHS:
        raise ValueError(f"p2 = {p.p2} with paths = 8: p2 <= {SGM_MAX_P2_EIGHT_PATHS}")
    return int(paths)


SGM_GUIDE_WEIGHT = 100              # the guide's penalty min(guide_weight * |d - h|, guide_cap) (include/dcmt.h, step 2b)
SGM_GUIDE_CAP = 1000                # with the default p2 = 800 exactly the eight-path limit on p2 + guide_cap
SGM_MAX_P2 = 10000
SGM_MAX_GUIDE_WEIGHT = 10000


def _check_sgm_guide(guide_weight, guide_cap, paths: int, p: L.SgmParams) -> tuple[int, int]:
    """The guide_weight / guide_cap keywords of sgm_dev / sgm / stereo_sgm when a guide is given (without one they are not looked at).
    Raises ValueError on what dcmt_sgm_guided_dev refuses of them and of the parameters, before any call."""
    for name, v in (("guide_weight", guide_weight), ("guide_cap", guide_cap)):
        if isinstance(v, bool) or int(v) != v or not -2 ** 31 <= int(v) < 2 ** 31:
            raise ValueError(f"{name} = {v!r} is not an int32")
    w, cap = int(guide_weight), int(guide_cap)
    if not 0 <= w <= SGM_MAX_GUIDE_WEIGHT:
        raise ValueError(f"guide_weight = {w}: 0..{SGM_MAX_GUIDE_WEIGHT}")
    if cap < 0:
        raise ValueError(f"guide_cap = {cap}: >= 0")
    limit = SGM_MAX_P2_EIGHT_PATHS if paths == 8 else SGM_MAX_P2
    if p.p2 + cap > limit:
        raise ValueError(f"p2 + guide_cap = {p.p2} + {cap} with paths = {paths}: <= {limit}")
    for name in ("baseline", "focal"):                      # the hint needs them, with or without a depth plane
        v = getattr(p, name)
        if not (np.isfinite(v) and v > 0):
            raise ValueError(f"{name} = {v!r}: finite and > 0 with a guide")
    return w, cap


SGM_COSTS = {"absdiff": 0, "census": 1}     # DCMT_SGM_COST_ABSDIFF, DCMT_SGM_COST_CENSUS (include/dcmt.h, steps 1 / 2 and 1c / 2c)


def _check_sgm_cost(cost) -> int:
    """The cost keyword of sgm_dev / sgm / stereo_sgm: "absdiff" or "census", or ValueError before any call."""
    if not isinstance(cost, str) or cost not in SGM_COSTS:
        raise ValueError(f"cost = {cost!r}: one of {sorted(SGM_COSTS)}")
    return SGM_COSTS[cost]


def sgm_workspace_bytes(rows: int, cols: int, num_disparities: int = 64, frames: int = 1) -> int:
    """dcmt_sgm_workspace_bytes: the bytes of workspace that hold `frames` frames in flight (0 for sizes the call refuses)."""
    return int(L.lib().dcmt_sgm_workspace_bytes(rows, cols, num_disparities, frames))


CLOUD_CALIB_DTYPE = np.dtype([("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8")])                    # dcmt_cloud_params, 32 B
REPROJECT_CALIB_DTYPE = np.dtype({"names": ["fx", "fy", "cx", "cy", "M", "K"], "formats": ["<f8", "<f8", "<f8", "<f8", ("<f4", (16,)), ("<f4", (9,))],
                                  "offsets": [0, 8, 16, 24, 32, 96], "itemsize": 136})                      # dcmt_reproject_params
STEREO_CALIB_DTYPE = np.dtype([("baseline", "<f4"), ("focal", "<f4")])                                       # dcmt_stereo_calib, 8 B


def _finite_or_raise(what: str, a) -> None:
    bad = ~np.isfinite(np.asarray(a, dtype=np.float64))
    if bad.any():
        raise ValueError(f"{what}: a non-finite entry in record {int(np.argwhere(bad)[0][0])}")


def _nonzero_or_raise(what: str, a) -> None:
    bad = np.asarray(a) == 0
    if bad.any():
        raise ValueError(f"{what} is zero in record {int(np.argwhere(bad)[0][0])}")


def _batch_of(**arrays) -> int:
    """The number of records a make_*_calib call describes: its arguments are arrays of [b] or scalars, at least one an array."""
    shapes = {k: np.shape(v) for k, v in arrays.items()}
    try:
        shp = np.broadcast_shapes(*shapes.values())
    except ValueError:
        shp = None
    if shp is None or len(shp) != 1:
        raise ValueError(f"per-frame values must be scalars or arrays of one common length [b], at least one an array; got shapes {shapes}")
    return int(shp[0])


def _intrinsics(out, b, fx, fy, cx, cy) -> None:
    for k, v in (("fx", fx), ("fy", fy), ("cx", cx), ("cy", cy)):
        out[k] = np.broadcast_to(np.asarray(v, dtype=np.float64), (b,))
        _finite_or_raise(k, out[k])
    _nonzero_or_raise("fx", out["fx"])
    _nonzero_or_raise("fy", out["fy"])


def make_project_calib(T, P) -> np.ndarray:
    """The table of Context.project_points_calib_dev: T [b][4][4] (or [b][3][4]: the bottom row is never used), P [b][3][4], both
    row-major, rounded to f32.  Raises ValueError on a non-finite entry -- a record the device call would answer with an empty
    frame.  Upload it once, outside the hot loop (calib_to_device)."""
    T, P = np.asarray(T, dtype=np.float32), np.asarray(P, dtype=np.float32)
    b = T.shape[0]
    assert T.shape in ((b, 4, 4), (b, 3, 4)) and P.shape == (b, 3, 4), (T.shape, P.shape)
    out = np.zeros(b, PROJECT_CALIB_DTYPE)
    out["T"], out["P"] = T[:, :3].reshape(b, 12), P.reshape(b, 12)
    _finite_or_raise("T", out["T"])
    _finite_or_raise("P", out["P"])
    return out


def make_cloud_calib(fx, fy, cx, cy) -> np.ndarray:
    """The table of Context.depth_to_cloud_calib_dev: per-frame intrinsics, arrays of [b] (a scalar is repeated; at least one
    must be an array).  Raises ValueError on a non-finite entry and on fx or fy zero, what dcmt_depth_to_cloud_dev refuses."""
    out = np.zeros(_batch_of(fx=fx, fy=fy, cx=cx, cy=cy), CLOUD_CALIB_DTYPE)
    _intrinsics(out, len(out), fx, fy, cx, cy)
    return out


def make_normals_calib(fx, fy, cx, cy) -> np.ndarray:
    """The table of Context.depth_normals_calib_dev: make_cloud_calib's table (the one depth_to_cloud_calib_dev takes), refused with
    ValueError where dcmt_depth_normals_dev refuses a record: fx, fy outside 2^-10 <= |.| <= 2^20, |cx| or |cy| above 2^20."""
    out = make_cloud_calib(fx, fy, cx, cy)
    _normals_intrinsics_or_raise(out["fx"], out["fy"], out["cx"], out["cy"])
    return out


def make_reproject_calib(M, K, fx, fy, cx, cy) -> np.ndarray:
    """The table of Context.reproject_depth_calib_dev: M [b][4][4] (the matrix that is APPLIED; its 4th row is ignored), K [b][3][3]
    (its 3rd row is ignored), row-major, rounded to f32; fx, fy, cx, cy arrays of [b] or scalars.  Raises ValueError on what
    dcmt_reproject_depth_dev refuses: a non-finite intrinsic or entry of the rows that are read, fx or fy zero."""
    M, K = np.asarray(M, dtype=np.float32), np.asarray(K, dtype=np.float32)
    b = M.shape[0]
    assert M.shape == (b, 4, 4) and K.shape == (b, 3, 3), (M.shape, K.shape)
    out = np.zeros(b, REPROJECT_CALIB_DTYPE)
    _intrinsics(out, b, fx, fy, cx, cy)
    out["M"], out["K"] = M.reshape(b, 16), K.reshape(b, 9)
    _finite_or_raise("M", out["M"][:, :12])
    _finite_or_raise("K", out["K"][:, :6])
    return out


def make_stereo_calib(baseline, focal) -> np.ndarray:
    """The table of Context.stereo_refine_calib_dev: per-frame baseline and focal length, arrays of [b] (a scalar is repeated; at
    least one must be an array).  Raises ValueError on a non-finite entry and on focal zero."""
    out = np.zeros(_batch_of(baseline=baseline, focal=focal), STEREO_CALIB_DTYPE)
    for k, v in (("baseline", baseline), ("focal", focal)):
        out[k] = np.broadcast_to(np.asarray(v, dtype=np.float32), (len(out),))
        _finite_or_raise(k, out[k])
    _nonzero_or_raise("focal", out["focal"])
    return out


RECTIFY_CALIB_DTYPE = np.dtype([("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"), ("k1", "<f8"), ("k2", "<f8"), ("p1", "<f8"),
                                ("p2", "<f8"), ("k3", "<f8"), ("R", "<f8", (9,)), ("fxp", "<f8"), ("fyp", "<f8"), ("cxp", "<f8"),
                                ("cyp", "<f8")])                                                             # dcmt_rectify_calib, 176 B


def make_rectify_calib(K, D, R, P, device="cuda"):
    """The table of Context.rectify_map_dev: one record per camera out of what calib_cam_to_cam.txt gives -- K [3][3] the distorted
    camera, D [5] = k1 k2 p1 p2 k3, R [3][3] the rectifying rotation (R_rect), P [3][3] or [3][4] the new camera (P_rect: its left
    3 x 3 is used) --, each one entry or a [b] stack (a single entry is repeated).  Raises ValueError for what the device answers with
    an all-outside map: a non-finite entry, fxp or fyp zero.  Returns the table on the device (calib_to_device: one synchronous
    upload, outside the hot loop); device=None returns the numpy table instead."""
    K, D, R, P = (np.asarray(a, dtype=np.float64) for a in (K, D, R, P))
    if K.shape[-2:] != (3, 3) or D.shape[-1:] != (5,) or R.shape[-2:] != (3, 3) or P.shape[-2:] not in ((3, 3), (3, 4)):
        raise ValueError(f"K [3][3], D [5], R [3][3], P [3][3] or [3][4], each alone or stacked [b]; got {K.shape}, {D.shape}, {R.shape}, {P.shape}")
    stacks = [a.shape[0] for a, nd in ((K, 2), (D, 1), (R, 2), (P, 2)) if a.ndim == nd + 1]
    if any(a.ndim not in (nd, nd + 1) for a, nd in ((K, 2), (D, 1), (R, 2), (P, 2))) or len(set(stacks)) > 1:
        raise ValueError(f"stacks of one common length [b]; got {K.shape}, {D.shape}, {R.shape}, {P.shape}")
    b = stacks[0] if stacks else 1
    K, R, P = (np.broadcast_to(a, (b,) + a.shape[-2:]) for a in (K, R, P))
    D = np.broadcast_to(D, (b, 5))
    out = np.zeros(b, RECTIFY_CALIB_DTYPE)
    out["fx"], out["fy"], out["cx"], out["cy"] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]
    for i, k in enumerate(("k1", "k2", "p1", "p2", "k3")):
        out[k] = D[:, i]
    out["R"] = R.reshape(b, 9)
    out["fxp"], out["fyp"], out["cxp"], out["cyp"] = P[:, 0, 0], P[:, 1, 1], P[:, 0, 2], P[:, 1, 2]
    for k in RECTIFY_CALIB_DTYPE.names:
        _finite_or_raise(k, out[k])
    _nonzero_or_raise("fxp", out["fxp"])
    _nonzero_or_raise("fyp", out["fyp"])
    return out if device is None else calib_to_device(out, device)


CROP_SRC_DTYPE = np.dtype([("offset", "<u8"), ("row_stride", "<u4"), ("rows", "<i4"), ("cols", "<i4"), ("x0", "<i4"), ("y0", "<i4"),
                           ("reserved", "<u4")])                                                              # dcmt_crop_src, 32 B


def kitti_crop_origin(rows: int, cols: int, out_rows: int = 352, out_cols: int = 1216):
    """(y0, x0) of the bottom-centre out_rows x out_cols window of a rows x cols frame, the cut the KITTI depth benchmark's cropped
    sets are made with AS THIS PROJECT STATES IT: y0 = rows - out_rows, x0 = (cols - out_cols) // 2.  What a crop table holds is
    explicit origins; this is only their default."""
    return rows - out_rows, (cols - out_cols) // 2


def pack_ragged(frames):
    """Frames of several sizes, [rows][cols] or [rows][cols][3] arrays of one dtype, packed back to back into one flat uint8 array:
    (bytes, shapes [(rows, cols)], offsets in bytes) -- what make_crop_table's defaults describe."""
    frames = [np.ascontiguousarray(f) for f in frames]
    assert frames and all(f.ndim in (2, 3) and f.dtype == frames[0].dtype and f.shape[2:] == frames[0].shape[2:] for f in frames)
    sizes = [f.nbytes for f in frames]
    offsets = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
    flat = np.concatenate([f.reshape(-1).view(np.uint8) for f in frames])
    return flat, [tuple(f.shape[:2]) for f in frames], offsets


def make_crop_table(shapes, out_shape, elem_bytes: int, offsets=None, row_strides=None, origins=None, src_bytes: int | None = None) -> np.ndarray:
    """The table of Context.crop_frames_dev: one dcmt_crop_src record per frame.  shapes: [(rows, cols)] of the source frames;
    out_shape: (out_rows, out_cols) of the window; elem_bytes: 1..4.  Defaults: frames packed back to back from byte 0 (offsets),
    tight rows (row_strides = cols * elem_bytes), origins [(y0, x0)] from kitti_crop_origin.  Raises ValueError on what the device
    call would answer with a zero frame: a size below 1, a negative origin, a window that leaves its frame, a stride shorter than a
    row and -- where src_bytes, the size of the source buffer, is given -- a frame that leaves the buffer.  Upload it with
    calib_to_device."""
    out_rows, out_cols = (int(v) for v in out_shape)
    if elem_bytes not in (1, 2, 3, 4) or out_rows < 1 or out_cols < 1:
        raise ValueError(f"elem_bytes must be 1..4 and the window at least 1 x 1; got {elem_bytes}, {out_rows} x {out_cols}")
    shapes = [(int(r), int(c)) for r, c in shapes]
    b = len(shapes)
    if row_strides is None:
        row_strides = [c * elem_bytes for _, c in shapes]
    if offsets is None:
        offsets, at = [], 0
        for (r, _), st in zip(shapes, row_strides):
            offsets.append(at)
            at += max(r, 0) * int(st)
    if origins is None:
        origins = [kitti_crop_origin(r, c, out_rows, out_cols) for r, c in shapes]
    if not (len(offsets) == len(row_strides) == len(origins) == b):
        raise ValueError("shapes, offsets, row_strides and origins must have one entry per frame")
    out = np.zeros(b, CROP_SRC_DTYPE)
    for f, ((r, c), off, st, (y0, x0)) in enumerate(zip(shapes, offsets, row_strides, origins)):
        off, st, y0, x0 = int(off), int(st), int(y0), int(x0)
        if r < 1 or c < 1 or r > 0x7fffffff or c > 0x7fffffff:
            raise ValueError(f"frame {f}: rows and cols must be 1 .. 2^31 - 1; got {r} x {c}")
        if x0 < 0 or y0 < 0:
            raise ValueError(f"frame {f}: a negative origin ({y0}, {x0})")
        if x0 + out_cols > c or y0 + out_rows > r:
            raise ValueError(f"frame {f}: the {out_rows} x {out_cols} window at ({y0}, {x0}) leaves the {r} x {c} frame")
        if st < c * elem_bytes or st > 0xffffffff:
            raise ValueError(f"frame {f}: row_stride {st} is not in {c * elem_bytes} .. 2^32 - 1")
        if off < 0 or off >= 1 << 64:
            raise ValueError(f"frame {f}: offset {off}")
        if src_bytes is not None and off + (r - 1) * st + c * elem_bytes > src_bytes:
            raise ValueError(f"frame {f}: ends at byte {off + (r - 1) * st + c * elem_bytes} of a source of {src_bytes}")
        out[f] = (off, st, r, c, x0, y0, 0)
    return out


def calib_to_device(table: np.ndarray, device="cuda"):
    """A make_*_calib array as the CUDA tensor the *_calib_dev wrappers take: uint8 [b][record bytes] (torch has no structured
    dtype).  One synchronous upload: do it outside the hot loop."""
    import torch
    t = np.ascontiguousarray(table)
    return torch.from_numpy(t.view(np.uint8).reshape(len(t), t.dtype.itemsize)).to(device)


def _table_ptr(d_table, batch: int, rec: int) -> int:
    """The device address of a calibration table: a contiguous CUDA tensor of any dtype that holds exactly batch records."""
    assert _is_dev(d_table) and d_table.numel() * d_table.element_size() == batch * rec, (tuple(d_table.shape), d_table.dtype, batch, rec)
    return d_table.data_ptr()


def inverse_f32(R_rect) -> np.ndarray:
    """What unrectify_sol passes as M: the inverse of the 4x4 R_rect computed in f64 (numpy.linalg.inv) and rounded once to f32.
    This inverse is OURS: the reference calls Eigen's f32 Matrix4f::inverse() inside its loop, whose bits are not reproduced."""
    return np.linalg.inv(np.asarray(R_rect, dtype=np.float64).reshape(4, 4)).astype(np.float32)


class Context:
    """One dcmt_ctx: bound to one GPU, owns the device scratch.  Not thread-safe."""

    def __init__(self, device: int = 0, max_rows: int = 352, max_cols: int = 1216, max_batch: int = 1):
        self._h = ctypes.c_void_p()
        self.device, self.max_rows, self.max_cols, self.max_batch = device, max_rows, max_cols, max_batch
        st = L.lib().dcmt_create(device, max_rows, max_cols, max_batch, ctypes.byref(self._h))
        _check(st, "dcmt_create")

    def close(self):
        if self._h:
            L.lib().dcmt_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- host arrays ------------------------------------------------------------
    def complete(self, sparse: np.ndarray, params: L.Params | None = None, labels: np.ndarray | None = None,
                 n_labels: int = 0, use_superpixel: int = 1, allow_not_converged: bool = False) -> np.ndarray:
        """sparse: f32 [rows][cols] or [batch][rows][cols] (any row stride); returns a new array."""
        p = params or make_params()
        src = np.asarray(sparse, dtype=np.float32)
        single = src.ndim == 2
        if single:
            src = src[None]
        if src.ndim != 3 or src.strides[2] != 4:
            src = np.ascontiguousarray(src)
        b, r, c = src.shape
        dst = np.empty((b, r, c), dtype=np.float32)
        if labels is None:
            st = L.lib().dcmt_complete_f32(self._h, src.ctypes.data, src.strides[1], src.strides[0],
                                           dst.ctypes.data, dst.strides[1], dst.strides[0], r, c, b, ctypes.byref(p))
        else:
            lab = np.ascontiguousarray(np.asarray(labels, dtype=np.int32).reshape(b, r, c))
            st = L.lib().dcmt_complete_labeled_f32(self._h, src.ctypes.data, src.strides[1], src.strides[0],
                                                   lab.ctypes.data, lab.strides[1], lab.strides[0], int(n_labels),
                                                   dst.ctypes.data, dst.strides[1], dst.strides[0], r, c, b,
                                                   ctypes.byref(p), int(use_superpixel))
        if st != L.OK and not (allow_not_converged and st == L.E_NOT_CONVERGED):
            raise DcmtError(st, "dcmt_complete_f32")
        self.last_status = st
        return dst[0] if single else dst

    # ---- device tensors (torch only as the owner of device memory) ----------------
    def complete_dev(self, d_src, d_dst=None, params: L.Params | None = None, d_labels=None, n_labels: int = 0,
                     use_superpixel: int = 1, stream: int | None = None):
        """d_src/d_dst: contiguous f32 CUDA tensors [batch][rows][cols] (or [rows][cols]) on this
        context's GPU.  Enqueues on `stream` (a hipStream_t as int; default torch's current stream)
        and returns immediately.  An output that is not given is allocated (and, where it has a fill, filled) on
        that same stream."""
        import torch
        p = params or make_params()
        assert _is_dev(d_src, torch.float32)
        if d_dst is None:
            with _on_stream(stream, d_src):
                d_dst = torch.full_like(d_src, float("nan"))     # never mistake stale memory for output
        assert _is_dev(d_dst, torch.float32) and d_dst.shape == d_src.shape
        b, r, c = _brc(d_src)
        if d_labels is None:
            st = L.lib().dcmt_complete_f32_dev(self._h, d_src.data_ptr(), d_dst.data_ptr(), r, c, b, ctypes.byref(p),
                                               _stream(stream, d_src))
        else:
            assert _is_dev(d_labels, torch.int32)
            st = L.lib().dcmt_complete_labeled_f32_dev(self._h, d_src.data_ptr(), d_labels.data_ptr(), int(n_labels),
                                                       d_dst.data_ptr(), r, c, b, ctypes.byref(p), int(use_superpixel),
                                                       _stream(stream, d_src))
        _check(st, "dcmt_complete_f32_dev")
        return d_dst

    def complete_u16_dev(self, d_src16, scale: float = 1.0 / 256.0, d_dst=None, params: L.Params | None = None,
                         stream: int | None = None):
        """KITTI uint16 depth payload in (torch.uint16 or int16-viewed CUDA tensor [batch][rows][cols]), metres out:
        the reference's imread + convertTo(CV_32F, 1/256) (src/DC_lidar_only/main.cpp:75-82) fused into the first kernel.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        p = params or make_params()
        assert _is_dev(d_src16) and d_src16.element_size() == 2
        b, r, c = _brc(d_src16)
        if d_dst is None:
            with _on_stream(stream, d_src16):
                d_dst = torch.full(tuple(d_src16.shape), float("nan"), dtype=torch.float32, device=d_src16.device)
        st = L.lib().dcmt_complete_u16_dev(self._h, d_src16.data_ptr(), ctypes.c_float(scale), d_dst.data_ptr(), r, c, b,
                                           ctypes.byref(p), _stream(stream, d_src16))
        _check(st, "dcmt_complete_u16_dev")
        return d_dst

    def _project_points_dev(self, d_points, d_offsets, name, geo, rows, cols, d_sparse, stream):
        """project_points_dev / project_points_calib_dev: `name` the entry point, geo(batch) what it takes between batch and d_sparse."""
        import torch
        assert _is_dev(d_points, torch.float32) and d_points.shape[-1] == 4
        assert _is_dev(d_offsets, torch.int32)
        batch = d_offsets.numel() - 1
        n = d_points.numel() // 4
        if d_sparse is None:
            with _on_stream(stream, d_points):
                d_sparse = torch.full((batch, rows, cols), float("nan"), dtype=torch.float32, device=d_points.device)
        assert _is_dev(d_sparse, torch.float32) and tuple(d_sparse.shape) == (batch, rows, cols)
        st = getattr(L.lib(), name)(self._h, d_points.data_ptr(), d_offsets.data_ptr(), n, batch, *geo(batch), d_sparse.data_ptr(), rows, cols,
                                    _stream(stream, d_points))
        _check(st, name)
        return d_sparse

    def project_points_dev(self, d_points, d_offsets, T, P, rows: int, cols: int, d_sparse=None, stream: int | None = None,
                           nearest: bool = False):
        """N2 (SL/main_sl.cpp:478-520): velodyne points -> sparse depth images on the device.  d_points: f32 CUDA tensor
        [n][4] (x, y, z, reflectance); d_offsets: int32 CUDA tensor [batch + 1], frame f owns points
        [offsets[f], offsets[f+1]); T 4x4, P 3x4 row-major.  Returns [batch][rows][cols] f32, 0 = no point.
        A pixel several points land on keeps the last in file order (the reference's rule) or, with nearest=True, the closest: the
        smallest p.z (dcmt_project_points_nearest_dev; d_sparse must then overlap none of the inputs).
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        t = np.ascontiguousarray(T, dtype=np.float32).reshape(16)
        p = np.ascontiguousarray(P, dtype=np.float32).reshape(12)
        return self._project_points_dev(d_points, d_offsets, _rule("dcmt_project_points_dev", nearest), lambda batch: (t.ctypes.data, p.ctypes.data),
                                        rows, cols, d_sparse, stream)

    def project_points_calib_dev(self, d_points, d_offsets, d_calib, rows: int, cols: int, d_sparse=None, stream: int | None = None,
                                 nearest: bool = False):
        """project_points_dev with the matrices of each sweep's own drive (dcmt_project_points_calib_dev): d_calib is a CUDA tensor
        holding [batch] dcmt_project_calib records (make_project_calib, calib_to_device), read on the stream the call enqueues on.
        A sweep whose record has a non-finite entry gives a zero plane.  nearest: as for project_points_dev.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        return self._project_points_dev(d_points, d_offsets, _rule("dcmt_project_points_calib_dev", nearest),
                                        lambda batch: (_table_ptr(d_calib, batch, PROJECT_CALIB_DTYPE.itemsize),), rows, cols, d_sparse, stream)

    def slic_labels_dev(self, d_lab, step: int, nc: int, d_labels=None, return_centers: bool = False, stream: int | None = None):
        """N3, Slic::generate_superpixels (LC/slic.cpp:101-182) on the device.  d_lab: uint8 CUDA tensor [batch][rows][cols][3]
        (or [rows][cols][3]).  Returns (labels int32 [batch][rows][cols], n_centers[, centers float64 [batch][n][5]]).
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_lab, torch.uint8) and d_lab.shape[-1] == 3
        b, r, c = _brc(d_lab, 1)
        n = L.lib().dcmt_slic_num_centers(r, c, int(step))
        with _on_stream(stream, d_lab):
            if d_labels is None:
                d_labels = torch.full((b, r, c), -7, dtype=torch.int32, device=d_lab.device)
            d_cent = torch.empty((b, max(n, 1), 5), dtype=torch.float64, device=d_lab.device) if return_centers else None
        assert _is_dev(d_labels, torch.int32) and tuple(d_labels.shape) == (b, r, c)
        st = L.lib().dcmt_slic_labels_dev(self._h, d_lab.data_ptr(), r, c, b, int(step), int(nc), d_labels.data_ptr(),
                                          d_cent.data_ptr() if return_centers else None, _stream(stream, d_lab))
        _check(st, "dcmt_slic_labels_dev")
        return (d_labels, n, d_cent[:, :n]) if return_centers else (d_labels, n)

    def slic_connectivity_dev(self, d_labels, n_centers: int, d_out=None, d_counts=None, stream: int | None = None):
        """Slic::create_connectivity (LC/slic.cpp:186-254) on the device as include/dcmt.h states it (dcmt_slic_connectivity_dev):
        every label one 4-connected region, fragments below a quarter of a superpixel merged into a neighbour.  d_labels: int32
        CUDA tensor [batch][rows][cols] (or [rows][cols]), what slic_labels_dev returns; n_centers: its second return value.
        d_out may be d_labels (in place).  Returns (d_out, max_labels, d_counts) without synchronising: max_labels bounds every
        frame's label count and is the n_labels complete_dev takes, d_counts int32 [batch] holds the counts themselves.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_labels, torch.int32)
        b, r, c = _brc(d_labels)
        with _on_stream(stream, d_labels):
            if d_out is None:
                d_out = torch.full_like(d_labels, -7)
            if d_counts is None:
                d_counts = torch.full((b,), -7, dtype=torch.int32, device=d_labels.device)
        assert _is_dev(d_out, torch.int32) and d_out.numel() == d_labels.numel()
        assert _is_dev(d_counts, torch.int32) and d_counts.numel() == b
        st = L.lib().dcmt_slic_connectivity_dev(self._h, d_labels.data_ptr(), r, c, b, int(n_centers), d_out.data_ptr(), d_counts.data_ptr(),
                                                _stream(stream, d_labels))
        _check(st, "dcmt_slic_connectivity_dev")
        return d_out, slic_connectivity_max_labels(r, c, n_centers), d_counts

    def slic_connectivity(self, labels: np.ndarray, n_centers: int):
        """One frame of host memory (dcmt_slic_connectivity, synchronous; any row stride): (a new int32 array, its label count)."""
        a = np.asarray(labels, dtype=np.int32)
        assert a.ndim == 2
        a = a if a.strides[1] == 4 else np.ascontiguousarray(a)
        out = np.empty(a.shape, dtype=np.int32)
        count = ctypes.c_int32(-1)
        st = L.lib().dcmt_slic_connectivity(self._h, a.ctypes.data, a.strides[0], a.shape[0], a.shape[1], int(n_centers), out.ctypes.data,
                                            out.strides[0], ctypes.byref(count))
        _check(st, "dcmt_slic_connectivity")
        return out, count.value

    def slic_contours_dev(self, d_labels, d_bgr=None, colour=(0, 0, 200), d_mask=None, stream: int | None = None):
        """Slic::display_contours (LC/slic.cpp:337-384; main_lc.cpp:214) on the device as include/dcmt.h states it
        (dcmt_slic_contours_dev).  d_labels: int32 CUDA tensor [batch][rows][cols] (or [rows][cols]).  d_bgr: uint8 CUDA tensor of
        d_labels' shape + (3,), painted IN PLACE with `colour` (B, G, R; the default is the reference's CV_RGB(200,0,0)) where a pixel
        is taken; d_mask: uint8 of d_labels' shape, 255 taken / 0 not.  With neither given the mask is created.  Returns
        (d_bgr, d_mask), None for the one that was not asked for, without synchronising.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_labels, torch.int32)
        b, r, c = _brc(d_labels)
        if d_bgr is None and d_mask is None:
            with _on_stream(stream, d_labels):
                d_mask = torch.full(tuple(d_labels.shape), 0xA5, dtype=torch.uint8, device=d_labels.device)
        assert d_bgr is None or (_is_dev(d_bgr, torch.uint8) and d_bgr.numel() == 3 * b * r * c)
        assert d_mask is None or (_is_dev(d_mask, torch.uint8) and d_mask.numel() == b * r * c)
        col = (ctypes.c_uint8 * 3)(*[int(v) & 0xFF for v in colour])
        st = L.lib().dcmt_slic_contours_dev(self._h, d_labels.data_ptr(), r, c, b, None if d_bgr is None else d_bgr.data_ptr(), col,
                                            None if d_mask is None else d_mask.data_ptr(), _stream(stream, d_labels))
        _check(st, "dcmt_slic_contours_dev")
        return d_bgr, d_mask

    def slic_cluster_means_dev(self, d_labels, n_labels: int, d_bgr, d_sums=None, stream: int | None = None):
        """Slic::colour_with_cluster_means (LC/slic.cpp:392-433) on the device as include/dcmt.h states it
        (dcmt_slic_cluster_means_dev): every pixel of d_bgr (uint8, d_labels' shape + (3,), IN PLACE) whose label is in [0, n_labels)
        becomes its label's mean colour, integer division.  d_sums: int32 CUDA tensor [batch][n_labels][4] = sumB, sumG, sumR, count;
        None: not wanted; True: created.  Returns (d_bgr, d_sums) without synchronising.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_labels, torch.int32)
        b, r, c = _brc(d_labels)
        assert _is_dev(d_bgr, torch.uint8) and d_bgr.numel() == 3 * b * r * c
        if d_sums is True:
            with _on_stream(stream, d_labels):
                d_sums = torch.full((b, int(n_labels), 4), -7, dtype=torch.int32, device=d_labels.device)
        assert d_sums is None or (_is_dev(d_sums, torch.int32) and d_sums.numel() == 4 * b * int(n_labels))
        st = L.lib().dcmt_slic_cluster_means_dev(self._h, d_labels.data_ptr(), r, c, b, int(n_labels), d_bgr.data_ptr(),
                                                 None if d_sums is None else d_sums.data_ptr(), _stream(stream, d_labels))
        _check(st, "dcmt_slic_cluster_means_dev")
        return d_bgr, d_sums

    def slic_contours(self, labels: np.ndarray, image=None, colour=(0, 0, 200)):
        """One frame of host memory (dcmt_slic_contours, synchronous; any row stride): (a painted copy of `image` -- uint8
        [rows][cols][3] -- or None where no image is given, the uint8 [rows][cols] mask)."""
        a = np.asarray(labels, dtype=np.int32)
        assert a.ndim == 2
        a = a if a.strides[1] == 4 else np.ascontiguousarray(a)
        img = None if image is None else np.array(image, dtype=np.uint8, order="C")
        assert img is None or img.shape == a.shape + (3,)
        mask = np.empty(a.shape, dtype=np.uint8)
        col = (ctypes.c_uint8 * 3)(*[int(v) & 0xFF for v in colour])
        st = L.lib().dcmt_slic_contours(self._h, a.ctypes.data, a.strides[0], a.shape[0], a.shape[1], None if img is None else img.ctypes.data,
                                        0 if img is None else img.strides[0], col, mask.ctypes.data, mask.strides[0])
        _check(st, "dcmt_slic_contours")
        return img, mask

    def slic_cluster_means(self, labels: np.ndarray, image, n_labels: int):
        """One frame of host memory (dcmt_slic_cluster_means, synchronous): (the mean-coloured copy of `image`, int32
        [n_labels][4] = sumB, sumG, sumR, count)."""
        a = np.asarray(labels, dtype=np.int32)
        assert a.ndim == 2
        a = a if a.strides[1] == 4 else np.ascontiguousarray(a)
        img = np.array(image, dtype=np.uint8, order="C")
        assert img.shape == a.shape + (3,)
        sums = np.empty((max(int(n_labels), 0), 4), dtype=np.int32)
        st = L.lib().dcmt_slic_cluster_means(self._h, a.ctypes.data, a.strides[0], a.shape[0], a.shape[1], int(n_labels), img.ctypes.data,
                                             img.strides[0], sums.ctypes.data)
        _check(st, "dcmt_slic_cluster_means")
        return img, sums

    def _stereo_refine_dev(self, d_depth, d_left, d_right, d_calib, d_out, iterations, stream, kw):
        import torch
        assert _is_dev(d_depth, torch.float32)
        for t in (d_left, d_right):
            assert _is_dev(t, torch.uint8) and t.shape == d_depth.shape
        b, r, c = _brc(d_depth)
        if d_out is None:
            with _on_stream(stream, d_depth):
                d_out = torch.full_like(d_depth, float("nan"))
        sp = L.StereoParams()
        L.lib().dcmt_default_stereo_params(ctypes.byref(sp))
        for k, v in kw.items():
            assert d_calib is None or k in ("damp", "max_depth"), k
            setattr(sp, k, float(v))
        if iterations is not None:
            sp.iterations = int(iterations)
        name = "dcmt_stereo_refine_dev" if d_calib is None else "dcmt_stereo_refine_calib_dev"
        table = () if d_calib is None else (_table_ptr(d_calib, b, STEREO_CALIB_DTYPE.itemsize),)
        st = getattr(L.lib(), name)(self._h, d_depth.data_ptr(), d_left.data_ptr(), d_right.data_ptr(), d_out.data_ptr(), r, c, b, ctypes.byref(sp),
                                    *table, _stream(stream, d_depth))
        _check(st, name)
        return d_out

    def stereo_refine_dev(self, d_depth, d_left, d_right, d_out=None, iterations: int | None = None, stream: int | None = None, **kw):
        """N4 (SL/main_sl.cpp:715-885): dense depth + grey stereo pair (uint8 CUDA tensors) -> refined depth.
        kw: baseline, focal, damp, max_depth override the reference's constants.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        return self._stereo_refine_dev(d_depth, d_left, d_right, None, d_out, iterations, stream, kw)

    def stereo_refine_calib_dev(self, d_depth, d_left, d_right, d_calib, d_out=None, iterations: int | None = None, stream: int | None = None, **kw):
        """stereo_refine_dev with each frame's own baseline and focal length (dcmt_stereo_refine_calib_dev): d_calib is a CUDA tensor
        holding [batch] dcmt_stereo_calib records (make_stereo_calib, calib_to_device), read on the stream the call enqueues on.
        kw: damp, max_depth.  A frame whose record has a non-finite entry or focal zero gives a zero plane.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        assert d_calib is not None
        return self._stereo_refine_dev(d_depth, d_left, d_right, d_calib, d_out, iterations, stream, kw)

    # ---- photometric error maps (dcmt_photo_error*) ---------------------------------------
    def _photo_error_dev(self, d_depth, d_left, d_right, d_calib, d_err, d_stats, want_err, want_stats, stream, kw):
        import torch
        assert _is_dev(d_depth, torch.float32)
        for t in (d_left, d_right):
            assert _is_dev(t, torch.uint8) and t.shape == d_depth.shape
        b, r, c = _brc(d_depth)
        want_err, want_stats = want_err or d_err is not None, want_stats or d_stats is not None
        with _on_stream(stream, d_depth):
            if want_err and d_err is None:
                d_err = torch.empty(tuple(d_depth.shape), dtype=torch.uint8, device=d_depth.device)
            if want_stats and d_stats is None:
                d_stats = torch.empty((b, 4), dtype=torch.int64, device=d_depth.device)
        assert d_err is None or (_is_dev(d_err, torch.uint8) and d_err.numel() == b * r * c)
        assert d_stats is None or (_is_dev(d_stats) and d_stats.element_size() == 8 and d_stats.numel() == 4 * b)
        p = make_photo_error_params(**kw)
        e, s = d_err.data_ptr() if want_err else None, d_stats.data_ptr() if want_stats else None
        if d_calib is None:
            st = L.lib().dcmt_photo_error_dev(self._h, d_depth.data_ptr(), d_left.data_ptr(), d_right.data_ptr(), r, c, b, ctypes.byref(p), e, s,
                                              _stream(stream, d_depth))
            _check(st, "dcmt_photo_error_dev")
        else:
            st = L.lib().dcmt_photo_error_calib_dev(self._h, d_depth.data_ptr(), d_left.data_ptr(), d_right.data_ptr(), r, c, b, ctypes.byref(p),
                                                    _table_ptr(d_calib, b, STEREO_CALIB_DTYPE.itemsize), e, s, _stream(stream, d_depth))
            _check(st, "dcmt_photo_error_calib_dev")
        return (d_err, d_stats) if want_err and want_stats else d_err if want_err else d_stats

    def photo_error_dev(self, d_depth, d_left, d_right, err: bool = True, stats: bool = True, d_err=None, d_stats=None,
                        stream: int | None = None, **kw):
        """The reference's get_initial_error on the device (dcmt_photo_error_dev; SL/main_sl.cpp:618-712, its data): a dense f32 depth
        plane and a grey stereo pair (uint8 CUDA tensors of its shape, what bgr_convert_dev writes) -> the uint8 error map and / or the
        int64 CUDA tensor [batch, 4] of PHOTO_STATS (valid pixels, matches, pixels with err > 0, the sum of err), without synchronising.
        Returns (err, stats), or the one that is wanted; without err the plane is not stored.  A d_err / d_stats that is given is written
        and wanted.  kw: baseline, focal, window (1..4) override the reference's constants.
        Outputs that are not given are allocated on the stream the call enqueues on."""
        return self._photo_error_dev(d_depth, d_left, d_right, None, d_err, d_stats, err, stats, stream, kw)

    def photo_error_calib_dev(self, d_depth, d_left, d_right, d_calib, err: bool = True, stats: bool = True, d_err=None, d_stats=None,
                              stream: int | None = None, **kw):
        """photo_error_dev with each frame's own baseline and focal length (dcmt_photo_error_calib_dev): d_calib is a CUDA tensor holding
        [batch] dcmt_stereo_calib records (make_stereo_calib, calib_to_device), read on the stream the call enqueues on.  kw: window.
        A frame whose record has an entry that is not finite and > 0 gives a zero plane and zero counts."""
        assert set(kw) <= {"window"}, kw
        assert d_calib is not None
        return self._photo_error_dev(d_depth, d_left, d_right, d_calib, d_err, d_stats, err, stats, stream, kw)

    def photo_error(self, depth: np.ndarray, left: np.ndarray, right: np.ndarray, err: bool = True, stats: bool = True, **kw):
        """One frame of host memory (dcmt_photo_error, synchronous; any row stride): (uint8 [rows][cols], uint64 [4]), or the one that
        is wanted."""
        d = _frame_f32(depth)
        imgs = []
        for a in (left, right):
            a = np.asarray(a, dtype=np.uint8)
            assert a.shape == d.shape
            imgs.append(a if a.strides[1] == 1 else np.ascontiguousarray(a))
        assert err or stats
        e = np.empty(d.shape, dtype=np.uint8) if err else None
        s = np.zeros(4, dtype=np.uint64) if stats else None
        p = make_photo_error_params(**kw)
        st = L.lib().dcmt_photo_error(self._h, d.ctypes.data, d.strides[0], imgs[0].ctypes.data, imgs[0].strides[0], imgs[1].ctypes.data,
                                      imgs[1].strides[0], d.shape[0], d.shape[1], ctypes.byref(p), e.ctypes.data if err else None,
                                      e.strides[0] if err else 0, s.ctypes.data if stats else None)
        _check(st, "dcmt_photo_error")
        return (e, s) if err and stats else e if err else s

    # ---- dense stereo matching (dcmt_sgm*) --------------------------------------------------
    def sgm_dev(self, d_left, d_right, disp16: bool = True, depth: bool = False, d_disp16=None, d_depth=None, d_work=None,
                frames_in_flight: int | None = None, stream: int | None = None, speckle_window: int | None = None,
                speckle_range: int | None = None, paths: int = 4, d_guide=None, guide_weight: int = SGM_GUIDE_WEIGHT,
                guide_cap: int = SGM_GUIDE_CAP, cost: str = "absdiff", **kw):
        """Semi-global stereo matching on the device (dcmt_sgm_dev, as include/dcmt.h states it; the reference's cv::StereoSGBM block,
        SL/main_sl.cpp:1293-1339): a rectified grey pair (uint8 CUDA tensors [batch][rows][cols], what bgr_convert_dev(gray=True) writes)
        -> the int16 disparity map in sixteenths of a pixel (-16: invalid) and / or the f32 depth plane stereo_refine_dev,
        photo_error_dev, evaluate_dev and colorize_dev take, without synchronising.  Returns (disp16, depth), or the one that is wanted;
        a d_disp16 / d_depth that is given is written and wanted.  d_work: the workspace, a CUDA tensor of at least
        sgm_workspace_bytes(rows, cols, D, 1) bytes, 16-byte aligned; the batch is worked through in chunks of as many frames as it
        holds.  Without one a workspace for frames_in_flight frames (default: the batch, but no more than 1 GiB and at least one frame)
        is allocated on the stream the call enqueues on.  kw: the fields of make_sgm_params.
        paths: 4 (dcmt_sgm_dev: the two horizontal and the two vertical paths) or 8 (dcmt_sgm_paths_dev: the four diagonals as well, two
        more launches a chunk; p2 <= 1800).  Anything else, or a larger p2 with 8, raises ValueError before any call.
        d_guide: an f32 CUDA tensor of the images' shape, a depth plane in the left camera in metres with 0 where there is none (what
        project_points_dev(nearest=True) writes, or a completed plane): dcmt_sgm_guided_dev, which adds min(guide_weight * |d - h|,
        guide_cap) to the block cost of every pixel with a hint h = (int)(baseline * focal / z + 0.5) < D (include/dcmt.h, step 2b).
        guide_weight in 0..10000, guide_cap >= 0 and p2 + guide_cap <= 10000 (1800 with 8 paths), baseline and focal finite and > 0, or
        ValueError before any call; without a guide the two integers are not looked at.
        cost: "absdiff" (the calls above, as they were) or "census" (dcmt_sgm_cost_dev with DCMT_SGM_COST_CENSUS: 24-bit census codes
        and 10 * the Hamming distance over the block, steps 1c / 2c of include/dcmt.h, which a difference in exposure or gain between
        the two cameras does not disturb; with or without a guide, with either path count).  Anything else raises ValueError before
        any call.
        speckle_window, speckle_range: StereoSGBM's speckleWindowSize and speckleRange (whole disparities: max_diff = 16 *
        speckle_range; the reference's are 200 and 2).  With both None nothing changes and no further call is made; with a window > 0
        filter_speckles_dev is enqueued behind the matcher on the same stream, in place on both outputs."""
        import torch
        assert _is_dev(d_left, torch.uint8) and _is_dev(d_right, torch.uint8) and d_left.shape == d_right.shape
        b, r, c = _brc(d_left)
        want_disp, want_depth = disp16 or d_disp16 is not None, depth or d_depth is not None
        p = make_sgm_params(for_depth=want_depth, **kw)
        paths = _check_sgm_paths(paths, p)
        cost = _check_sgm_cost(cost)
        if d_guide is not None:
            assert _is_dev(d_guide, torch.float32) and d_guide.shape == d_left.shape
            guide_weight, guide_cap = _check_sgm_guide(guide_weight, guide_cap, paths, p)
        assert want_disp or want_depth
        speckle = _speckle_kw(speckle_window, speckle_range)
        asked_disp, want_disp = want_disp, want_disp or speckle is not None        # the filter works on the disparities
        one = sgm_workspace_bytes(r, c, p.num_disparities, 1)
        with _on_stream(stream, d_left):
            if want_disp and d_disp16 is None:
                d_disp16 = torch.empty(tuple(d_left.shape), dtype=torch.int16, device=d_left.device)
            if want_depth and d_depth is None:
                d_depth = torch.empty(tuple(d_left.shape), dtype=torch.float32, device=d_left.device)
            if d_work is None:
                n = frames_in_flight if frames_in_flight is not None else max(1, min(b, (1 << 30) // max(one, 1)))
                assert n >= 1
                d_work = torch.empty(min(n, b) * one, dtype=torch.uint8, device=d_left.device)
        assert d_disp16 is None or (_is_dev(d_disp16, torch.int16) and d_disp16.numel() == b * r * c)
        assert d_depth is None or (_is_dev(d_depth, torch.float32) and d_depth.numel() == b * r * c)
        assert _is_dev(d_work)
        outs = (d_disp16.data_ptr() if want_disp else None, d_depth.data_ptr() if want_depth else None, r, c, b, ctypes.byref(p))
        args = (self._h, d_left.data_ptr(), d_right.data_ptr(), *outs)
        tail = (d_work.data_ptr(), d_work.numel() * d_work.element_size(), _stream(stream, d_left))
        if cost != 0:
            guided = d_guide is not None
            _check(L.lib().dcmt_sgm_cost_dev(self._h, d_left.data_ptr(), d_right.data_ptr(), d_guide.data_ptr() if guided else None, *outs, paths,
                                             guide_weight if guided else 0, guide_cap if guided else 0, cost, *tail), "dcmt_sgm_cost_dev")
        elif d_guide is not None:
            _check(L.lib().dcmt_sgm_guided_dev(self._h, d_left.data_ptr(), d_right.data_ptr(), d_guide.data_ptr(), *outs, paths, guide_weight,
                                               guide_cap, *tail), "dcmt_sgm_guided_dev")
        elif paths == 4:
            _check(L.lib().dcmt_sgm_dev(*args, *tail), "dcmt_sgm_dev")
        else:
            _check(L.lib().dcmt_sgm_paths_dev(*args, paths, *tail), "dcmt_sgm_paths_dev")
        if speckle is not None:
            self.filter_speckles_dev(d_disp16, d_depth=d_depth if want_depth else None, d_out=d_disp16, stream=stream, **speckle)
        return (d_disp16, d_depth) if asked_disp and want_depth else d_disp16 if asked_disp else d_depth

    def sgm(self, left: np.ndarray, right: np.ndarray, disp16: bool = True, depth: bool = False, speckle_window: int | None = None,
            speckle_range: int | None = None, paths: int = 4, guide=None, guide_weight: int = SGM_GUIDE_WEIGHT,
            guide_cap: int = SGM_GUIDE_CAP, cost: str = "absdiff", **kw):
        """One pair of host memory (dcmt_sgm, synchronous; any row stride): (int16 [rows][cols], f32 [rows][cols]), or the one that is
        wanted.  speckle_window, speckle_range: as sgm_dev; the filter is a second host call (dcmt_filter_speckles), in place.
        paths: as sgm_dev (8: dcmt_sgm_paths).  guide, guide_weight, guide_cap: as sgm_dev's d_guide, an f32 [rows][cols] host plane of
        any row stride (dcmt_sgm_guided).  cost: as sgm_dev ("census": dcmt_sgm_cost)."""
        imgs = []
        for a in (left, right):
            a = np.asarray(a, dtype=np.uint8)
            assert a.ndim == 2
            imgs.append(a if a.strides[1] == 1 else np.ascontiguousarray(a))
        assert imgs[0].shape == imgs[1].shape and (disp16 or depth)
        rows, cols = imgs[0].shape
        speckle = _speckle_kw(speckle_window, speckle_range)
        asked_disp, disp16 = disp16, disp16 or speckle is not None
        d = np.empty((rows, cols), dtype=np.int16) if disp16 else None
        z = np.empty((rows, cols), dtype=np.float32) if depth else None
        p = make_sgm_params(for_depth=depth, **kw)
        paths = _check_sgm_paths(paths, p)
        cost = _check_sgm_cost(cost)
        pair = (self._h, imgs[0].ctypes.data, imgs[0].strides[0], imgs[1].ctypes.data, imgs[1].strides[0])
        outs = (rows, cols, ctypes.byref(p), d.ctypes.data if disp16 else None, d.strides[0] if disp16 else 0, z.ctypes.data if depth else None,
                z.strides[0] if depth else 0)
        args = (*pair, *outs)
        if guide is not None:
            g = np.asarray(guide, dtype=np.float32)
            assert g.shape == (rows, cols)
            g = g if g.strides[1] == 4 else np.ascontiguousarray(g)
            guide_weight, guide_cap = _check_sgm_guide(guide_weight, guide_cap, paths, p)
        if cost != 0:
            plane = (g.ctypes.data, g.strides[0], *outs, paths, guide_weight, guide_cap) if guide is not None else (None, 0, *outs, paths, 0, 0)
            _check(L.lib().dcmt_sgm_cost(*pair, *plane, cost), "dcmt_sgm_cost")
        elif guide is not None:
            _check(L.lib().dcmt_sgm_guided(*pair, g.ctypes.data, g.strides[0], *outs, paths, guide_weight, guide_cap), "dcmt_sgm_guided")
        elif paths == 4:
            _check(L.lib().dcmt_sgm(*args), "dcmt_sgm")
        else:
            _check(L.lib().dcmt_sgm_paths(*args, paths), "dcmt_sgm_paths")
        if speckle is not None:
            sp = make_speckle_params(**speckle)
            st = L.lib().dcmt_filter_speckles(self._h, d.ctypes.data, d.strides[0], d.ctypes.data, d.strides[0], z.ctypes.data if depth else None,
                                              z.strides[0] if depth else 0, rows, cols, ctypes.byref(sp), None)
            _check(st, "dcmt_filter_speckles")
        return (d, z) if asked_disp and depth else d if asked_disp else z

    # ---- the speckle filter of a disparity map (dcmt_filter_speckles*) -------------------------
    def filter_speckles_dev(self, d_disp16, d_depth=None, d_out=None, removed: bool = False, d_removed=None, stream: int | None = None, **kw):
        """cv::filterSpeckles for a 16-bit disparity map on the device (dcmt_filter_speckles_dev, as include/dcmt.h states it): every
        4-connected component of pixels != new_val under the edge relation |a - b| <= max_diff that has at most max_size pixels is
        set to new_val, without synchronising.  d_disp16: an int16 CUDA tensor [batch][rows][cols] (what sgm_dev writes); d_out: where
        the result goes (may be d_disp16 itself: in place), allocated where not given; d_depth: the f32 plane sgm_dev wrote beside
        it, set to 0 IN PLACE where the call removes a disparity.  Returns d_out, or (d_out, removed) with removed=True or a
        d_removed: the int32 CUDA tensor [batch] of the pixels changed per frame.  kw: max_size (200), max_diff (32, in sixteenths),
        new_val (-16).  Outputs that are not given are allocated on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_disp16, torch.int16)
        b, r, c = _brc(d_disp16)
        p = make_speckle_params(**kw)
        want_removed = removed or d_removed is not None
        with _on_stream(stream, d_disp16):
            if d_out is None:
                d_out = torch.empty(tuple(d_disp16.shape), dtype=torch.int16, device=d_disp16.device)
            if want_removed and d_removed is None:
                d_removed = torch.empty((b,), dtype=torch.int32, device=d_disp16.device)
        assert _is_dev(d_out, torch.int16) and d_out.numel() == b * r * c
        assert d_depth is None or (_is_dev(d_depth, torch.float32) and d_depth.numel() == b * r * c)
        assert d_removed is None or (_is_dev(d_removed) and d_removed.element_size() == 4 and d_removed.numel() == b)
        st = L.lib().dcmt_filter_speckles_dev(self._h, d_disp16.data_ptr(), d_out.data_ptr(), d_depth.data_ptr() if d_depth is not None else None,
                                              r, c, b, ctypes.byref(p), d_removed.data_ptr() if want_removed else None,
                                              _stream(stream, d_disp16))
        _check(st, "dcmt_filter_speckles_dev")
        return (d_out, d_removed) if want_removed else d_out

    def filter_speckles(self, disp16: np.ndarray, depth: np.ndarray | None = None, **kw):
        """One frame of host memory (dcmt_filter_speckles, synchronous; any row stride): (the filtered int16 plane, the number of
        pixels changed), or with a depth plane (f32 [rows][cols]) (plane, the depth with the removed pixels at 0, count).  Both are
        new arrays; the arguments are not modified."""
        d = np.asarray(disp16, dtype=np.int16)
        assert d.ndim == 2
        d = d if d.strides[1] == 2 else np.ascontiguousarray(d)
        rows, cols = d.shape
        out = np.empty((rows, cols), dtype=np.int16)
        z = None
        if depth is not None:
            z = np.array(depth, dtype=np.float32, order="C")
            assert z.shape == d.shape
        n = ctypes.c_uint32(0)
        p = make_speckle_params(**kw)
        st = L.lib().dcmt_filter_speckles(self._h, d.ctypes.data, d.strides[0], out.ctypes.data, out.strides[0], z.ctypes.data if z is not None else None,
                                          z.strides[0] if z is not None else 0, rows, cols, ctypes.byref(p), ctypes.byref(n))
        _check(st, "dcmt_filter_speckles")
        return (out, int(n.value)) if z is None else (out, z, int(n.value))

    # ---- per-superpixel plane fitting of sparse depth (dcmt_superpixel_planes*) ----------------
    def superpixel_planes_dev(self, d_depth, d_labels, n_labels: int, d_out=None, d_fits=None, stream: int | None = None, **kw):
        """One least-squares plane of inverse depth per superpixel through the returns that fall in it, painted over the label's
        pixels (dcmt_superpixel_planes_dev, as include/dcmt.h states it), without synchronising: between slic_labels_dev /
        slic_connectivity_dev and complete_dev, which then fills only what the planes left open.  d_depth: f32 CUDA tensor
        [batch][rows][cols] (or [rows][cols]), metres, 0 = no return; d_labels: int32 of the same shape; d_out: where the result goes
        (may be d_depth itself: in place), allocated where not given.  d_fits: None: not wanted; True: created; or a uint8 CUDA tensor
        of batch * n_labels * 48 bytes (PLANE_FIT_DTYPE records once on the host).  kw: the fields of make_planes_params.  Returns
        d_out, or (d_out, d_fits) where fits were asked for.  Outputs that are not given are allocated on the stream the call
        enqueues on."""
        import torch
        assert _is_dev(d_depth, torch.float32) and _is_dev(d_labels, torch.int32)
        b, r, c = _brc(d_depth)
        assert d_labels.numel() == b * r * c
        p = make_planes_params(**kw)
        want_fits = d_fits is not None
        with _on_stream(stream, d_depth):
            if d_out is None:
                d_out = torch.empty(tuple(d_depth.shape), dtype=torch.float32, device=d_depth.device)
            if d_fits is True:
                d_fits = torch.full((b, max(int(n_labels), 0), PLANE_FIT_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device=d_depth.device)
        assert _is_dev(d_out, torch.float32) and d_out.numel() == b * r * c
        assert d_fits is None or (_is_dev(d_fits, torch.uint8) and d_fits.numel() == b * int(n_labels) * PLANE_FIT_DTYPE.itemsize)
        st = L.lib().dcmt_superpixel_planes_dev(self._h, d_depth.data_ptr(), d_labels.data_ptr(), r, c, b, int(n_labels), ctypes.byref(p),
                                                d_out.data_ptr(), d_fits.data_ptr() if want_fits else None, _stream(stream, d_depth))
        _check(st, "dcmt_superpixel_planes_dev")
        return (d_out, d_fits) if want_fits else d_out

    def superpixel_planes(self, depth: np.ndarray, labels: np.ndarray, n_labels: int, **kw):
        """One frame of host memory (dcmt_superpixel_planes, synchronous; any row stride): (the painted f32 plane, the fits as a
        PLANE_FIT_DTYPE array [n_labels]).  Both are new arrays; the arguments are not modified."""
        z = np.asarray(depth, dtype=np.float32)
        a = np.asarray(labels, dtype=np.int32)
        assert z.ndim == 2 and a.shape == z.shape
        z = z if z.strides[1] == 4 else np.ascontiguousarray(z)
        a = a if a.strides[1] == 4 else np.ascontiguousarray(a)
        out = np.empty(z.shape, dtype=np.float32)
        fits = np.zeros(max(int(n_labels), 0), dtype=PLANE_FIT_DTYPE)
        p = make_planes_params(**kw)
        st = L.lib().dcmt_superpixel_planes(self._h, z.ctypes.data, z.strides[0], a.ctypes.data, a.strides[0], z.shape[0], z.shape[1], int(n_labels),
                                            ctypes.byref(p), out.ctypes.data, out.strides[0], fits.ctypes.data)
        _check(st, "dcmt_superpixel_planes")
        return out, fits

    # ---- occlusion filter of projected LiDAR returns (dcmt_sparse_occlusion*) ------------------
    def sparse_occlusion_dev(self, d_sparse, d_out=None, removed: bool = False, d_removed=None, u16: bool = False, scale: float = 1.0 / 256.0,
                             stream: int | None = None, **kw):
        """Removes from a sparse depth plane every return that a nearer return in the window (2 rx + 1) x (2 ry + 1) around it shows to
        be hidden from the camera (dcmt_sparse_occlusion_dev, as include/dcmt.h states it), without synchronising: between
        project_points_dev(nearest=True) and complete_dev, superpixel_planes_dev or sgm_dev(d_guide=...).  d_sparse: f32 CUDA tensor
        [batch][rows][cols] (or [rows][cols]), metres, 0 = no return; with u16=True the KITTI uint16 payload complete_u16_dev
        ingests (a uint16 or int16 tensor, metres = value * scale; dcmt_sparse_occlusion_u16_dev).  d_out: where the result goes (may
        be d_sparse itself: in place), allocated where not given.  Returns d_out, or (d_out, removed) with removed=True or a
        d_removed: the int32 CUDA tensor [batch] of the pixels changed per frame.  kw: the fields of make_occlusion_params.  Outputs
        that are not given are allocated on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_sparse) and (d_sparse.element_size() == 2 and not d_sparse.is_floating_point() if u16 else d_sparse.dtype == torch.float32)
        b, r, c = _brc(d_sparse)
        p = make_occlusion_params(**kw)
        want_removed = removed or d_removed is not None
        with _on_stream(stream, d_sparse):
            if d_out is None:
                d_out = torch.empty(tuple(d_sparse.shape), dtype=d_sparse.dtype, device=d_sparse.device)
            if want_removed and d_removed is None:
                d_removed = torch.empty((b,), dtype=torch.int32, device=d_sparse.device)
        assert _is_dev(d_out, d_sparse.dtype) and d_out.numel() == b * r * c
        assert d_removed is None or (_is_dev(d_removed) and d_removed.element_size() == 4 and d_removed.numel() == b)
        rem = d_removed.data_ptr() if want_removed else None
        if u16:
            st = L.lib().dcmt_sparse_occlusion_u16_dev(self._h, d_sparse.data_ptr(), float(scale), d_out.data_ptr(), r, c, b, ctypes.byref(p), rem,
                                                       _stream(stream, d_sparse))
        else:
            st = L.lib().dcmt_sparse_occlusion_dev(self._h, d_sparse.data_ptr(), d_out.data_ptr(), r, c, b, ctypes.byref(p), rem, _stream(stream, d_sparse))
        _check(st, "dcmt_sparse_occlusion_u16_dev" if u16 else "dcmt_sparse_occlusion_dev")
        return (d_out, d_removed) if want_removed else d_out

    def sparse_occlusion(self, depth: np.ndarray, **kw):
        """One frame of host memory (dcmt_sparse_occlusion, synchronous; any row stride): (the filtered f32 plane, the number of
        returns removed).  The plane is a new array; the argument is not modified."""
        z = np.asarray(depth, dtype=np.float32)
        assert z.ndim == 2
        z = z if z.strides[1] == 4 else np.ascontiguousarray(z)
        out = np.empty(z.shape, dtype=np.float32)
        n = ctypes.c_uint32(0)
        p = make_occlusion_params(**kw)
        st = L.lib().dcmt_sparse_occlusion(self._h, z.ctypes.data, z.strides[0], out.ctypes.data, out.strides[0], z.shape[0], z.shape[1], ctypes.byref(p),
                                           ctypes.byref(n))
        _check(st, "dcmt_sparse_occlusion")
        return out, int(n.value)

    # ---- distance to the nearest return and the trust mask (dcmt_support_distance*) -------------
    def support_distance_dev(self, d_sparse, d_dense=None, d_fallback=None, d_out=None, dist2: bool = False, d_dist2=None, beyond: bool = False,
                             d_beyond=None, u16: bool = False, scale: float = 1.0 / 256.0, stream: int | None = None, **kw):
        """The support map of a sparse depth plane and the trust mask of a dense one (dcmt_support_distance_dev, as include/dcmt.h
        states it), without synchronising.  d_sparse: f32 CUDA tensor [batch][rows][cols] (or [rows][cols]), metres; with u16=True the
        KITTI uint16 payload (a uint16 or int16 tensor, metres = value * scale; dcmt_support_distance_u16_dev).  With d_dense (f32, the
        same shape) the trust mask goes to d_out (may be d_dense itself: in place; allocated where not given): d_dense within
        max_radius of a return, beyond it d_fallback (f32) or +0.0.  dist2=True or a d_dist2 (any 2-byte dtype): the uint16 plane of
        squared distances, 65535 beyond max_radius; it is also what a call without d_dense produces.  beyond=True or a d_beyond
        (any 4-byte dtype, [batch]): the pixels beyond max_radius per frame, as int32.  Returns the outputs wanted in the order
        (d_out, d_dist2, d_beyond): the tensor itself where that is one, else a tuple.  kw: the fields of make_support_params.
        Outputs that are not given are allocated on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_sparse) and (d_sparse.element_size() == 2 and not d_sparse.is_floating_point() if u16 else d_sparse.dtype == torch.float32)
        b, r, c = _brc(d_sparse)
        p = make_support_params(**kw)
        if d_dense is None and (d_out is not None or d_fallback is not None):
            raise ValueError("d_out and d_fallback go with a d_dense")
        want_out = d_dense is not None
        want_dist2 = dist2 or d_dist2 is not None or not want_out
        want_beyond = beyond or d_beyond is not None
        with _on_stream(stream, d_sparse):
            if want_out and d_out is None:
                d_out = torch.empty(tuple(d_sparse.shape), dtype=torch.float32, device=d_sparse.device)
            if want_dist2 and d_dist2 is None:
                d_dist2 = torch.empty(tuple(d_sparse.shape), dtype=torch.uint16, device=d_sparse.device)
            if want_beyond and d_beyond is None:
                d_beyond = torch.empty((b,), dtype=torch.int32, device=d_sparse.device)
        for t in (d_dense, d_fallback, d_out):
            assert t is None or (_is_dev(t, torch.float32) and t.numel() == b * r * c)
        assert d_dist2 is None or (_is_dev(d_dist2) and d_dist2.element_size() == 2 and d_dist2.numel() == b * r * c)
        assert d_beyond is None or (_is_dev(d_beyond) and d_beyond.element_size() == 4 and d_beyond.numel() == b)
        ptr = lambda t: None if t is None else t.data_ptr()
        tail = (ptr(d_dense), ptr(d_fallback), ptr(d_out), ptr(d_dist2), r, c, b, ctypes.byref(p), ptr(d_beyond), _stream(stream, d_sparse))
        if u16:
            st = L.lib().dcmt_support_distance_u16_dev(self._h, d_sparse.data_ptr(), float(scale), *tail)
        else:
            st = L.lib().dcmt_support_distance_dev(self._h, d_sparse.data_ptr(), *tail)
        _check(st, "dcmt_support_distance_u16_dev" if u16 else "dcmt_support_distance_dev")
        got = tuple(t for t, w in ((d_out, want_out), (d_dist2, want_dist2), (d_beyond, want_beyond)) if w)
        return got[0] if len(got) == 1 else got

    def support_distance(self, sparse: np.ndarray, dense=None, fallback=None, **kw):
        """One frame of host memory (dcmt_support_distance, synchronous; any row stride).  Without dense: (the uint16 plane of squared
        distances to the nearest return, 65535 beyond max_radius; the number of pixels beyond it).  With dense: (the trust mask, a new
        f32 array: dense within max_radius of a return, elsewhere fallback or +0.0; that plane of distances; that count)."""
        z = _frame_f32(sparse)
        rows, cols = z.shape
        d = f = out = None
        if dense is not None:
            d = _frame_f32(dense)
            assert d.shape == z.shape
            out = np.empty(z.shape, dtype=np.float32)
        if fallback is not None:
            if dense is None:
                raise ValueError("a fallback goes with a dense plane")
            f = _frame_f32(fallback)
            assert f.shape == z.shape
        dist2 = np.empty(z.shape, dtype=np.uint16)
        n = ctypes.c_uint32(0)
        p = make_support_params(**kw)
        at = lambda a: (None, 0) if a is None else (a.ctypes.data, a.strides[0])
        st = L.lib().dcmt_support_distance(self._h, *at(z), *at(d), *at(f), *at(out), *at(dist2), rows, cols, ctypes.byref(p), ctypes.byref(n))
        _check(st, "dcmt_support_distance")
        return (dist2, int(n.value)) if out is None else (out, dist2, int(n.value))

    # ---- image-guided filling: the joint bilateral filter (dcmt_joint_bilateral*) ------------------
    def joint_bilateral_dev(self, d_depth, d_guide, d_tables, d_out=None, counts: bool = False, d_counts=None, stream: int | None = None, **kw):
        """Fill (and with smooth=True smooth) a depth plane under the guidance of a camera image (dcmt_joint_bilateral_dev, as
        include/dcmt.h states it), without synchronising.  d_depth: f32 CUDA tensor [batch][rows][cols] (or [rows][cols]), metres.
        d_guide: uint8 [batch][rows][cols] (grey) or [batch][rows][cols][3] (BGR, Lab): what bgr_convert_dev and rectify_dev write.
        d_tables: one JOINT_TABLES_DTYPE record on the device (make_joint_tables, calib_to_device).  d_out: f32, the same shape, not
        d_depth (allocated where not given).  counts=True or a d_counts (any 4-byte dtype, [batch][2]): {holes filled, holes left}
        per frame, as int32; then (d_out, d_counts) is returned, else d_out.  kw: the fields of make_joint_params.  Outputs that are
        not given are allocated on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_depth, torch.float32) and _is_dev(d_guide, torch.uint8)
        b, r, c = _brc(d_depth)
        ch = d_guide.numel() // (b * r * c)
        assert ch in (1, 3) and d_guide.numel() == b * r * c * ch and (ch == 1 or d_guide.shape[-1] == 3), tuple(d_guide.shape)
        p = make_joint_params(**kw)
        want_counts = counts or d_counts is not None
        with _on_stream(stream, d_depth):
            if d_out is None:
                d_out = torch.empty(tuple(d_depth.shape), dtype=torch.float32, device=d_depth.device)
            if want_counts and d_counts is None:
                d_counts = torch.empty((b, 2), dtype=torch.int32, device=d_depth.device)
        assert _is_dev(d_out, torch.float32) and d_out.numel() == b * r * c
        assert d_counts is None or (_is_dev(d_counts) and d_counts.element_size() == 4 and d_counts.numel() == 2 * b)
        st = L.lib().dcmt_joint_bilateral_dev(self._h, d_depth.data_ptr(), d_guide.data_ptr(), ch, _table_ptr(d_tables, 1, JOINT_TABLES_DTYPE.itemsize),
                                              d_out.data_ptr(), r, c, b, ctypes.byref(p), None if d_counts is None else d_counts.data_ptr(),
                                              _stream(stream, d_depth))
        _check(st, "dcmt_joint_bilateral_dev")
        return (d_out, d_counts) if want_counts else d_out

    def joint_bilateral(self, depth: np.ndarray, guide: np.ndarray, tables=None, **kw):
        """One frame of host memory (dcmt_joint_bilateral, synchronous; any row stride).  depth: f32 [rows][cols]; guide: uint8
        [rows][cols] or [rows][cols][3]; tables: a make_joint_tables record (by default make_joint_tables() at the call's radius).
        Returns (the filled plane, a new f32 array; holes filled; holes left).  kw: the fields of make_joint_params."""
        z = _frame_f32(depth)
        rows, cols = z.shape
        g = np.asarray(guide)
        assert g.dtype == np.uint8 and g.shape[:2] == z.shape and (g.ndim == 2 or (g.ndim == 3 and g.shape[2] in (1, 3))), (g.dtype, g.shape)
        ch = 1 if g.ndim == 2 else g.shape[2]
        if g.strides[-1] != 1 or (g.ndim == 3 and g.strides[1] != ch):
            g = np.ascontiguousarray(g)
        p = make_joint_params(**kw)
        if tables is None:
            tables = make_joint_tables(radius=p.radius)
        t = np.ascontiguousarray(tables)
        assert t.dtype == JOINT_TABLES_DTYPE and t.size == 1
        out = np.empty(z.shape, dtype=np.float32)
        n = (ctypes.c_uint32 * 2)()
        st = L.lib().dcmt_joint_bilateral(self._h, z.ctypes.data, z.strides[0], g.ctypes.data, g.strides[0], ch, t.ctypes.data, out.ctypes.data,
                                          out.strides[0], rows, cols, ctypes.byref(p), n)
        _check(st, "dcmt_joint_bilateral")
        return out, int(n[0]), int(n[1])

    # ---- surface normals and the flying-pixel filter (dcmt_depth_normals*) ------------------
    def depth_normals_dev(self, d_depth, params: L.CloudParams | None = None, normals: bool = True, d_normals=None, d_out=None, counts: bool = False,
                          d_counts=None, stream: int | None = None, filtered: bool = False, **kw):
        """The unit normal and plane distance of every pixel of a depth plane, and the flying-pixel filter (dcmt_depth_normals_dev, as
        include/dcmt.h states it), without synchronising.  d_depth: f32 CUDA tensor [batch][rows][cols] (or [rows][cols]), metres.
        params: the intrinsics (make_cloud_params; the reference's by default).  normals=True or a d_normals (f32, [..][rows][cols][4]:
        nx ny nz dist): the records.  d_out (f32, the same shape; may be d_depth itself: in place): the plane without the pixels whose
        local plane passes closer to the camera centre than min_plane_dist; with filtered=True, or with normals=False, it is allocated.
        counts=True or a d_counts (any 4-byte dtype, [batch][2]): {removed, valid pixels with no normal} per frame, as int32.  Returns
        the outputs wanted in the order (d_normals, d_out, d_counts): the tensor itself where that is one, else a tuple.  kw: the
        fields of make_normals_params.  Outputs that are not given are allocated on the stream the call enqueues on."""
        p = params or make_cloud_params()
        _normals_intrinsics_or_raise(p.fx, p.fy, p.cx, p.cy)
        return self._depth_normals_dev(d_depth, "dcmt_depth_normals_dev", lambda b: ctypes.byref(p), normals, d_normals, d_out, filtered, counts, d_counts, stream, kw)

    def depth_normals_calib_dev(self, d_depth, d_calib, normals: bool = True, d_normals=None, d_out=None, counts: bool = False, d_counts=None,
                                stream: int | None = None, filtered: bool = False, **kw):
        """depth_normals_dev with each frame's own intrinsics (dcmt_depth_normals_calib_dev): d_calib is a CUDA tensor holding [batch]
        dcmt_cloud_params records (make_normals_calib or make_cloud_calib, calib_to_device), read on the stream the call enqueues on.
        A frame whose record is outside the call's bounds gets no normals and loses no pixel: its counts are {0, its valid pixels}."""
        return self._depth_normals_dev(d_depth, "dcmt_depth_normals_calib_dev", lambda b: _table_ptr(d_calib, b, CLOUD_CALIB_DTYPE.itemsize), normals,
                                       d_normals, d_out, filtered, counts, d_counts, stream, kw)

    def _depth_normals_dev(self, d_depth, name, geo, normals, d_normals, d_out, filtered, counts, d_counts, stream, kw):
        """depth_normals_dev / depth_normals_calib_dev: `name` the entry point, geo(batch) what it takes behind batch."""
        import torch
        assert _is_dev(d_depth, torch.float32)
        b, r, c = _brc(d_depth)
        p = make_normals_params(**kw)
        want_normals = normals or d_normals is not None
        want_out = filtered or d_out is not None or not want_normals
        want_counts = counts or d_counts is not None
        with _on_stream(stream, d_depth):
            if want_normals and d_normals is None:
                d_normals = torch.empty(tuple(d_depth.shape) + (4,), dtype=torch.float32, device=d_depth.device)
            if want_out and d_out is None:
                d_out = torch.empty(tuple(d_depth.shape), dtype=torch.float32, device=d_depth.device)
            if want_counts and d_counts is None:
                d_counts = torch.empty((b, 2), dtype=torch.int32, device=d_depth.device)
        assert d_normals is None or (_is_dev(d_normals, torch.float32) and d_normals.numel() == 4 * b * r * c)
        assert d_out is None or (_is_dev(d_out, torch.float32) and d_out.numel() == b * r * c)
        assert d_counts is None or (_is_dev(d_counts) and d_counts.element_size() == 4 and d_counts.numel() == 2 * b)
        ptr = lambda t: None if t is None else t.data_ptr()
        st = getattr(L.lib(), name)(self._h, d_depth.data_ptr(), r, c, b, geo(b), ctypes.byref(p), ptr(d_normals), ptr(d_out), ptr(d_counts),
                                    _stream(stream, d_depth))
        _check(st, name)
        got = tuple(t for t, w in ((d_normals, want_normals), (d_out, want_out), (d_counts, want_counts)) if w)
        return got[0] if len(got) == 1 else got

    def depth_normals(self, depth: np.ndarray, params: L.CloudParams | None = None, normals: bool = True, filtered: bool = True, **kw):
        """One frame of host memory (dcmt_depth_normals, synchronous; any row stride): (the records, f32 [rows][cols][4] = nx ny nz
        dist, or None with normals=False; the filtered plane, a new f32 array, or None with filtered=False; the pixels removed; the
        valid pixels with no normal).  params: the intrinsics (make_cloud_params); kw: the fields of make_normals_params."""
        z = _frame_f32(depth)
        rows, cols = z.shape
        if not normals and not filtered:
            raise ValueError("normals or filtered: at least one of them")
        cp = params or make_cloud_params()
        _normals_intrinsics_or_raise(cp.fx, cp.fy, cp.cx, cp.cy)
        p = make_normals_params(**kw)
        nrm = np.empty((rows, cols, 4), dtype=np.float32) if normals else None
        out = np.empty(z.shape, dtype=np.float32) if filtered else None
        n = (ctypes.c_uint32 * 2)()
        at = lambda a: (None, 0) if a is None else (a.ctypes.data, a.strides[0])
        st = L.lib().dcmt_depth_normals(self._h, z.ctypes.data, z.strides[0], rows, cols, ctypes.byref(cp), ctypes.byref(p), *at(nrm), *at(out), n)
        _check(st, "dcmt_depth_normals")
        return nrm, out, int(n[0]), int(n[1])

    # ---- accuracy against ground truth (dcmt_evaluate*) ------------------------------
    def evaluate_dev(self, d_gt, d_pred, thresh: float = 0.0, mode="both", gt_scale: float = 1.0 / 256.0, d_out=None,
                     stream: int | None = None):
        """Per-frame sums of the reference's error terms on the device (dcmt_evaluate_dev).  d_gt, d_pred: contiguous CUDA tensors
        [batch][rows][cols] (or [rows][cols]); d_pred f32; d_gt f32, or a 2-byte type (torch.uint16 / int16 view of the KITTI
        PNG payload) that goes to dcmt_evaluate_u16_dev with gt = payload * gt_scale.  mode "gt": mask gt > thresh; "both":
        gt > thresh and pred > thresh.  Returns a float64 CUDA tensor [batch, 7] (EVAL_FIELDS) without synchronising.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_pred, torch.float32)
        assert _is_dev(d_gt) and d_gt.shape == d_pred.shape
        b, r, c = _brc(d_pred)
        if d_out is None:
            with _on_stream(stream, d_pred):
                d_out = torch.empty((b, 7), dtype=torch.float64, device=d_pred.device)
        assert _is_dev(d_out, torch.float64) and d_out.numel() == 7 * b
        m = _eval_mode(mode)
        if d_gt.element_size() == 2:
            st = L.lib().dcmt_evaluate_u16_dev(self._h, d_gt.data_ptr(), ctypes.c_float(gt_scale), d_pred.data_ptr(), r, c, b,
                                               ctypes.c_float(thresh), m, d_out.data_ptr(), _stream(stream, d_pred))
        else:
            assert d_gt.dtype == torch.float32
            st = L.lib().dcmt_evaluate_dev(self._h, d_gt.data_ptr(), d_pred.data_ptr(), r, c, b, ctypes.c_float(thresh), m,
                                           d_out.data_ptr(), _stream(stream, d_pred))
        _check(st, "dcmt_evaluate_dev")
        return d_out

    def evaluate(self, gt: np.ndarray, pred: np.ndarray, thresh: float = 0.0, mode="both") -> np.ndarray:
        """One frame of host memory (dcmt_evaluate, synchronous; any row stride): float64 [7] (EVAL_FIELDS)."""
        g, q = _frame_f32(gt), _frame_f32(pred)
        assert g.shape == q.shape
        out = L.EvalFrame()
        st = L.lib().dcmt_evaluate(self._h, g.ctypes.data, g.strides[0], q.ctypes.data, q.strides[0], g.shape[0], g.shape[1],
                                   ctypes.c_float(thresh), _eval_mode(mode), ctypes.byref(out))
        _check(st, "dcmt_evaluate")
        return np.array([getattr(out, f) for f in EVAL_FIELDS], dtype=np.float64)

    # ---- JET colourisation (dcmt_colorize*) --------------------------------------------
    def colorize_dev(self, d_src, d_bgr=None, stream: int | None = None):
        """The reference's toColorImage on the device (dcmt_colorize_dev): per frame min-max to [0, 1], * 255 to u8, JET palette.
        d_src: contiguous f32 CUDA tensor [batch][rows][cols] (or [rows][cols]).  Returns a uint8 CUDA tensor of d_src's shape + (3,),
        B, G, R per pixel, without synchronising.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_src, torch.float32)
        b, r, c = _brc(d_src)
        if d_bgr is None:
            with _on_stream(stream, d_src):
                d_bgr = torch.empty(tuple(d_src.shape) + (3,), dtype=torch.uint8, device=d_src.device)
        assert _is_dev(d_bgr, torch.uint8) and d_bgr.numel() == 3 * b * r * c
        st = L.lib().dcmt_colorize_dev(self._h, d_src.data_ptr(), r, c, b, d_bgr.data_ptr(), _stream(stream, d_src))
        _check(st, "dcmt_colorize_dev")
        return d_bgr

    def colorize(self, frame: np.ndarray) -> np.ndarray:
        """One frame of host memory (dcmt_colorize, synchronous; any row stride): uint8 [rows][cols][3], B, G, R."""
        a = _frame_f32(frame)
        out = np.empty(a.shape + (3,), dtype=np.uint8)
        st = L.lib().dcmt_colorize(self._h, a.ctypes.data, a.strides[0], a.shape[0], a.shape[1], out.ctypes.data, out.strides[0])
        _check(st, "dcmt_colorize")
        return out

    # ---- camera BGR bytes -> 8-bit Lab and grey planes (dcmt_bgr_convert*) ---------------------------------------
    def bgr_convert_dev(self, d_bgr, lab: bool = True, gray: bool = False, d_lab=None, d_gray=None, stream: int | None = None):
        """cv::cvtColor(BGR2Lab) and / or cv::cvtColor(BGR2GRAY) on the device (dcmt_bgr_convert_dev; LC/main_lc.cpp:183,
        SL/main_sl.cpp:439, :1167, :1171), one read of the image for both.  d_bgr: contiguous uint8 CUDA tensor
        [batch][rows][cols][3] (or [rows][cols][3]), B, G, R.  Returns the Lab tensor (d_bgr's shape: what slic_labels_dev takes),
        the grey tensor (d_bgr's shape without the 3: what stereo_refine_dev takes), or (lab, grey) where both are wanted, without
        synchronising.  A d_lab / d_gray that is given is written and wanted; d_lab may be d_bgr (in place).
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_bgr, torch.uint8) and d_bgr.shape[-1] == 3
        b, r, c = _brc(d_bgr, 1)
        lab, gray = lab or d_lab is not None, gray or d_gray is not None
        with _on_stream(stream, d_bgr):
            if lab and d_lab is None:
                d_lab = torch.empty_like(d_bgr)
            if gray and d_gray is None:
                d_gray = torch.empty(tuple(d_bgr.shape[:-1]), dtype=torch.uint8, device=d_bgr.device)
        assert d_lab is None or (_is_dev(d_lab, torch.uint8) and d_lab.numel() == 3 * b * r * c)
        assert d_gray is None or (_is_dev(d_gray, torch.uint8) and d_gray.numel() == b * r * c)
        st = L.lib().dcmt_bgr_convert_dev(self._h, d_bgr.data_ptr(), r, c, b, d_lab.data_ptr() if lab else None,
                                          d_gray.data_ptr() if gray else None, _stream(stream, d_bgr))
        _check(st, "dcmt_bgr_convert_dev")
        return (d_lab, d_gray) if lab and gray else d_lab if lab else d_gray

    # ---- ragged frames in, the uint16 payload out (dcmt_crop_frames_dev, dcmt_depth_to_u16*) -----------------------------
    def crop_frames_dev(self, d_src, d_table, out_rows: int, out_cols: int, elem_bytes: int | None = None, dtype=None, d_dst=None,
                        stream: int | None = None):
        """One window out of each frame of a ragged batch, into one uniform batch, in one launch (dcmt_crop_frames_dev).  d_src: a
        flat uint8 CUDA tensor or any contiguous one -- all its bytes are the source buffer; d_table: a CUDA tensor holding [batch]
        dcmt_crop_src records (make_crop_table, calib_to_device), read on the stream the call enqueues on.  The element is
        elem_bytes bytes, or dtype's, or d_src's.  Returns [batch][out_rows][out_cols] of dtype (by default uint8, uint16, uint8
        [...][3] or float32 for 1, 2, 3, 4 bytes), without synchronising; a frame whose record is bad is all zero.  d_dst: any
        contiguous CUDA tensor of exactly the output's bytes, at any byte alignment.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_src) and _is_dev(d_table)
        if dtype is None and elem_bytes is None:
            dtype = d_src.dtype
        if elem_bytes is None:
            elem_bytes = torch.empty(0, dtype=dtype).element_size()
        if dtype is None:
            dtype = {1: torch.uint8, 2: torch.uint16, 3: torch.uint8, 4: torch.float32}[elem_bytes]
        item = torch.empty(0, dtype=dtype).element_size()
        assert elem_bytes in (1, 2, 3, 4) and elem_bytes % item == 0, (elem_bytes, dtype)
        batch, rem = divmod(d_table.numel() * d_table.element_size(), CROP_SRC_DTYPE.itemsize)
        assert batch >= 1 and rem == 0, tuple(d_table.shape)
        if d_dst is None:
            shape = (batch, out_rows, out_cols) + ((elem_bytes // item,) if elem_bytes != item else ())
            with _on_stream(stream, d_src):
                d_dst = torch.empty(shape, dtype=dtype, device=d_src.device)
        assert _is_dev(d_dst) and d_dst.numel() * d_dst.element_size() == batch * out_rows * out_cols * elem_bytes
        st = L.lib().dcmt_crop_frames_dev(self._h, d_src.data_ptr(), d_src.numel() * d_src.element_size(), d_table.data_ptr(), elem_bytes,
                                          d_dst.data_ptr(), out_rows, out_cols, batch, _stream(stream, d_src))
        _check(st, "dcmt_crop_frames_dev")
        return d_dst

    def depth_to_u16_dev(self, d_depth, scale: float = 256.0, d_out=None, stream: int | None = None):
        """A dense plane as the KITTI payload (dcmt_depth_to_u16_dev): round-to-nearest-even of depth * scale, saturated to
        0..65535 -- cv::Mat::convertTo(CV_16U, scale), the inverse of complete_u16_dev's ingest.  d_depth: contiguous f32 CUDA tensor
        [batch][rows][cols] (or [rows][cols]).  Returns a torch.uint16 CUDA tensor of its shape (d_out: any 2-byte dtype), without
        synchronising.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_depth, torch.float32)
        b, r, c = _brc(d_depth)
        if d_out is None:
            with _on_stream(stream, d_depth):
                d_out = torch.empty(tuple(d_depth.shape), dtype=torch.uint16, device=d_depth.device)
        assert _is_dev(d_out) and d_out.element_size() == 2 and d_out.numel() == b * r * c
        st = L.lib().dcmt_depth_to_u16_dev(self._h, d_depth.data_ptr(), ctypes.c_float(scale), d_out.data_ptr(), r, c, b, _stream(stream, d_depth))
        _check(st, "dcmt_depth_to_u16_dev")
        return d_out

    def depth_to_u16(self, frame: np.ndarray, scale: float = 256.0) -> np.ndarray:
        """One frame of host memory (dcmt_depth_to_u16, synchronous; any row stride): uint16 [rows][cols]."""
        a = _frame_f32(frame)
        out = np.empty(a.shape, dtype=np.uint16)
        st = L.lib().dcmt_depth_to_u16(self._h, a.ctypes.data, a.strides[0], ctypes.c_float(scale), out.ctypes.data, out.strides[0],
                                       a.shape[0], a.shape[1])
        _check(st, "dcmt_depth_to_u16")
        return out

    def bgr_convert(self, frame: np.ndarray, lab: bool = True, gray: bool = False):
        """One frame of host memory (dcmt_bgr_convert, synchronous; any row stride): uint8 [rows][cols][3] B, G, R -> the Lab
        frame, the grey frame [rows][cols], or (lab, grey)."""
        a = np.asarray(frame, dtype=np.uint8)
        assert a.ndim == 3 and a.shape[2] == 3 and (lab or gray)
        if a.strides[1] != 3 or a.strides[2] != 1:
            a = np.ascontiguousarray(a)
        o_lab = np.empty(a.shape, dtype=np.uint8) if lab else None
        o_gray = np.empty(a.shape[:2], dtype=np.uint8) if gray else None
        st = L.lib().dcmt_bgr_convert(self._h, a.ctypes.data, a.strides[0], a.shape[0], a.shape[1],
                                      o_lab.ctypes.data if lab else None, o_lab.strides[0] if lab else 0,
                                      o_gray.ctypes.data if gray else None, o_gray.strides[0] if gray else 0)
        _check(st, "dcmt_bgr_convert")
        return (o_lab, o_gray) if lab and gray else o_lab if lab else o_gray

    # ---- undistortion and rectification of camera frames (dcmt_rectify*) --------------------------------------------
    def rectify_map_dev(self, d_table, rows: int, cols: int, d_map=None, stream: int | None = None):
        """The undistort-and-rectify maps of a table of cameras (dcmt_rectify_map_dev: cv::initUndistortRectifyMap as include/dcmt.h
        states it; the reference's rectify(), SL/main_sl.cpp:1350-1381).  d_table: a CUDA tensor holding [n_maps] dcmt_rectify_calib
        records (make_rectify_calib), read on the stream the call enqueues on.  Returns the int32 CUDA tensor
        [n_maps][rows][cols][2] of 1/32-pixel source positions (sx, sy), without synchronising; a bad record's map is all outside.
        Computed once per calibration.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_table)
        n_maps, rem = divmod(d_table.numel() * d_table.element_size(), RECTIFY_CALIB_DTYPE.itemsize)
        assert n_maps >= 1 and rem == 0, tuple(d_table.shape)
        if d_map is None:
            with _on_stream(stream, d_table):
                d_map = torch.empty((n_maps, rows, cols, 2), dtype=torch.int32, device=d_table.device)
        assert _is_dev(d_map, torch.int32) and d_map.numel() == n_maps * rows * cols * 2
        st = L.lib().dcmt_rectify_map_dev(self._h, d_table.data_ptr(), n_maps, rows, cols, d_map.data_ptr(), _stream(stream, d_table))
        _check(st, "dcmt_rectify_map_dev")
        return d_map

    def rectify_dev(self, d_src, d_map, out=None, d_map_index=None, force_gather: bool = False, stream: int | None = None):
        """cv::remap(..., cv::INTER_LINEAR) of a batch through rectify_map_dev's maps (dcmt_rectify_dev), in front of crop_frames_dev
        and bgr_convert_dev.  d_src: uint8 CUDA tensor [b][r][c] (grey) or [b][r][c][3], any byte alignment; d_map: int32
        [n_maps][rows][cols][2] (or [rows][cols][2]).  Frame f goes through map d_map_index[f] (an int32 CUDA tensor [b]; an index
        outside 0 .. n_maps - 1 gives a zero frame), without one through map f % n_maps: one map for the batch, two for interleaved
        left and right frames.  Returns uint8 [b][rows][cols] or [b][rows][cols][3] -- the shape comes from the map --, without
        synchronising; samples outside the source are 0.  force_gather: the global-gather route for every tile (tests, timing; the
        same bytes).  last_path() names the routes taken once the call has run.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_src, torch.uint8) and d_src.dim() in (3, 4) and (d_src.dim() == 3 or d_src.shape[3] == 3), tuple(d_src.shape)
        assert _is_dev(d_map, torch.int32) and d_map.dim() in (3, 4) and d_map.shape[-1] == 2, tuple(d_map.shape)
        b, sr, sc = d_src.shape[:3]
        ch = 1 if d_src.dim() == 3 else 3
        n_maps = 1 if d_map.dim() == 3 else d_map.shape[0]
        rows, cols = d_map.shape[-3], d_map.shape[-2]
        if out is None:
            with _on_stream(stream, d_src):
                out = torch.empty((b, rows, cols) + tuple(d_src.shape[3:]), dtype=torch.uint8, device=d_src.device)
        assert _is_dev(out, torch.uint8) and out.numel() == b * rows * cols * ch
        assert d_map_index is None or (_is_dev(d_map_index, torch.int32) and d_map_index.numel() == b)
        st = L.lib().dcmt_rectify_dev(self._h, d_src.data_ptr(), sr, sc, ch, d_map.data_ptr(), n_maps,
                                      d_map_index.data_ptr() if d_map_index is not None else None,
                                      L.RECTIFY_FORCE_GATHER if force_gather else 0, out.data_ptr(), rows, cols, b, _stream(stream, d_src))
        _check(st, "dcmt_rectify_dev")
        return out

    def rectify(self, img, K, D, R, P, out_shape):
        """One frame, undistorted and rectified: img uint8 [r][c] or [r][c][3], the camera as make_rectify_calib takes it (single
        entries), out_shape = (rows, cols).  A numpy frame goes through the host entry point (dcmt_rectify, synchronous; any row
        stride); a CUDA tensor through the two device calls, on torch's current stream, and comes back as a CUDA tensor without
        synchronising (the record's upload apart)."""
        rows, cols = out_shape
        if hasattr(img, "is_cuda") and img.is_cuda:
            d_map = self.rectify_map_dev(make_rectify_calib(K, D, R, P, device=img.device), rows, cols)
            return self.rectify_dev(img[None].contiguous(), d_map)[0]
        rec = make_rectify_calib(K, D, R, P, device=None)
        assert len(rec) == 1
        a = np.asarray(img, dtype=np.uint8)
        assert a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3), a.shape
        ch = 1 if a.ndim == 2 else 3
        if a.strides[1] != ch or (ch == 3 and a.strides[2] != 1):
            a = np.ascontiguousarray(a)
        o = np.empty((rows, cols) + a.shape[2:], dtype=np.uint8)
        st = L.lib().dcmt_rectify(self._h, a.ctypes.data, a.strides[0], a.shape[0], a.shape[1], ch, rec.ctypes.data, o.ctypes.data,
                                  o.strides[0], rows, cols)
        _check(st, "dcmt_rectify")
        return o

    # ---- point cloud of a dense plane (dcmt_depth_to_cloud*) and the blur in front of it (dcmt_gaussian5*) -----------
    def depth_to_cloud_dev(self, d_depth, d_bgr=None, params: L.CloudParams | None = None, d_points=None, d_offsets=None,
                           capacity: int | None = None, stream: int | None = None):
        """The reference's reproject_pc_colors / reproject_pc (SL/main_sl.cpp:924-965, :887-922) on the device: one record per pixel
        with depth > 0, frames in batch order, pixels row-major.  d_depth: contiguous f32 CUDA tensor [batch][rows][cols] (or
        [rows][cols]: a batch of one); d_bgr: uint8 CUDA tensor of d_depth's shape + (3,) or None (fourth dword 1.0f).
        Returns (points, offsets): points float32 [capacity, 4] (default capacity batch * rows * cols; the fourth column holds the
        colour BITS b | g << 8 | r << 16 | 255 << 24: compare and slice it through .view(torch.int32) / .view(torch.uint8)),
        offsets int32 [batch + 1]; frame f owns points[offsets[f]:offsets[f + 1]].  Rows of points from offsets[batch] on are not
        written.  No synchronisation.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        p = params or make_cloud_params()
        return self._depth_to_cloud_dev(d_depth, d_bgr, "dcmt_depth_to_cloud_dev", lambda b: (ctypes.byref(p),), d_points, d_offsets, capacity, stream)

    def _depth_to_cloud_dev(self, d_depth, d_bgr, name, geo, d_points, d_offsets, capacity, stream):
        """depth_to_cloud_dev / depth_to_cloud_calib_dev: `name` the entry point, geo(batch) what it takes between batch and d_points."""
        import torch
        assert _is_dev(d_depth, torch.float32)
        b, r, c = _brc(d_depth)
        if d_bgr is not None:
            assert _is_dev(d_bgr, torch.uint8) and d_bgr.numel() == 3 * b * r * c
        if capacity is None:
            capacity = d_points.numel() // 4 if d_points is not None else b * r * c
        with _on_stream(stream, d_depth):
            if d_points is None:
                d_points = torch.empty((capacity, 4), dtype=torch.float32, device=d_depth.device)
            if d_offsets is None:
                d_offsets = torch.empty((b + 1,), dtype=torch.int32, device=d_depth.device)
        assert _is_dev(d_points, torch.float32) and d_points.numel() >= 4 * capacity
        assert _is_dev(d_offsets, torch.int32) and d_offsets.numel() == b + 1
        st = getattr(L.lib(), name)(self._h, d_depth.data_ptr(), d_bgr.data_ptr() if d_bgr is not None else None, r, c, b, *geo(b),
                                    d_points.data_ptr(), int(capacity), d_offsets.data_ptr(), _stream(stream, d_depth))
        _check(st, name)
        return d_points, d_offsets

    def depth_to_cloud_calib_dev(self, d_depth, d_calib, d_bgr=None, d_points=None, d_offsets=None, capacity: int | None = None,
                                 stream: int | None = None):
        """depth_to_cloud_dev with each frame's own intrinsics (dcmt_depth_to_cloud_calib_dev): d_calib is a CUDA tensor holding
        [batch] dcmt_cloud_params records (make_cloud_calib, calib_to_device), read on the stream the call enqueues on.  A frame
        whose record has a non-finite entry or fx or fy zero gives no records: offsets[f + 1] == offsets[f].
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        return self._depth_to_cloud_dev(d_depth, d_bgr, "dcmt_depth_to_cloud_calib_dev", lambda b: (_table_ptr(d_calib, b, CLOUD_CALIB_DTYPE.itemsize),),
                                        d_points, d_offsets, capacity, stream)

    def depth_to_cloud(self, depth: np.ndarray, bgr: np.ndarray | None = None, params: L.CloudParams | None = None) -> np.ndarray:
        """One frame of host memory (dcmt_depth_to_cloud, synchronous; any row stride): a structured array (CLOUD_DTYPE: x y z f32,
        b g r a u8) of the true length."""
        a = _frame_f32(depth)
        rows, cols = a.shape
        col = None
        if bgr is not None:
            col = np.asarray(bgr, dtype=np.uint8)
            assert col.shape == (rows, cols, 3)
            if col.strides[1] != 3 or col.strides[2] != 1:
                col = np.ascontiguousarray(col)
        out = np.empty(rows * cols, dtype=CLOUD_DTYPE)
        n = ctypes.c_int64(0)
        p = params or make_cloud_params()
        st = L.lib().dcmt_depth_to_cloud(self._h, a.ctypes.data, a.strides[0], col.ctypes.data if col is not None else None,
                                         col.strides[0] if col is not None else 0, rows, cols, ctypes.byref(p), out.ctypes.data,
                                         out.size, ctypes.byref(n))
        _check(st, "dcmt_depth_to_cloud")
        return out[:n.value].copy()

    def gaussian5_dev(self, d_src, d_dst=None, stream: int | None = None, valid_thresh: float | None = None):
        """cv::GaussianBlur(src, dst, Size(5, 5), 0) on the device (dcmt_gaussian5_dev; SL/main_sl.cpp:1253), without the cascade's
        masked select.  d_src: contiguous f32 CUDA tensor [batch][rows][cols] (or [rows][cols]); d_dst may be d_src (in place).
        Returns d_dst without synchronising.
        valid_thresh=t: the Gaussian that ignores holes (dcmt_gaussian5_valid_dev, include/dcmt.h): a pixel >= t becomes the
        average of its taps >= t, weighted as the Gaussian weights them; any other pixel comes back as it is.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        import torch
        assert _is_dev(d_src, torch.float32)
        b, r, c = _brc(d_src)
        if d_dst is None:
            with _on_stream(stream, d_src):
                d_dst = torch.full_like(d_src, float("nan"))
        assert _is_dev(d_dst, torch.float32) and d_dst.numel() == d_src.numel()
        if valid_thresh is not None:
            st = L.lib().dcmt_gaussian5_valid_dev(self._h, d_src.data_ptr(), d_dst.data_ptr(), r, c, b, float(valid_thresh), _stream(stream, d_src))
            _check(st, "dcmt_gaussian5_valid_dev")
            return d_dst
        st = L.lib().dcmt_gaussian5_dev(self._h, d_src.data_ptr(), d_dst.data_ptr(), r, c, b, _stream(stream, d_src))
        _check(st, "dcmt_gaussian5_dev")
        return d_dst

    def gaussian5(self, frame: np.ndarray, valid_thresh: float | None = None) -> np.ndarray:
        """One frame of host memory (dcmt_gaussian5, synchronous; any row stride): a new f32 array.  valid_thresh: as gaussian5_dev
        (dcmt_gaussian5_valid)."""
        a = _frame_f32(frame)
        out = np.empty(a.shape, dtype=np.float32)
        if valid_thresh is not None:
            st = L.lib().dcmt_gaussian5_valid(self._h, a.ctypes.data, a.strides[0], out.ctypes.data, out.strides[0], a.shape[0], a.shape[1],
                                              float(valid_thresh))
            _check(st, "dcmt_gaussian5_valid")
            return out
        st = L.lib().dcmt_gaussian5(self._h, a.ctypes.data, a.strides[0], out.ctypes.data, out.strides[0], a.shape[0], a.shape[1])
        _check(st, "dcmt_gaussian5")
        return out

    def bilateral5_dev(self, d_src, d_dst=None, sigma_color: float = 1.5, sigma_space: float = 2.0, stream: int | None = None):
        """cv::bilateralFilter(src, dst, 5, sigma_color, sigma_space) on the device as include/dcmt.h states it (dcmt_bilateral5_dev):
        the edge-preserving alternative to gaussian5_dev, and the filter of blur_type="bilateral_clone".  Arguments, in-place use
        and the return value as gaussian5_dev."""
        import torch
        assert _is_dev(d_src, torch.float32)
        b, r, c = _brc(d_src)
        if d_dst is None:
            with _on_stream(stream, d_src):
                d_dst = torch.full_like(d_src, float("nan"))
        assert _is_dev(d_dst, torch.float32) and d_dst.numel() == d_src.numel()
        st = L.lib().dcmt_bilateral5_dev(self._h, d_src.data_ptr(), d_dst.data_ptr(), r, c, b, float(sigma_color), float(sigma_space),
                                         _stream(stream, d_src))
        _check(st, "dcmt_bilateral5_dev")
        return d_dst

    def bilateral5(self, frame: np.ndarray, sigma_color: float = 1.5, sigma_space: float = 2.0) -> np.ndarray:
        """One frame of host memory (dcmt_bilateral5, synchronous; any row stride): a new f32 array."""
        a = _frame_f32(frame)
        out = np.empty(a.shape, dtype=np.float32)
        st = L.lib().dcmt_bilateral5(self._h, a.ctypes.data, a.strides[0], out.ctypes.data, out.strides[0], a.shape[0], a.shape[1],
                                     float(sigma_color), float(sigma_space))
        _check(st, "dcmt_bilateral5")
        return out

    # ---- a plane seen by one camera -> the plane another camera sees (dcmt_reproject_depth*) ------------------------------
    def reproject_depth_dev(self, d_depth, out_rows: int, out_cols: int, params: L.ReprojectParams | None = None, d_out=None,
                            stream: int | None = None, nearest: bool = False):
        """The data part of the reference's unrectify_sol (SL/main_sl.cpp:967-1028) on the device: every source pixel is un-projected
        with the intrinsics, moved by M, projected with K and, where it lands inside [out_rows][out_cols], stores its new depth; the
        last source pixel in row-major order wins a destination pixel, pixels nothing lands on are 0.  d_depth: contiguous f32 CUDA
        tensor [batch][rows][cols] (or [rows][cols]: a batch of one).  Returns d_out, f32 [batch][out_rows][out_cols] (or
        [out_rows][out_cols]), which must not overlap d_depth.  No synchronisation.  nearest=True: a z-buffer -- a destination pixel
        keeps the smallest new depth that lands on it instead of the last (dcmt_reproject_depth_nearest_dev).
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        p = params or make_reproject_params()
        return self._reproject_depth_dev(d_depth, out_rows, out_cols, _rule("dcmt_reproject_depth_dev", nearest), lambda b: (ctypes.byref(p),), d_out, stream)

    def _reproject_depth_dev(self, d_depth, out_rows, out_cols, name, geo, d_out, stream):
        """reproject_depth_dev / reproject_depth_calib_dev: `name` the entry point, geo(batch) what it takes between batch and d_out."""
        import torch
        assert _is_dev(d_depth, torch.float32)
        b, r, c = _brc(d_depth)
        if d_out is None:
            with _on_stream(stream, d_depth):
                d_out = torch.full(tuple(d_depth.shape[:-2]) + (out_rows, out_cols), float("nan"), dtype=torch.float32, device=d_depth.device)
        assert _is_dev(d_out, torch.float32) and d_out.numel() == b * out_rows * out_cols
        st = getattr(L.lib(), name)(self._h, d_depth.data_ptr(), r, c, b, *geo(b), d_out.data_ptr(), int(out_rows), int(out_cols),
                                    _stream(stream, d_depth))
        _check(st, name)
        return d_out

    def reproject_depth_calib_dev(self, d_depth, out_rows: int, out_cols: int, d_calib, d_out=None, stream: int | None = None,
                                  nearest: bool = False):
        """reproject_depth_dev with each frame's own intrinsics, M and K (dcmt_reproject_depth_calib_dev): d_calib is a CUDA tensor
        holding [batch] dcmt_reproject_params records (make_reproject_calib, calib_to_device), read on the stream the call enqueues
        on.  A frame whose record the uniform call would refuse gives a zero plane.  nearest: as for reproject_depth_dev.
        Outputs that are not given are allocated (and, where they have a fill, filled) on the stream the call enqueues on."""
        return self._reproject_depth_dev(d_depth, out_rows, out_cols, _rule("dcmt_reproject_depth_calib_dev", nearest),
                                         lambda b: (_table_ptr(d_calib, b, REPROJECT_CALIB_DTYPE.itemsize),), d_out, stream)

    def reproject_depth(self, depth: np.ndarray, out_rows: int, out_cols: int, params: L.ReprojectParams | None = None,
                        nearest: bool = False) -> np.ndarray:
        """One frame of host memory (dcmt_reproject_depth, synchronous; any row stride): a new f32 array [out_rows][out_cols].
        nearest=True: dcmt_reproject_depth_nearest, the z-buffer of reproject_depth_dev."""
        a = _frame_f32(depth)
        out = np.empty((int(out_rows), int(out_cols)), dtype=np.float32)
        p = params or make_reproject_params()
        name = _rule("dcmt_reproject_depth", nearest)
        st = getattr(L.lib(), name)(self._h, a.ctypes.data, a.strides[0], a.shape[0], a.shape[1], ctypes.byref(p), out.ctypes.data,
                                    out.strides[0], out.shape[0], out.shape[1])
        _check(st, name)
        return out

    def last_fill_iters(self, n: int):
        out = (ctypes.c_int * n)()
        st = L.lib().dcmt_last_fill_iters(self._h, out, n)
        if st not in (L.OK, L.E_NOT_CONVERGED):
            raise DcmtError(st, "dcmt_last_fill_iters")
        return list(out), st

    def set_kernel_timing(self, on: bool = True):
        """Measurement aid: HIP events around the kernel groups of the streaming path of every following *_dev call."""
        st = L.lib().dcmt_set_kernel_timing(self._h, int(bool(on)))
        _check(st, "dcmt_set_kernel_timing")

    def last_kernel_times(self) -> dict:
        """Milliseconds of the last *_dev call's kernel groups (synchronises with its stream)."""
        ms = (ctypes.c_float * 4)()
        st = L.lib().dcmt_last_kernel_times(self._h, ms)
        _check(st, "dcmt_last_kernel_times")
        return {"front": ms[0], "k_pre": ms[1], "k_fp": ms[2], "k_fp_s": ms[2], "behind": ms[3]}

    def last_path(self) -> str:
        """The kernels the last cascade call dispatched (dcmt_last_path)."""
        return L.lib().dcmt_last_path(self._h).decode()

    def last_holes_after_extend(self, n: int):
        out = (ctypes.c_int * n)()
        st = L.lib().dcmt_last_holes_after_extend(self._h, out, n)
        _check(st, "dcmt_last_holes_after_extend")
        return list(out)


_default_ctx: dict = {}


def _ctx_for(rows: int, cols: int, batch: int, device: int = 0) -> Context:
    key = device
    c = _default_ctx.get(key)
    if c is None or c.max_rows < rows or c.max_cols < cols or c.max_batch < batch:
        if c is not None:
            c.close()
        c = Context(device, max(rows, 352), max(cols, 1216), max(batch, 1))
        _default_ctx[key] = c
    return c


def img_completion(sparse_r_img: np.ndarray, extr: bool = False, blur_type: str = "gaussian", **kw) -> np.ndarray:
    """Drop-in for the reference's img_completion (LO/img_completion.cpp:17): returns dense_r_img.
    `extr` is accepted and ignored, as in the reference (:19, never read); the cascade without its extrapolation is the keyword
    `extrapolate=False` (make_params)."""
    a = np.asarray(sparse_r_img, dtype=np.float32)
    b = 1 if a.ndim == 2 else a.shape[0]
    return _ctx_for(a.shape[-2], a.shape[-1], b).complete(a, make_params(blur_type=blur_type, **kw))


def interpolate_with_superpixels(labels: np.ndarray, n_labels: int, sparse_r_img: np.ndarray,
                                 blur_type: str = "gaussian", use_superpixel: int = 1, **kw) -> np.ndarray:
    """Drop-in for LC/img_completion_lc.cpp:34.  `labels` is int32 [rows][cols] (the reference's
    Slic::clusters is [col][row]: pass clusters.T), n_labels = slic.centers.size().  blur_type is
    accepted and ignored, as in the reference (:37, :183 always blurs) -- except "gaussian_valid", this project's own finish."""
    a = np.asarray(sparse_r_img, dtype=np.float32)
    b = 1 if a.ndim == 2 else a.shape[0]
    blur = "gaussian_valid" if blur_type == "gaussian_valid" else "gaussian"
    return _ctx_for(a.shape[-2], a.shape[-1], b).complete(a, make_params(blur_type=blur, **kw), labels=labels,
                                                          n_labels=n_labels, use_superpixel=use_superpixel)


def to_color_image(r_img):
    """The reference's toColorImage (DC_lidar_only/main.cpp:6-14): a depth plane -> its JET image, uint8 [rows][cols][3] in
    B, G, R order.  A numpy frame goes through the host entry point; a CUDA tensor ([rows][cols] or [batch][rows][cols]) through
    the device one, on torch's current stream, and comes back as a CUDA tensor without synchronising."""
    if hasattr(r_img, "is_cuda") and r_img.is_cuda:
        b = 1 if r_img.dim() == 2 else r_img.shape[0]
        return _ctx_for(r_img.shape[-2], r_img.shape[-1], b, r_img.device.index or 0).colorize_dev(r_img)
    a = np.asarray(r_img, dtype=np.float32)
    return _ctx_for(a.shape[0], a.shape[1], 1).colorize(a)


def _bgr_convert(img, lab: bool):
    if hasattr(img, "is_cuda") and img.is_cuda:
        b = 1 if img.dim() == 3 else img.shape[0]
        return _ctx_for(img.shape[-3], img.shape[-2], b, img.device.index or 0).bgr_convert_dev(img, lab=lab, gray=not lab)
    a = np.asarray(img, dtype=np.uint8)
    return _ctx_for(a.shape[0], a.shape[1], 1).bgr_convert(a, lab=lab, gray=not lab)


def bgr_to_lab(img):
    """cv::cvtColor(img, lab, cv::COLOR_BGR2Lab) on 8-bit pixels (LC/main_lc.cpp:183, SL/main_sl.cpp:439): uint8 [rows][cols][3]
    B, G, R -> L * 255 / 100, a + 128, b + 128.  A numpy frame goes through the host entry point; a CUDA tensor ([rows][cols][3] or
    [batch][rows][cols][3]) through the device one, on torch's current stream, and comes back as a CUDA tensor without synchronising."""
    return _bgr_convert(img, True)


def bgr_to_gray(img):
    """cv::cvtColor(img, gray, cv::COLOR_BGR2GRAY) on 8-bit pixels (SL/main_sl.cpp:1167, :1171): uint8 [...][rows][cols][3] ->
    [...][rows][cols]; numpy or CUDA tensor, as bgr_to_lab."""
    return _bgr_convert(img, False)


def undistort_rectify(img, K, D, R, P, out_shape):
    """The reference's rectify() for one camera (SL/main_sl.cpp:1350-1381: cv::initUndistortRectifyMap, then cv::remap with
    INTER_LINEAR), as include/dcmt.h states it: img uint8 [rows][cols] or [rows][cols][3] -> the undistorted, rectified frame of
    out_shape = (rows, cols).  K, D, R, P: K_0x, D_0x, R_rect_0x, P_rect_0x of calib_cam_to_cam.txt.  numpy or CUDA tensor, as
    bgr_to_lab."""
    rows, cols = out_shape
    if hasattr(img, "is_cuda") and img.is_cuda:
        return _ctx_for(rows, cols, 1, img.device.index or 0).rectify(img, K, D, R, P, out_shape)
    return _ctx_for(rows, cols, 1).rectify(img, K, D, R, P, out_shape)


def get_initial_error(depth, left, right, **params):
    """The reference's get_initial_error (SL/main_sl.cpp:618-712) on one host frame, its data: (err, stats) -- the uint8 error map and a
    dict of the four counts of PHOTO_STATS (the reference prints matches, nonzero and valid).  left, right: grey uint8 [rows][cols], or
    BGR uint8 [rows][cols][3], which go through bgr_to_gray as the reference's cv::cvtColor calls do (:625, :630).  params: baseline,
    focal, window."""
    d = np.asarray(depth, dtype=np.float32)
    imgs = [np.asarray(a, dtype=np.uint8) for a in (left, right)]
    imgs = [bgr_to_gray(a) if a.ndim == 3 else a for a in imgs]
    e, s = _ctx_for(d.shape[0], d.shape[1], 1).photo_error(d, imgs[0], imgs[1], **params)
    return e, {k: int(v) for k, v in zip(PHOTO_STATS, s)}


def stereo_sgm(left, right, depth: bool = False, speckle_window: int | None = None, speckle_range: int | None = None, paths: int = 4,
               guide=None, guide_weight: int = SGM_GUIDE_WEIGHT, guide_cap: int = SGM_GUIDE_CAP, cost: str = "absdiff", **params):
    """Semi-global matching of one rectified host pair (dcmt_sgm): the int16 disparity map in sixteenths of a pixel, -16 where invalid,
    as cv::StereoSGBM::compute returns it (SL/main_sl.cpp:1293-1339); with depth=True (disp16, depth).  left, right: grey uint8
    [rows][cols], or BGR uint8 [rows][cols][3], which go through bgr_to_gray.  params: the fields of make_sgm_params.
    speckle_window, speckle_range: StereoSGBM's speckleWindowSize and speckleRange (the reference's: 200, 2); None, None: no filter.
    paths: 4, or 8 for the four diagonal paths as well (p2 <= 1800 then); ValueError otherwise, before any call.
    guide: an f32 depth plane [rows][cols] in the left camera, metres, 0 where there is none (project_points(..., nearest=True)):
    LiDAR-guided matching (dcmt_sgm_guided; include/dcmt.h, step 2b) with the penalty min(guide_weight * |d - h|, guide_cap);
    guide_weight in 0..10000, guide_cap >= 0, p2 + guide_cap <= 10000 (1800 with 8 paths), or ValueError before any call.
    cost: "absdiff", or "census" for the census matching cost (dcmt_sgm_cost; include/dcmt.h, steps 1c / 2c), which differences in
    exposure and gain between the two images do not disturb; ValueError otherwise, before any call."""
    p = make_sgm_params(for_depth=depth, **params)
    paths = _check_sgm_paths(paths, p)
    _check_sgm_cost(cost)
    if guide is not None:
        _check_sgm_guide(guide_weight, guide_cap, paths, p)
    imgs = [np.asarray(a, dtype=np.uint8) for a in (left, right)]
    imgs = [bgr_to_gray(a) if a.ndim == 3 else a for a in imgs]
    return _ctx_for(imgs[0].shape[0], imgs[0].shape[1], 1).sgm(imgs[0], imgs[1], depth=depth, speckle_window=speckle_window,
                                                                speckle_range=speckle_range, paths=paths, guide=guide,
                                                                guide_weight=guide_weight, guide_cap=guide_cap, cost=cost, **params)


def filter_speckles(disp16, depth=None, **params):
    """cv::filterSpeckles of one int16 host disparity map (dcmt_filter_speckles, as include/dcmt.h states it): (the filtered plane,
    the number of pixels changed), or with a depth plane (plane, depth, count).  params: max_size (200), max_diff (32, in
    sixteenths), new_val (-16)."""
    d = np.asarray(disp16, dtype=np.int16)
    return _ctx_for(d.shape[0], d.shape[1], 1).filter_speckles(d, depth, **params)


def fit_superpixel_planes(depth, labels, n_labels: int, **params):
    """One plane of inverse depth per superpixel of one host frame (dcmt_superpixel_planes, as include/dcmt.h states it): depth f32
    [rows][cols] in metres with 0 = no return, labels int32 [rows][cols] -> (the painted plane, the fits [n_labels] as
    PLANE_FIT_DTYPE).  params: the fields of make_planes_params."""
    z = np.asarray(depth, dtype=np.float32)
    return _ctx_for(z.shape[0], z.shape[1], 1).superpixel_planes(z, labels, n_labels, **params)


def filter_occluded_returns(depth, **params):
    """The occlusion filter of one host frame (dcmt_sparse_occlusion, as include/dcmt.h states it): depth f32 [rows][cols] in metres
    with 0 = no return -> the plane without the returns a nearer return in the window shows to be hidden from the camera (a new
    array).  params: the fields of make_occlusion_params."""
    z = np.asarray(depth, dtype=np.float32)
    return _ctx_for(z.shape[0], z.shape[1], 1).sparse_occlusion(z, **params)[0]


def distance_to_returns(sparse, **params):
    """The support map of one host frame (dcmt_support_distance, as include/dcmt.h states it): sparse f32 [rows][cols] in metres ->
    uint16 [rows][cols], the exact squared Euclidean distance to the nearest return where that is at most max_radius^2 (default 9),
    65535 everywhere else.  params: the fields of make_support_params."""
    z = np.asarray(sparse, dtype=np.float32)
    return _ctx_for(z.shape[0], z.shape[1], 1).support_distance(z, **params)[0]


def trust_mask(sparse, dense, fallback=None, **params):
    """The trust mask of one host frame (dcmt_support_distance): dense where a return of sparse lies within max_radius (default 9),
    elsewhere fallback (the stereo matcher's depth, say) or 0 -- a new f32 array; the bits are copied, a NaN keeps its own.
    params: the fields of make_support_params."""
    z = np.asarray(sparse, dtype=np.float32)
    return _ctx_for(z.shape[0], z.shape[1], 1).support_distance(z, dense, fallback, **params)[0]


def joint_bilateral_fill(depth, guide, tables=None, **params):
    """Fill the holes of one host depth frame from the measured depths around them whose camera pixels look like theirs
    (dcmt_joint_bilateral, as include/dcmt.h states it): depth f32 [rows][cols] in metres, guide uint8 [rows][cols] or
    [rows][cols][3] -> a new f32 array; valid pixels keep their bytes unless smooth=True.  params: the fields of make_joint_params."""
    z = np.asarray(depth, dtype=np.float32)
    return _ctx_for(z.shape[0], z.shape[1], 1).joint_bilateral(z, guide, tables, **params)[0]


def depth_normals(depth, params=None, **kw):
    """The surface normals of one host depth frame (dcmt_depth_normals, as include/dcmt.h states it): depth f32 [rows][cols] in
    metres -> f32 [rows][cols][4], the unit normal towards the camera and the distance of the pixel's local plane from the camera
    centre; four zeros on a hole and where no normal is defined.  params: the intrinsics (make_cloud_params; the reference's by
    default); kw: the fields of make_normals_params."""
    z = np.asarray(depth, dtype=np.float32)
    return _ctx_for(z.shape[0], z.shape[1], 1).depth_normals(z, params, filtered=False, **kw)[0]


def filter_flying_pixels(depth, params=None, **kw):
    """The flying-pixel filter of one host depth frame (dcmt_depth_normals): a new f32 array, 0 where the pixel's local plane passes
    closer to the camera centre than min_plane_dist (default 0.4 m) -- the veil a blur strings between an object and the wall
    behind it --, elsewhere the input's bits.  params: the intrinsics; kw: the fields of make_normals_params."""
    z = np.asarray(depth, dtype=np.float32)
    return _ctx_for(z.shape[0], z.shape[1], 1).depth_normals(z, params, normals=False, **kw)[1]


def depth_to_u16(depth, scale: float = 256.0):
    """A depth plane in metres as KITTI stores it: uint16 round(depth * scale), ties to even, saturated (what the reference's
    commented imwrite lines intend, LC/main_lc.cpp:233-234).  A numpy frame goes through the host entry point; a CUDA tensor
    ([rows][cols] or [batch][rows][cols]) through the device one, on torch's current stream, without synchronising."""
    if hasattr(depth, "is_cuda") and depth.is_cuda:
        b = 1 if depth.dim() == 2 else depth.shape[0]
        return _ctx_for(depth.shape[-2], depth.shape[-1], b, depth.device.index or 0).depth_to_u16_dev(depth, scale)
    a = np.asarray(depth, dtype=np.float32)
    return _ctx_for(a.shape[0], a.shape[1], 1).depth_to_u16(a, scale)


def bilateral_filter5(frame, sigma_color: float = 1.5, sigma_space: float = 2.0) -> np.ndarray:
    """cv::bilateralFilter(frame, out, 5, sigma_color, sigma_space) on one host frame, as include/dcmt.h states it
    (Context.bilateral5): a new f32 array.  The defaults are the cascade's literals (LO/img_completion.cpp:174)."""
    a = np.asarray(frame, dtype=np.float32)
    return _ctx_for(a.shape[0], a.shape[1], 1).bilateral5(a, sigma_color, sigma_space)


def slic_connectivity_max_labels(rows: int, cols: int, n_centers: int) -> int:
    """The bound on a frame's label count behind the connectivity pass (dcmt_slic_connectivity_max_labels; needs no GPU): what
    complete_dev takes as n_labels.  ValueError for a shape the pass refuses (n_centers < 1, fewer than 4 pixels per centre)."""
    m = L.lib().dcmt_slic_connectivity_max_labels(int(rows), int(cols), int(n_centers))
    if m < 1:
        raise ValueError(f"slic_connectivity_max_labels({rows}, {cols}, {n_centers}): (rows * cols) / n_centers must be at least 4")
    return m


def slic_enforce_connectivity(labels, n_centers: int):
    """The reference's slic.create_connectivity(lab_image) (LC/main_lc.cpp:202) on one host frame, with its result kept
    (Context.slic_connectivity): labels int32 [rows][cols] (clusters.T), n_centers = slic.centers.size() -> (labels, count)."""
    a = np.asarray(labels, dtype=np.int32)
    return _ctx_for(a.shape[0], a.shape[1], 1).slic_connectivity(a, n_centers)


def slic_display_contours(labels, image, colour=(0, 0, 200)):
    """The reference's slic.display_contours(image, CV_RGB(200,0,0)) (LC/main_lc.cpp:214) on one host frame (Context.slic_contours):
    labels int32 [rows][cols] (clusters.T), image uint8 [rows][cols][3] B, G, R, colour B, G, R -> the painted copy of the image."""
    a = np.asarray(labels, dtype=np.int32)
    return _ctx_for(a.shape[0], a.shape[1], 1).slic_contours(a, image, colour)[0]


def slic_colour_with_cluster_means(labels, image, n_labels: int):
    """The reference's slic.colour_with_cluster_means(image) (LC/slic.cpp:392-433) on one host frame (Context.slic_cluster_means):
    n_labels = slic.centers.size() -> the copy of the image with every superpixel in its mean colour."""
    a = np.asarray(labels, dtype=np.int32)
    return _ctx_for(a.shape[0], a.shape[1], 1).slic_cluster_means(a, image, n_labels)[0]


def reproject_pc_colors(depth, bgr):
    """The reference's reproject_pc_colors (SL/main_sl.cpp:924-965) on one frame: the ordered coloured cloud of a depth plane.
    numpy in: a structured array (CLOUD_DTYPE) of the true length, through the host entry point.  CUDA tensors in ([rows][cols]
    f32 and [rows][cols][3] uint8): a float32 CUDA tensor [n, 4] of the true length (fourth column: the colour bits); reading the
    count synchronises with torch's current stream."""
    if hasattr(depth, "is_cuda") and depth.is_cuda:
        assert depth.dim() == 2
        pts, off = _ctx_for(depth.shape[0], depth.shape[1], 1, depth.device.index or 0).depth_to_cloud_dev(depth, bgr)
        return pts[:int(off[1].item())]
    a = np.asarray(depth, dtype=np.float32)
    return _ctx_for(a.shape[0], a.shape[1], 1).depth_to_cloud(a, bgr)


def reproject_pc(depth):
    """The reference's reproject_pc (SL/main_sl.cpp:887-922): as reproject_pc_colors without a colour plane; the fourth dword of
    every record is 1.0f."""
    return reproject_pc_colors(depth, None)


def reproject_pc_normals(depth, bgr=None):
    """reproject_pc_colors (reproject_pc without bgr) of one host frame with the normal of every point: (the cloud, f32 [n][4] = nx ny
    nz dist).  The cloud's records are the pixels with depth > 0 in row-major order, so the row-major selection of the normals is
    their order.  Both under the reference's intrinsics (make_cloud_params)."""
    a = np.asarray(depth, dtype=np.float32)
    return reproject_pc_colors(a, bgr), depth_normals(a)[a > 0]


def unrectify_sol(depth_pre_optim, out_shape, R_rect, nearest: bool = False) -> np.ndarray:
    """The reference's unrectify_sol (SL/main_sl.cpp:967-1028, called at :1228) on one host frame, without its drawing and printing:
    depth_pre_optim forward-warped into the un-rectified camera's frame, a new f32 array of out_shape = (rows, cols) that is 0 where
    nothing lands.  R_rect: the 4x4 matrix the reference passes (R_rect_02).  The matrix that is applied is inverse_f32(R_rect): the
    inverse computed in f64 and rounded to f32 -- ours, not the bits of Eigen's f32 inverse().  nearest=True: the warp as a z-buffer
    (Context.reproject_depth)."""
    a = np.asarray(depth_pre_optim, dtype=np.float32)
    rows, cols = int(out_shape[0]), int(out_shape[1])
    ctx = _ctx_for(max(a.shape[0], rows), max(a.shape[1], cols), 1)
    return ctx.reproject_depth(a, rows, cols, make_reproject_params(M=inverse_f32(R_rect)), nearest=nearest)


def write_pcd(path, points, normals=None) -> None:
    """Writes a cloud (CLOUD_DTYPE records, or anything of 16 bytes per record such as a float32 [n, 4] array) as the binary
    .pcd pcl::PCDWriter::writeBinary makes of a PointXYZRGB cloud (SL/main_sl.cpp:962-963): FIELDS x y z rgb, SIZE 4 4 4 4,
    TYPE F F F F, COUNT 1 1 1 1, WIDTH n, HEIGHT 1, POINTS n, DATA binary, then the records as they are.  With normals (f32 [n][3]
    or [n][4] as reproject_pc_normals gives them: nx ny nz and a fourth column that is not written) every record is followed by
    normal_x normal_y normal_z curvature, the fields of PCL's PointXYZRGBNormal, curvature written as 0.  The header text is
    what PCL's file-format page documents; neither PCL nor a file written by it was available to compare with, so it is checked
    only by the round trip through read_pcd."""
    rec = np.ascontiguousarray(points)
    if rec.dtype != CLOUD_DTYPE:
        rec = rec.view(np.uint8).reshape(-1, 16).view(CLOUD_DTYPE).reshape(-1)
    n = rec.shape[0]
    fields, k = "x y z rgb", 4
    body = rec.view(np.uint8).reshape(n, 16)
    if normals is not None:
        nrm = np.asarray(normals, dtype=np.float32)
        if nrm.ndim != 2 or nrm.shape[0] != n or nrm.shape[1] not in (3, 4):
            raise ValueError(f"write_pcd: normals of shape {nrm.shape} for {n} points; [n][3] or [n][4]")
        tail = np.zeros((n, 4), dtype=np.float32)
        tail[:, :3] = nrm[:, :3]
        body = np.concatenate([body, tail.view(np.uint8).reshape(n, 16)], axis=1)
        fields, k = fields + " normal_x normal_y normal_z curvature", 8
    head = (f"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS {fields}\nSIZE{' 4' * k}\nTYPE{' F' * k}\nCOUNT{' 1' * k}\n"
            f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(np.ascontiguousarray(body).tobytes())


def read_pcd(path, normals: bool = False):
    """Reads a binary .pcd of four or eight 4-byte fields per point (what write_pcd writes) back into CLOUD_DTYPE records; with
    normals=True (the records, f32 [n][3] = normal_x normal_y normal_z), and ValueError for a file without them."""
    with open(path, "rb") as f:
        blob = f.read()
    fields, pos = {}, 0
    while True:
        end = blob.index(b"\n", pos)
        line = blob[pos:end].decode("ascii")
        pos = end + 1
        if line.startswith("#") or not line.strip():
            continue
        key, _, val = line.partition(" ")
        fields[key] = val.strip()
        if key == "DATA":
            break
    names = fields.get("FIELDS", "").split()
    k = len(names)
    if fields["DATA"] != "binary" or k not in (4, 8) or fields.get("SIZE") != " ".join(["4"] * k) or fields.get("COUNT") != " ".join(["1"] * k):
        raise ValueError("read_pcd: only binary files of four or eight 4-byte fields per point are supported")
    if k == 8 and names[4:7] != ["normal_x", "normal_y", "normal_z"]:
        raise ValueError("read_pcd: eight fields that are not x y z rgb normal_x normal_y normal_z curvature")
    if normals and k != 8:
        raise ValueError("read_pcd: the file has no normals")
    n = int(fields["POINTS"])
    if len(blob) - pos < 4 * k * n:
        raise ValueError("read_pcd: file shorter than its POINTS line says")
    body = np.frombuffer(blob, dtype=np.uint8, count=4 * k * n, offset=pos).reshape(n, 4 * k)
    pts = np.ascontiguousarray(body[:, :16]).view(CLOUD_DTYPE).reshape(n).copy()
    if not normals:
        return pts
    return pts, np.ascontiguousarray(body[:, 16:28]).view(np.float32).reshape(n, 3).copy()


_jet = None


def __getattr__(name):
    # JET_BGR: the palette the kernels use (dcmt_colormap_jet), (256, 3) uint8, B, G, R; read-only.  Loaded on first use.
    global _jet
    if name == "JET_BGR":
        if _jet is None:
            buf = (ctypes.c_uint8 * 768)()
            L.lib().dcmt_colormap_jet(buf)
            _jet = np.ctypeslib.as_array(buf).reshape(256, 3)
            _jet.flags.writeable = False
        return _jet
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _sums_array(sums) -> np.ndarray:
    if hasattr(sums, "detach"):                  # a torch tensor: copying it to the host synchronises with its stream
        sums = sums.detach().cpu().numpy()
    return np.asarray(sums, dtype=np.float64).reshape(-1, 7)


def _metrics(s: np.ndarray) -> dict:
    with np.errstate(divide="ignore", invalid="ignore"):
        n, n_inv = s[:, 0], s[:, 4]
        return {"me": s[:, 1] / n, "mae": s[:, 2] / n, "rmse": np.sqrt(s[:, 3] / n),
                "imae": 1000.0 * s[:, 5] / n_inv, "irmse": 1000.0 * np.sqrt(s[:, 6] / n_inv)}


def eval_summary(sums) -> dict:
    """Metrics from evaluate_dev / evaluate sums ([batch, 7] or [7]; numpy or torch).  me (signed mean of gt - pred), mae, rmse in
    the GT's unit (metres); imae, irmse in 1/km (the KITTI depth-completion table's unit for inverse depth).  f64 throughout.
      "per_frame":      each metric per frame (arrays), plus the pixel counts n and n_inv; a frame with an empty mask gives NaN;
      "pixel_weighted": over the batch, every masked pixel weighing the same (the sums of all frames, then one division);
      "frame_mean":     the mean of the per-frame metrics over the frames whose mask is not empty (NaN if there is none)."""
    s = _sums_array(sums)
    per = _metrics(s)
    pw = {k: float(v[0]) for k, v in _metrics(s.sum(axis=0, keepdims=True)).items()}
    fm = {}
    for k, v in per.items():
        ok = ~np.isnan(v)
        fm[k] = float(v[ok].mean()) if ok.any() else float("nan")
    per = dict(per, n=s[:, 0].copy(), n_inv=s[:, 4].copy())
    return {"per_frame": per, "pixel_weighted": pw, "frame_mean": fm}


def reference_performance(sums, preset: str):
    """The reference function's own results from sums made with the preset's mode and threshold (EVAL_PRESETS), with its final
    arithmetic in f32: float(sum) / count, then sqrt (the count converted to float as `float / int` does).
      "lidar_only":   mse (the signed mean error; the name is the reference's)           LO main.cpp:33
      "lidar_camera": (mse, mae), where mse is the RMSE                                   LC main_lc.cpp:114-115
      "stereo_lidar": (mae, rmse)                                                         SL main_sl.cpp:1058-1059
    np.float32 values for a single frame's sums ([7]), arrays of them for [batch, 7].  An empty mask gives NaN (0 / 0)."""
    if preset not in EVAL_PRESETS:
        raise ValueError(f"preset must be one of {sorted(EVAL_PRESETS)}")
    arr = np.asarray(sums.detach().cpu().numpy() if hasattr(sums, "detach") else sums, dtype=np.float64)
    single = arr.ndim == 1
    s = arr.reshape(-1, 7)
    f32 = np.float32
    cnt = s[:, 0].astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        if preset == "lidar_only":
            res = (s[:, 1].astype(f32) / cnt,)
        else:
            mae = s[:, 2].astype(f32) / cnt
            rmse = np.sqrt(s[:, 3].astype(f32) / cnt)
            res = (rmse, mae) if preset == "lidar_camera" else (mae, rmse)
    res = tuple(r[0] if single else r for r in res)
    return res[0] if len(res) == 1 else res


def evaluate_performance(gt, pred, preset: str = "lidar_only", gt_scale: float = 1.0 / 256.0):
    """Drop-in for the reference's evaluate_performance(s) (EVAL_PRESETS, reference_performance for what each returns).
    numpy frames [rows][cols] go through the host entry point (a uint16 GT is converted as payload * gt_scale in f32);
    CUDA tensors [batch][rows][cols] through the device one (per-frame arrays; the result is copied back, so this synchronises)."""
    if preset not in EVAL_PRESETS:
        raise ValueError(f"preset must be one of {sorted(EVAL_PRESETS)}")
    mode, thresh = EVAL_PRESETS[preset]
    if hasattr(pred, "is_cuda") and pred.is_cuda:
        b = 1 if pred.dim() == 2 else pred.shape[0]
        ctx = _ctx_for(pred.shape[-2], pred.shape[-1], b, pred.device.index or 0)
        sums = ctx.evaluate_dev(gt, pred, thresh, mode, gt_scale).cpu().numpy()
        return reference_performance(sums[0] if pred.dim() == 2 else sums, preset)
    g = np.asarray(gt)
    if g.dtype == np.uint16:
        g = g.astype(np.float32) * np.float32(gt_scale)
    q = np.asarray(pred, dtype=np.float32)
    return reference_performance(_ctx_for(q.shape[0], q.shape[1], 1).evaluate(g, q, thresh, mode), preset)
