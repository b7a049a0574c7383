"""ctypes loader for libdcmt_hip.so (the C ABI of include/dcmt.h).

There is no fallback: if the shared library is missing it is built with hipcc, and if that
fails the import raises.  Nothing under oracle/ is ever imported from here.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(_CSRC, "libdcmt_hip.so")

OK, E_INVALID, E_UNSUPPORTED, E_NOMEM, E_HIP, E_NOT_CONVERGED, E_NO_DEVICE = 0, -1, -2, -3, -4, -5, -6
BLUR_NONE, BLUR_GAUSSIAN, BLUR_BILATERAL, BLUR_BILATERAL_CLONE, BLUR_GAUSSIAN_VALID = 0, 1, 2, 3, 5
STAGE_NORMALIZE = 1
STAGE_INVERT, STAGE_DILATE_K, STAGE_CLOSE5, STAGE_FILL7, STAGE_EXTEND = 2, 3, 4, 5, 6
FLAG_FORCE_STAGED = 1
FLAG_FORCE_FUSED = 2
FLAG_NORMALIZE = 4
FLAG_NO_EXTRAPOLATE = 8
STAGE_FILL31, STAGE_FILLLOOP, STAGE_MEDIAN5, STAGE_BLUR, STAGE_FINAL = 7, 8, 9, 10, 11
EVAL_GT, EVAL_BOTH = 0, 1
RECTIFY_FORCE_GATHER = 1

# every symbol include/dcmt.h declares (tests check the library exports exactly these)
EXPORTS = (
    "dcmt_device_count", "dcmt_create", "dcmt_destroy", "dcmt_default_params", "dcmt_k0_as_compiled",
    "dcmt_k0_diamond", "dcmt_complete_f32", "dcmt_complete_f32_dev", "dcmt_complete_labeled_f32",
    "dcmt_complete_labeled_f32_dev", "dcmt_complete_u16_dev", "dcmt_last_fill_iters", "dcmt_last_holes_after_extend",
    "dcmt_strerror", "dcmt_last_hip_error", "dcmt_version", "dcmt_project_points_dev", "dcmt_set_kernel_timing", "dcmt_last_kernel_times",
    "dcmt_slic_num_centers", "dcmt_slic_labels_dev", "dcmt_default_stereo_params", "dcmt_stereo_refine_dev",
    "dcmt_project_points", "dcmt_slic_labels", "dcmt_stereo_refine", "dcmt_last_path",
    "dcmt_evaluate_dev", "dcmt_evaluate_u16_dev", "dcmt_evaluate",
    "dcmt_colorize_dev", "dcmt_colorize", "dcmt_colormap_jet",
    "dcmt_default_cloud_params", "dcmt_depth_to_cloud_dev", "dcmt_depth_to_cloud", "dcmt_gaussian5_dev", "dcmt_gaussian5",
    "dcmt_default_reproject_params", "dcmt_reproject_depth_dev", "dcmt_reproject_depth",
    "dcmt_bgr_convert_dev", "dcmt_bgr_convert", "dcmt_lab_tables",
    "dcmt_project_points_calib_dev", "dcmt_depth_to_cloud_calib_dev", "dcmt_reproject_depth_calib_dev", "dcmt_stereo_refine_calib_dev",
    "dcmt_crop_frames_dev", "dcmt_depth_to_u16_dev", "dcmt_depth_to_u16",
    "dcmt_project_points_nearest_dev", "dcmt_project_points_nearest_calib_dev", "dcmt_reproject_depth_nearest_dev",
    "dcmt_reproject_depth_nearest_calib_dev", "dcmt_project_points_nearest", "dcmt_reproject_depth_nearest",
    "dcmt_bilateral5_dev", "dcmt_bilateral5",
    "dcmt_slic_connectivity_max_labels", "dcmt_slic_connectivity_dev", "dcmt_slic_connectivity",
    "dcmt_slic_contours_dev", "dcmt_slic_cluster_means_dev", "dcmt_slic_contours", "dcmt_slic_cluster_means",
    "dcmt_default_photo_error_params", "dcmt_photo_error_dev", "dcmt_photo_error_calib_dev", "dcmt_photo_error",
    "dcmt_default_sgm_params", "dcmt_sgm_workspace_bytes", "dcmt_sgm_dev", "dcmt_sgm", "dcmt_sgm_paths_dev", "dcmt_sgm_paths",
    "dcmt_sgm_guided_dev", "dcmt_sgm_guided", "dcmt_sgm_cost_dev", "dcmt_sgm_cost",
    "dcmt_default_speckle_params", "dcmt_filter_speckles_dev", "dcmt_filter_speckles",
    "dcmt_rectify_map_dev", "dcmt_rectify_dev", "dcmt_rectify",
    "dcmt_default_planes_params", "dcmt_superpixel_planes_max_labels", "dcmt_superpixel_planes_dev", "dcmt_superpixel_planes",
    "dcmt_default_occlusion_params", "dcmt_sparse_occlusion_dev", "dcmt_sparse_occlusion_u16_dev", "dcmt_sparse_occlusion",
    "dcmt_default_support_params", "dcmt_support_distance_dev", "dcmt_support_distance_u16_dev", "dcmt_support_distance",
    "dcmt_default_joint_params", "dcmt_make_joint_tables", "dcmt_joint_bilateral_dev", "dcmt_joint_bilateral",
    "dcmt_default_normals_params", "dcmt_depth_normals_dev", "dcmt_depth_normals_calib_dev", "dcmt_depth_normals",
    "dcmt_gaussian5_valid_dev", "dcmt_gaussian5_valid",
)


class Params(ctypes.Structure):
    """Mirror of dcmt_params (include/dcmt.h)."""
    _fields_ = [
        ("max_depth", ctypes.c_float),
        ("valid_thresh", ctypes.c_float),
        ("k0", ctypes.c_uint8 * 25),
        ("_pad", ctypes.c_uint8 * 3),
        ("blur", ctypes.c_int32),
        ("max_fill_iters", ctypes.c_int32),
        ("spec_fill_iters", ctypes.c_int32),
        ("stop_after", ctypes.c_int32),
        ("verbose", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("norm_lo", ctypes.c_float),
        ("norm_hi", ctypes.c_float),
    ]


class StereoParams(ctypes.Structure):
    """Mirror of dcmt_stereo_params (include/dcmt.h)."""
    _fields_ = [("baseline", ctypes.c_float), ("focal", ctypes.c_float), ("damp", ctypes.c_float),
                ("max_depth", ctypes.c_float), ("iterations", ctypes.c_int32)]


class EvalFrame(ctypes.Structure):
    """Mirror of dcmt_eval_frame (include/dcmt.h): one frame's sums against ground truth."""
    _fields_ = [("n", ctypes.c_double), ("sum_err", ctypes.c_double), ("sum_abs", ctypes.c_double), ("sum_sq", ctypes.c_double),
                ("n_inv", ctypes.c_double), ("sum_inv_abs", ctypes.c_double), ("sum_inv_sq", ctypes.c_double)]


class CloudParams(ctypes.Structure):
    """Mirror of dcmt_cloud_params (include/dcmt.h): the pinhole intrinsics of the back-projection."""
    _fields_ = [("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double)]


class CloudPoint(ctypes.Structure):
    """Mirror of dcmt_cloud_point (include/dcmt.h): one 16-byte record."""
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float), ("z", ctypes.c_float),
                ("b", ctypes.c_uint8), ("g", ctypes.c_uint8), ("r", ctypes.c_uint8), ("a", ctypes.c_uint8)]


class ReprojectParams(ctypes.Structure):
    """Mirror of dcmt_reproject_params (include/dcmt.h): the source camera's intrinsics, the 4x4 transform that is applied and the
    destination camera's 3x3 matrix, both row-major."""
    _fields_ = [("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double),
                ("M", ctypes.c_float * 16), ("K", ctypes.c_float * 9)]


class ProjectCalib(ctypes.Structure):
    """Mirror of dcmt_project_calib (include/dcmt.h): one frame's record of dcmt_project_points_calib_dev, rows 0..2 of T, then P."""
    _fields_ = [("T", ctypes.c_float * 12), ("P", ctypes.c_float * 12)]


class StereoCalib(ctypes.Structure):
    """Mirror of dcmt_stereo_calib (include/dcmt.h): one frame's record of dcmt_stereo_refine_calib_dev."""
    _fields_ = [("baseline", ctypes.c_float), ("focal", ctypes.c_float)]


class PhotoErrorParams(ctypes.Structure):
    """Mirror of dcmt_photo_error_params (include/dcmt.h)."""
    _fields_ = [("baseline", ctypes.c_float), ("focal", ctypes.c_float), ("window", ctypes.c_int32)]


class SgmParams(ctypes.Structure):
    """Mirror of dcmt_sgm_params (include/dcmt.h)."""
    _fields_ = [("num_disparities", ctypes.c_int32), ("p1", ctypes.c_int32), ("p2", ctypes.c_int32), ("uniqueness", ctypes.c_int32),
                ("disp12_max_diff", ctypes.c_int32), ("baseline", ctypes.c_float), ("focal", ctypes.c_float), ("max_depth", ctypes.c_float)]


class SpeckleParams(ctypes.Structure):
    """Mirror of dcmt_speckle_params (include/dcmt.h)."""
    _fields_ = [("max_size", ctypes.c_int32), ("max_diff", ctypes.c_int32), ("new_val", ctypes.c_int32)]


class PlanesParams(ctypes.Structure):
    """Mirror of dcmt_planes_params (include/dcmt.h), 24 bytes."""
    _fields_ = [("valid_thresh", ctypes.c_float), ("max_depth", ctypes.c_float), ("min_points", ctypes.c_int32),
                ("min_extent", ctypes.c_int32), ("refit_tol", ctypes.c_float), ("keep_returns", ctypes.c_int32)]


class PlaneFit(ctypes.Structure):
    """Mirror of dcmt_plane_fit (include/dcmt.h): one label's record of dcmt_superpixel_planes_dev, 48 bytes."""
    _fields_ = [("a", ctypes.c_double), ("b", ctypes.c_double), ("c", ctypes.c_double), ("seen", ctypes.c_uint32), ("used", ctypes.c_uint32),
                ("wmin", ctypes.c_uint32), ("wmax", ctypes.c_uint32), ("kind", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class OcclusionParams(ctypes.Structure):
    """Mirror of dcmt_occlusion_params (include/dcmt.h), 20 bytes."""
    _fields_ = [("rx", ctypes.c_int32), ("ry", ctypes.c_int32), ("tol_code", ctypes.c_int32), ("valid_thresh", ctypes.c_float),
                ("max_depth", ctypes.c_float)]


class SupportParams(ctypes.Structure):
    """Mirror of dcmt_support_params (include/dcmt.h), 12 bytes."""
    _fields_ = [("max_radius", ctypes.c_int32), ("valid_thresh", ctypes.c_float), ("max_depth", ctypes.c_float)]


JOINT_FILL, JOINT_SMOOTH = 1, 2          # DCMT_JOINT_FILL, DCMT_JOINT_SMOOTH


class JointParams(ctypes.Structure):
    """Mirror of dcmt_joint_params (include/dcmt.h), 20 bytes."""
    _fields_ = [("radius", ctypes.c_int32), ("flags", ctypes.c_uint32), ("min_weight", ctypes.c_uint32), ("valid_thresh", ctypes.c_float),
                ("max_depth", ctypes.c_float)]


class JointTables(ctypes.Structure):
    """Mirror of dcmt_joint_tables (include/dcmt.h), 1792 bytes."""
    _fields_ = [("w_space", ctypes.c_uint16 * 128), ("w_guide", ctypes.c_uint16 * 768)]


class NormalsParams(ctypes.Structure):
    """Mirror of dcmt_normals_params (include/dcmt.h), 12 bytes."""
    _fields_ = [("min_plane_dist", ctypes.c_float), ("valid_thresh", ctypes.c_float), ("max_depth", ctypes.c_float)]


class CropSrc(ctypes.Structure):
    """Mirror of dcmt_crop_src (include/dcmt.h): one frame's record of dcmt_crop_frames_dev, 32 bytes."""
    _fields_ = [("offset", ctypes.c_uint64), ("row_stride", ctypes.c_uint32), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
                ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class RectifyCalib(ctypes.Structure):
    """Mirror of dcmt_rectify_calib (include/dcmt.h): one camera's record of dcmt_rectify_map_dev, 22 doubles."""
    _fields_ = [("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double),
                ("k1", ctypes.c_double), ("k2", ctypes.c_double), ("p1", ctypes.c_double), ("p2", ctypes.c_double), ("k3", ctypes.c_double),
                ("R", ctypes.c_double * 9),
                ("fxp", ctypes.c_double), ("fyp", ctypes.c_double), ("cxp", ctypes.c_double), ("cyp", ctypes.c_double)]


def nearest_name(twin: str) -> str:
    """The nearest-wins form of a last-wins scatter entry point: dcmt_project_points[_calib]_dev -> dcmt_project_points_nearest[_calib]_dev,
    likewise dcmt_reproject_depth*; the host forms gain the suffix."""
    for stem in ("dcmt_project_points", "dcmt_reproject_depth"):
        if twin.startswith(stem):
            return stem + "_nearest" + twin[len(stem):]
    raise ValueError(twin)


def build(force: bool = False) -> str:
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h"))]
    root = os.path.dirname(os.path.dirname(_CSRC))
    srcs += [os.path.join(root, "include", "dcmt.h")]
    stale = force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(s) for s in srcs)
    if stale:
        r = subprocess.run(["make", "-C", _CSRC, "-B", "libdcmt_hip.so"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("building libdcmt_hip.so failed:\n" + r.stdout + r.stderr)
    return LIB_PATH


_lib = None


def _share_hip_runtime_with_torch() -> None:
    """One HIP runtime per process.  The PyTorch wheel bundles its own libamdhip64.so (SONAME
    libamdhip64.so.7, found through its RPATH); libdcmt_hip.so needs libamdhip64.so.7 too.  If
    the system copy were loaded for us and the bundled one for torch, two HIP/HSA runtimes
    would fight over the device ("No HIP GPUs are available").  Loading torch's copy first
    makes the dynamic linker resolve our NEEDED entry to it by SONAME; a later `import torch`
    finds the same file.  Without torch installed the system runtime is used."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        _share_hip_runtime_with_torch()
        L = ctypes.CDLL(LIB_PATH)
        vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        pp = ctypes.POINTER(Params)
        u8p = ctypes.POINTER(ctypes.c_uint8)
        ip = ctypes.POINTER(ctypes.c_int)
        L.dcmt_device_count.argtypes = []
        L.dcmt_create.argtypes = [i, i, i, i, ctypes.POINTER(vp)]
        L.dcmt_destroy.argtypes = [vp]
        L.dcmt_destroy.restype = None
        L.dcmt_default_params.argtypes = [pp]
        L.dcmt_default_params.restype = None
        L.dcmt_k0_as_compiled.argtypes = [u8p]
        L.dcmt_k0_as_compiled.restype = None
        L.dcmt_k0_diamond.argtypes = [u8p]
        L.dcmt_k0_diamond.restype = None
        L.dcmt_complete_f32.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, i, i, pp]
        L.dcmt_complete_f32_dev.argtypes = [vp, vp, vp, i, i, i, pp, vp]
        L.dcmt_complete_labeled_f32.argtypes = [vp, vp, sz, sz, vp, sz, sz, i, vp, sz, sz, i, i, i, pp, i]
        L.dcmt_complete_labeled_f32_dev.argtypes = [vp, vp, vp, i, vp, i, i, i, pp, i, vp]
        L.dcmt_complete_u16_dev.argtypes = [vp, vp, ctypes.c_float, vp, i, i, i, pp, vp]
        L.dcmt_project_points_dev.argtypes = [vp, vp, vp, i, i, vp, vp, vp, i, i, vp]
        L.dcmt_default_stereo_params.argtypes = [vp]
        L.dcmt_default_stereo_params.restype = None
        L.dcmt_stereo_refine_dev.argtypes = [vp, vp, vp, vp, vp, i, i, i, vp, vp]
        L.dcmt_project_points.argtypes = [vp, vp, i, vp, vp, vp, sz, i, i]
        L.dcmt_slic_labels.argtypes = [vp, vp, sz, i, i, i, i, vp, vp]
        L.dcmt_stereo_refine.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, sz, i, i, vp]
        L.dcmt_slic_num_centers.argtypes = [i, i, i]
        L.dcmt_slic_connectivity_max_labels.argtypes = [i, i, i]
        L.dcmt_slic_connectivity_dev.argtypes = [vp, vp, i, i, i, i, vp, vp, vp]
        L.dcmt_slic_connectivity.argtypes = [vp, vp, sz, i, i, i, vp, sz, vp]
        L.dcmt_slic_contours_dev.argtypes = [vp, vp, i, i, i, vp, vp, vp, vp]
        L.dcmt_slic_cluster_means_dev.argtypes = [vp, vp, i, i, i, i, vp, vp, vp]
        L.dcmt_slic_contours.argtypes = [vp, vp, sz, i, i, vp, sz, vp, vp, sz]
        L.dcmt_slic_cluster_means.argtypes = [vp, vp, sz, i, i, i, vp, sz, vp]
        f32 = ctypes.c_float
        L.dcmt_evaluate_dev.argtypes = [vp, vp, vp, i, i, i, f32, i, vp, vp]
        L.dcmt_evaluate_u16_dev.argtypes = [vp, vp, f32, vp, i, i, i, f32, i, vp, vp]
        L.dcmt_evaluate.argtypes = [vp, vp, sz, vp, sz, i, i, f32, i, ctypes.POINTER(EvalFrame)]
        L.dcmt_colorize_dev.argtypes = [vp, vp, i, i, i, vp, vp]
        L.dcmt_colorize.argtypes = [vp, vp, sz, i, i, vp, sz]
        L.dcmt_colormap_jet.argtypes = [vp]
        L.dcmt_colormap_jet.restype = None
        i64 = ctypes.c_int64
        L.dcmt_default_cloud_params.argtypes = [vp]
        L.dcmt_default_cloud_params.restype = None
        L.dcmt_depth_to_cloud_dev.argtypes = [vp, vp, vp, i, i, i, vp, vp, i64, vp, vp]
        L.dcmt_depth_to_cloud.argtypes = [vp, vp, sz, vp, sz, i, i, vp, vp, i64, ctypes.POINTER(i64)]
        L.dcmt_gaussian5_dev.argtypes = [vp, vp, vp, i, i, i, vp]
        L.dcmt_gaussian5.argtypes = [vp, vp, sz, vp, sz, i, i]
        L.dcmt_gaussian5_valid_dev.argtypes = [vp, vp, vp, i, i, i, f32, vp]
        L.dcmt_gaussian5_valid.argtypes = [vp, vp, sz, vp, sz, i, i, f32]
        L.dcmt_bilateral5_dev.argtypes = [vp, vp, vp, i, i, i, f32, f32, vp]
        L.dcmt_bilateral5.argtypes = [vp, vp, sz, vp, sz, i, i, f32, f32]
        L.dcmt_default_reproject_params.argtypes = [vp]
        L.dcmt_default_reproject_params.restype = None
        L.dcmt_reproject_depth_dev.argtypes = [vp, vp, i, i, i, vp, vp, i, i, vp]
        L.dcmt_reproject_depth.argtypes = [vp, vp, sz, i, i, vp, vp, sz, i, i]
        L.dcmt_bgr_convert_dev.argtypes = [vp, vp, i, i, i, vp, vp, vp]
        L.dcmt_bgr_convert.argtypes = [vp, vp, sz, i, i, vp, sz, vp, sz]
        L.dcmt_lab_tables.argtypes = [vp, vp, vp]
        L.dcmt_lab_tables.restype = None
        L.dcmt_project_points_calib_dev.argtypes = [vp, vp, vp, i, i, vp, vp, i, i, vp]
        L.dcmt_depth_to_cloud_calib_dev.argtypes = [vp, vp, vp, i, i, i, vp, vp, i64, vp, vp]
        L.dcmt_reproject_depth_calib_dev.argtypes = [vp, vp, i, i, i, vp, vp, i, i, vp]
        L.dcmt_stereo_refine_calib_dev.argtypes = [vp, vp, vp, vp, vp, i, i, i, vp, vp, vp]
        L.dcmt_crop_frames_dev.argtypes = [vp, vp, sz, vp, i, vp, i, i, i, vp]
        L.dcmt_depth_to_u16_dev.argtypes = [vp, vp, f32, vp, i, i, i, vp]
        L.dcmt_depth_to_u16.argtypes = [vp, vp, sz, f32, vp, sz, i, i]
        L.dcmt_default_photo_error_params.argtypes = [vp]
        L.dcmt_default_photo_error_params.restype = None
        L.dcmt_photo_error_dev.argtypes = [vp, vp, vp, vp, i, i, i, vp, vp, vp, vp]
        L.dcmt_photo_error_calib_dev.argtypes = [vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp]
        L.dcmt_photo_error.argtypes = [vp, vp, sz, vp, sz, vp, sz, i, i, vp, vp, sz, vp]
        L.dcmt_default_sgm_params.argtypes = [vp]
        L.dcmt_default_sgm_params.restype = None
        L.dcmt_sgm_workspace_bytes.argtypes = [i, i, i, i]
        L.dcmt_sgm_workspace_bytes.restype = sz
        L.dcmt_sgm_dev.argtypes = [vp, vp, vp, vp, vp, i, i, i, vp, vp, sz, vp]
        L.dcmt_sgm.argtypes = [vp, vp, sz, vp, sz, i, i, vp, vp, sz, vp, sz]
        L.dcmt_sgm_paths_dev.argtypes = [vp, vp, vp, vp, vp, i, i, i, vp, i, vp, sz, vp]
        L.dcmt_sgm_paths.argtypes = [vp, vp, sz, vp, sz, i, i, vp, vp, sz, vp, sz, i]
        L.dcmt_sgm_guided_dev.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, vp, i, i, i, vp, sz, vp]
        L.dcmt_sgm_guided.argtypes = [vp, vp, sz, vp, sz, vp, sz, i, i, vp, vp, sz, vp, sz, i, i, i]
        L.dcmt_sgm_cost_dev.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, vp, i, i, i, i, vp, sz, vp]
        L.dcmt_sgm_cost.argtypes = [vp, vp, sz, vp, sz, vp, sz, i, i, vp, vp, sz, vp, sz, i, i, i, i]
        L.dcmt_default_speckle_params.argtypes = [vp]
        L.dcmt_default_speckle_params.restype = None
        L.dcmt_filter_speckles_dev.argtypes = [vp, vp, vp, vp, i, i, i, vp, vp, vp]
        L.dcmt_filter_speckles.argtypes = [vp, vp, sz, vp, sz, vp, sz, i, i, vp, vp]
        L.dcmt_rectify_map_dev.argtypes = [vp, vp, i, i, i, vp, vp]
        L.dcmt_rectify_dev.argtypes = [vp, vp, i, i, i, vp, i, vp, ctypes.c_uint32, vp, i, i, i, vp]
        L.dcmt_rectify.argtypes = [vp, vp, sz, i, i, i, vp, vp, sz, i, i]
        L.dcmt_default_planes_params.argtypes = [vp]
        L.dcmt_default_planes_params.restype = None
        L.dcmt_superpixel_planes_max_labels.argtypes = [i, i, i, i]
        L.dcmt_superpixel_planes_dev.argtypes = [vp, vp, vp, i, i, i, i, vp, vp, vp, vp]
        L.dcmt_superpixel_planes.argtypes = [vp, vp, sz, vp, sz, i, i, i, vp, vp, sz, vp]
        L.dcmt_default_occlusion_params.argtypes = [vp]
        L.dcmt_default_occlusion_params.restype = None
        L.dcmt_sparse_occlusion_dev.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp]
        L.dcmt_sparse_occlusion_u16_dev.argtypes = [vp, vp, ctypes.c_float, vp, i, i, i, vp, vp, vp]
        L.dcmt_sparse_occlusion.argtypes = [vp, vp, sz, vp, sz, i, i, vp, vp]
        L.dcmt_default_support_params.argtypes = [vp]
        L.dcmt_default_support_params.restype = None
        L.dcmt_support_distance_dev.argtypes = [vp, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp]
        L.dcmt_support_distance_u16_dev.argtypes = [vp, vp, ctypes.c_float, vp, vp, vp, vp, i, i, i, vp, vp, vp]
        L.dcmt_support_distance.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz, i, i, vp, vp]
        L.dcmt_default_joint_params.argtypes = [vp]
        L.dcmt_default_joint_params.restype = None
        L.dcmt_make_joint_tables.argtypes = [i, ctypes.c_double, ctypes.c_double, vp]
        L.dcmt_joint_bilateral_dev.argtypes = [vp, vp, vp, i, vp, vp, i, i, i, vp, vp, vp]
        L.dcmt_joint_bilateral.argtypes = [vp, vp, sz, vp, sz, i, vp, vp, sz, i, i, vp, vp]
        L.dcmt_default_normals_params.argtypes = [vp]
        L.dcmt_default_normals_params.restype = None
        L.dcmt_depth_normals_dev.argtypes = [vp, vp, i, i, i, vp, vp, vp, vp, vp, vp]
        L.dcmt_depth_normals_calib_dev.argtypes = [vp, vp, i, i, i, vp, vp, vp, vp, vp, vp]
        L.dcmt_depth_normals.argtypes = [vp, vp, sz, i, i, vp, vp, vp, sz, vp, sz, vp]
        for twin in ("dcmt_project_points_dev", "dcmt_project_points_calib_dev", "dcmt_reproject_depth_dev", "dcmt_reproject_depth_calib_dev",
                     "dcmt_project_points", "dcmt_reproject_depth"):           # the nearest-wins forms take their twins' arguments
            getattr(L, nearest_name(twin)).argtypes = getattr(L, twin).argtypes
        L.dcmt_slic_labels_dev.argtypes = [vp, vp, i, i, i, i, i, vp, vp, vp]
        L.dcmt_last_fill_iters.argtypes = [vp, ip, i]
        L.dcmt_last_holes_after_extend.argtypes = [vp, ip, i]
        L.dcmt_strerror.argtypes = [i]
        L.dcmt_strerror.restype = ctypes.c_char_p
        L.dcmt_last_hip_error.argtypes = [vp]
        L.dcmt_last_path.argtypes = [vp]
        L.dcmt_last_path.restype = ctypes.c_char_p
        L.dcmt_set_kernel_timing.argtypes = [vp, i]
        L.dcmt_last_kernel_times.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.dcmt_version.argtypes = []
        _lib = L
    return _lib


def strerror(status: int) -> str:
    return lib().dcmt_strerror(status).decode()
