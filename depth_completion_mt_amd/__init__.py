"""MI355X-native (gfx950) morphological depth completion: the `img_completion` cascade of
PatrizioPerugini/depth_completion_MT as hand-written HIP kernels behind a C ABI.

    from depth_completion_mt_amd import img_completion, interpolate_with_superpixels, Context
"""
from .api import (CLOUD_DTYPE, Context, DcmtError, bgr_to_gray, bgr_to_lab, eval_summary, evaluate_performance, img_completion,  # noqa: F401
                  interpolate_with_superpixels, make_cloud_params, make_params, make_reproject_params, read_pcd, reference_performance,
                  reproject_pc, reproject_pc_colors, to_color_image, unrectify_sol, write_pcd,
                  calib_to_device, make_cloud_calib, make_project_calib, make_reproject_calib, make_stereo_calib,
                  depth_to_u16, kitti_crop_origin, make_crop_table, pack_ragged, bilateral_filter5,
                  slic_connectivity_max_labels, slic_enforce_connectivity, slic_display_contours,
                  slic_colour_with_cluster_means, get_initial_error, make_photo_error_params, make_sgm_params,
                  sgm_workspace_bytes, stereo_sgm, make_speckle_params, filter_speckles,
                  RECTIFY_CALIB_DTYPE, make_rectify_calib, undistort_rectify,
                  PLANE_FIT_DTYPE, make_planes_params, fit_superpixel_planes, superpixel_planes_max_labels,
                  make_occlusion_params, filter_occluded_returns, make_support_params, distance_to_returns, trust_mask,
                  JOINT_TABLES_DTYPE, make_joint_params, make_joint_tables, joint_bilateral_fill,
                  make_normals_params, make_normals_calib, depth_normals, filter_flying_pixels, reproject_pc_normals)
from . import synth  # noqa: F401

__all__ = ["Context", "DcmtError", "eval_summary", "evaluate_performance", "img_completion", "interpolate_with_superpixels",
           "make_params", "reference_performance", "synth", "to_color_image", "JET_BGR", "CLOUD_DTYPE", "make_cloud_params",
           "reproject_pc_colors", "reproject_pc", "write_pcd", "read_pcd", "make_reproject_params", "unrectify_sol",
           "bgr_to_lab", "bgr_to_gray", "make_project_calib", "make_cloud_calib", "make_reproject_calib", "make_stereo_calib",
           "calib_to_device", "depth_to_u16", "kitti_crop_origin", "make_crop_table", "pack_ragged",
           "bilateral_filter5", "slic_connectivity_max_labels", "slic_enforce_connectivity",
           "slic_display_contours", "slic_colour_with_cluster_means", "get_initial_error", "make_photo_error_params",
           "make_sgm_params", "sgm_workspace_bytes", "stereo_sgm", "make_speckle_params", "filter_speckles",
           "RECTIFY_CALIB_DTYPE", "make_rectify_calib", "undistort_rectify",
           "PLANE_FIT_DTYPE", "make_planes_params", "fit_superpixel_planes", "superpixel_planes_max_labels",
           "make_occlusion_params", "filter_occluded_returns", "make_support_params", "distance_to_returns", "trust_mask",
           "JOINT_TABLES_DTYPE", "make_joint_params", "make_joint_tables", "joint_bilateral_fill",
           "make_normals_params", "make_normals_calib", "depth_normals", "filter_flying_pixels", "reproject_pc_normals"]


def __getattr__(name):
    if name == "JET_BGR":                        # loads the library on first use (api.JET_BGR)
        from . import api
        return api.JET_BGR
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
