// dcmt_cloud.hip -- the kernels of dcmt_kernels_cloud.h, dcmt_kernels_reproject.h, dcmt_kernels_nearest.h, dcmt_kernels_bgr.h and dcmt_kernels_crop.h, a code
// object of their own, and the entry points that launch them: dcmt_depth_to_cloud_dev, dcmt_gaussian5_dev, dcmt_reproject_depth_dev,
// the four nearest-wins scatter calls (dcmt_kernels_nearest.h: dcmt_project_points_nearest*_dev, dcmt_reproject_depth_nearest*_dev),
// dcmt_bgr_convert_dev, dcmt_crop_frames_dev, dcmt_depth_to_u16_dev, dcmt_bilateral5_dev (dcmt_kernels_bilateral.h; the cascade's bilateral finish launches the same kernel through bilateral5_enqueue),
// dcmt_slic_connectivity_dev (dcmt_kernels_connect.h), dcmt_filter_speckles_dev (dcmt_kernels_speckle.h), dcmt_slic_contours_dev and dcmt_slic_cluster_means_dev (dcmt_kernels_contour.h), dcmt_superpixel_planes_dev (dcmt_kernels_planes.h), dcmt_sparse_occlusion_dev and dcmt_sparse_occlusion_u16_dev (dcmt_kernels_occlusion.h), dcmt_support_distance_dev and dcmt_support_distance_u16_dev (dcmt_kernels_support.h), dcmt_joint_bilateral_dev (dcmt_kernels_joint.h), dcmt_depth_normals_dev and dcmt_depth_normals_calib_dev (dcmt_kernels_normals.h),
// dcmt_photo_error_dev (dcmt_kernels_photo.h), the defaults of their parameter structs and dcmt_lab_tables.  A *_calib_dev entry point
// shares its one launch sequence with the uniform entry point beside it: the calibration source (one record by value, or the device
// table) is the kernels' template type.  The context and the checks they share with dcmt.hip come from dcmt_ctx.h; their single-frame
// host variants are in dcmt_host.hip.
#include <algorithm>
#include <cmath>

#include "dcmt_chunks.h"
#include "dcmt_plan_side.h"
#include "dcmt_ctx.h"
#include "dcmt_kernels_bgr.h"
#include "dcmt_kernels_cloud.h"
#include "dcmt_kernels_crop.h"
#include "dcmt_kernels_nearest.h"
#include "dcmt_kernels_reproject.h"
#include "dcmt_kernels_bilateral.h"
#include "dcmt_kernels_connect.h"
#include "dcmt_kernels_speckle.h"
#include "dcmt_kernels_contour.h"
#include "dcmt_kernels_photo.h"
#include "dcmt_kernels_planes.h"
#include "dcmt_kernels_occlusion.h"
#include "dcmt_kernels_support.h"
#include "dcmt_kernels_joint.h"
#include "dcmt_kernels_normals.h"

using namespace dcmt;

extern "C" {

void dcmt_default_cloud_params(dcmt_cloud_params* p)
{
    if (!p) return;
    p->fx = 9.597910e+02;   // main_sl.cpp:927-930
    p->fy = 9.569251e+02;
    p->cx = 6.960217e+02;
    p->cy = 2.241806e+02;
}

}  // extern "C"

// per-wave counts, their exclusive scan in one workgroup, then the scatter (dcmt_kernels_cloud.h).  params: the host's one set of
// intrinsics (dcmt_depth_to_cloud_dev) or null with d_table, the device's [batch] (dcmt_depth_to_cloud_calib_dev)
static int depth_to_cloud(dcmt_ctx* ctx, const float* d_depth, const uint8_t* d_bgr, int rows, int cols, int batch,
                          const dcmt_cloud_params* params, const dcmt_cloud_params* d_table, dcmt_cloud_point* d_points, int64_t capacity,
                          int32_t* d_offsets, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !d_depth || !d_points || !d_offsets || (!params && !d_table)) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    if (capacity < 0 || (int64_t)batch * rows * cols > (int64_t)INT32_MAX) return DCMT_E_INVALID;
    if ((uintptr_t)d_depth % 4 != 0 || (uintptr_t)d_points % 16 != 0 || (uintptr_t)d_offsets % 4 != 0) return DCMT_E_INVALID;
    if (params && !intrinsics_ok(params->fx, params->fy, params->cx, params->cy)) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = (uint32_t)rows * (uint32_t)cols, room = (uint32_t)std::min<int64_t>(capacity, INT32_MAX);
    if (d_table && (!plan::calib_table_aligned((uintptr_t)d_table, 8) || !plan::calib_table_clear_of((uintptr_t)d_table, sizeof *d_table, batch, (uintptr_t)d_points, sizeof(dcmt_cloud_point) * (size_t)room) ||
                    !plan::calib_table_clear_of((uintptr_t)d_table, sizeof *d_table, batch, (uintptr_t)d_offsets, sizeof(int32_t) * ((size_t)batch + 1))))
        return DCMT_E_INVALID;
    const uint32_t chunks = eval_chunks(n), groups = eval_chunk_groups(n);
    const dim3 grid(chunks, batch);
    const uint32_t per = chunks * kCloudWaves;      // slab: [batch][chunks][kCloudWaves] uint32
    uint4* points = reinterpret_cast<uint4*>(d_points);
    const auto launch = [&](auto src) {                // CloudK or CloudTable
        using Src = decltype(src);
        hipLaunchKernelGGL(k_cloud_count<Src>, grid, dim3(kCloudThreads), 0, st, d_depth, n, groups, ctx->cloud_slab, src);
        hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(kCloudScanThreads), 0, st, ctx->cloud_slab, per * (uint32_t)batch, per, (uint32_t)batch, d_offsets);
        with_value<true, false>(d_bgr != nullptr, [&](auto color) {
            hipLaunchKernelGGL((k_cloud_scatter<decltype(color)::value, Src>), grid, dim3(kCloudThreads), 0, st, d_depth, d_bgr, n, groups, (uint32_t)cols, src,
                               ctx->cloud_slab, points, room);
        });
    };
    if (d_table) launch(CloudTable{d_table});
    else launch(CloudK{params->fx, params->fy, params->cx, params->cy});
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

// what the uniform reprojection calls refuse in their host record: a non-finite intrinsic or matrix entry (of the rows that are read),
// fx or fy zero
static bool reproject_params_ok(const dcmt_reproject_params* params)
{
    if (!intrinsics_ok(params->fx, params->fy, params->cx, params->cy)) return false;
    for (int i = 0; i < 12; ++i) if (!finite_bits(params->M[i])) return false;         // (M's 4th row and K's 3rd are never read)
    for (int i = 0; i < 6; ++i) if (!finite_bits(params->K[i])) return false;
    return true;
}

// ... and the record as the kernels take it
static ReprojK reproject_k(const dcmt_reproject_params* params)
{
    ReprojK k;
    k.fx = params->fx; k.fy = params->fy; k.cx = params->cx; k.cy = params->cy;
    std::memcpy(k.M, params->M, sizeof k.M);
    std::memcpy(k.K, params->K, sizeof k.K);
    return k;
}

// k_reproject_scatter, k_reproject_resolve (dcmt_kernels_reproject.h) on the context's winner plane (winner_generation, dcmt_ctx.h);
// params / d_table as for depth_to_cloud
static int reproject_depth(dcmt_ctx* ctx, const float* d_depth, int rows, int cols, int batch, const dcmt_reproject_params* params,
                           const dcmt_reproject_params* d_table, float* d_out, int out_rows, int out_cols, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !d_depth || !d_out || (!params && !d_table)) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch) || !dims_ok(ctx, out_rows, out_cols, batch)) return DCMT_E_INVALID;
    if ((uintptr_t)d_depth % 4 != 0 || (uintptr_t)d_out % 4 != 0) return DCMT_E_INVALID;
    if (params && !reproject_params_ok(params)) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = (uint32_t)rows * (uint32_t)cols, dst_n = (uint32_t)out_rows * (uint32_t)out_cols;
    const size_t n_px = (size_t)batch * dst_n;
    if (plan::ranges_overlap((uintptr_t)d_depth, sizeof(float) * n * batch, (uintptr_t)d_out, sizeof(float) * n_px)) return DCMT_E_INVALID;
    if (d_table && (!plan::calib_table_aligned((uintptr_t)d_table, 8) || !plan::calib_table_clear_of((uintptr_t)d_table, sizeof *d_table, batch, (uintptr_t)d_out, sizeof(float) * n_px)))
        return DCMT_E_INVALID;
    unsigned gen_tag = 0;
    const int rc = winner_generation(ctx, n_px, n, st, &gen_tag);
    if (rc != DCMT_OK) return rc;
    const dim3 scatter_grid((n + kReprojectPxPerWg - 1) / kReprojectPxPerWg, batch);
    const auto launch = [&](auto src) {                // ReprojK or ReprojTable
        using Src = decltype(src);
        hipLaunchKernelGGL(k_reproject_scatter<Src>, scatter_grid, dim3(256), 0, st, d_depth, n, (uint32_t)cols, src, ctx->winner,
                           (uint32_t)out_rows, (uint32_t)out_cols, gen_tag);
        with_value<4, 2, 1>(plan::resolve_vec(n_px, (uintptr_t)d_out), [&](auto v) {
            hipLaunchKernelGGL((k_reproject_resolve<decltype(v)::value, Src>), dim3((unsigned)((n_px / v + 255) / 256)), dim3(256), 0, st, d_depth, n, (uint32_t)cols,
                               src, ctx->winner, d_out, dst_n, n_px, gen_tag, ctx->winner_bits);
        });
    };
    if (d_table) launch(ReprojTable{d_table});
    else launch(reproject_k(params));
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

extern "C" {

int dcmt_depth_to_cloud_dev(dcmt_ctx* ctx, const float* d_depth, const uint8_t* d_bgr, int rows, int cols, int batch,
                            const dcmt_cloud_params* params, dcmt_cloud_point* d_points, int64_t capacity, int32_t* d_offsets, void* stream)
{
    if (!params) return DCMT_E_INVALID;
    return depth_to_cloud(ctx, d_depth, d_bgr, rows, cols, batch, params, nullptr, d_points, capacity, d_offsets, stream);
}

int dcmt_depth_to_cloud_calib_dev(dcmt_ctx* ctx, const float* d_depth, const uint8_t* d_bgr, int rows, int cols, int batch,
                                  const dcmt_cloud_params* d_params, dcmt_cloud_point* d_points, int64_t capacity, int32_t* d_offsets, void* stream)
{
    if (!d_params) return DCMT_E_INVALID;
    return depth_to_cloud(ctx, d_depth, d_bgr, rows, cols, batch, nullptr, d_params, d_points, capacity, d_offsets, stream);
}

// one streaming kernel (k_gauss5, dcmt_kernels_cloud.h), whose src and dst must not overlap: an in-place call writes to pp[0]
// (scratch every cascade call rewrites before it reads it) and copies the result over the source
int dcmt_gaussian5_dev(dcmt_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int batch, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !d_src || !d_dst) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    if ((uintptr_t)d_src % 4 != 0 || (uintptr_t)d_dst % 4 != 0) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = sizeof(float) * (size_t)batch * rows * cols;
    const bool in_place = d_dst == d_src;
    if (!in_place && plan::ranges_overlap((uintptr_t)d_src, bytes, (uintptr_t)d_dst, bytes)) return DCMT_E_INVALID;
    float* out = in_place ? ctx->pp[0] : d_dst;
    const plan::GaussPlan pl = plan::plan_gauss5(rows, cols, batch);
    hipLaunchKernelGGL((k_gauss5<false, false>), dim3(pl.grid_x, batch), dim3(256), 0, st, d_src, out, rows, cols, pl.strips, pl.bands, pl.band_rows,
                       0.0f, 0.0f);
    DCMT_HIP(ctx, hipGetLastError());
    if (in_place) DCMT_HIP(ctx, hipMemcpyAsync(d_dst, out, bytes, hipMemcpyDeviceToDevice, st));
    return DCMT_OK;
}

// as dcmt_gaussian5_dev, with k_gauss5<VALID>
int dcmt_gaussian5_valid_dev(dcmt_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int batch, float valid_thresh, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !d_src || !d_dst) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    if ((uintptr_t)d_src % 4 != 0 || (uintptr_t)d_dst % 4 != 0) return DCMT_E_INVALID;
    // as dcmt_params.valid_thresh (check_params): finite, sign clear, not zero -- on its bits (-ffinite-math-only)
    uint32_t tb;
    std::memcpy(&tb, &valid_thresh, sizeof tb);
    if ((tb & 0x7f800000u) == 0x7f800000u || (tb >> 31) != 0 || (tb << 1) == 0) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = sizeof(float) * (size_t)batch * rows * cols;
    const bool in_place = d_dst == d_src;
    if (!in_place && plan::ranges_overlap((uintptr_t)d_src, bytes, (uintptr_t)d_dst, bytes)) return DCMT_E_INVALID;
    float* out = in_place ? ctx->pp[0] : d_dst;
    DCMT_TRY(gauss5_valid_enqueue(ctx, d_src, out, rows, cols, batch, valid_thresh, false, 0.0f, st));
    if (in_place) DCMT_HIP(ctx, hipMemcpyAsync(d_dst, out, bytes, hipMemcpyDeviceToDevice, st));
    return DCMT_OK;
}

void dcmt_default_reproject_params(dcmt_reproject_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->fx = 9.597910e+02;   // main_sl.cpp:969-972
    p->fy = 9.569251e+02;
    p->cx = 6.960217e+02;
    p->cy = 2.241806e+02;
    p->M[0] = p->M[5] = p->M[10] = p->M[15] = 1.0f;
    p->K[0] = 9.597910e+02f; p->K[2] = 6.960217e+02f;     // camera_mat, :974-976
    p->K[4] = 9.569251e+02f; p->K[5] = 2.241806e+02f;
    p->K[8] = 1.0f;
}

int dcmt_reproject_depth_dev(dcmt_ctx* ctx, const float* d_depth, int rows, int cols, int batch, const dcmt_reproject_params* params,
                             float* d_out, int out_rows, int out_cols, void* stream)
{
    if (!params) return DCMT_E_INVALID;
    return reproject_depth(ctx, d_depth, rows, cols, batch, params, nullptr, d_out, out_rows, out_cols, stream);
}

int dcmt_reproject_depth_calib_dev(dcmt_ctx* ctx, const float* d_depth, int rows, int cols, int batch, const dcmt_reproject_params* d_params,
                                   float* d_out, int out_rows, int out_cols, void* stream)
{
    if (!d_params) return DCMT_E_INVALID;
    return reproject_depth(ctx, d_depth, rows, cols, batch, nullptr, d_params, d_out, out_rows, out_cols, stream);
}

}  // extern "C"

// The nearest-wins calls (dcmt_kernels_nearest.h): clear the output, scatter keys into it, fix it up in place -- what the plan says
// (plan_project_nearest / plan_reproject_nearest, which also hold the checks on the buffers).  Nothing of the context is read or
// written but its device and its limits: no scratch, no state, no allocation.
template <typename Scatter>
static int nearest_launch(dcmt_ctx* ctx, const plan::NearestPlan& pl, float* d_out, hipStream_t st, Scatter scatter)
{
    unsigned* keys = reinterpret_cast<unsigned*>(d_out);
    DCMT_HIP(ctx, hipMemsetAsync(d_out, 0, pl.clear_bytes, st));
    if (pl.scatter_x > 0) scatter(dim3(pl.scatter_x, pl.scatter_y), keys);
    with_value<4, 2, 1>(pl.vec, [&](auto v) {
        hipLaunchKernelGGL(k_nearest_fixup<decltype(v)::value>, dim3(pl.fixup_x), dim3(256), 0, st, keys, pl.n_px);
    });
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

// T, P / d_table as for dcmt.hip's project_points
static int project_points_nearest(dcmt_ctx* ctx, const float* d_points, const int32_t* d_offsets, int n_points, int batch, const float* T,
                                  const float* P, const dcmt_project_calib* d_table, float* d_sparse, int rows, int cols, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || (!d_table && (!T || !P))) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const plan::NearestPlan pl = plan::plan_project_nearest(rows, cols, batch, n_points, (uintptr_t)d_points, (uintptr_t)d_offsets, d_table != nullptr,
                                                            (uintptr_t)d_table, (uintptr_t)d_sparse);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const auto launch = [&](auto src) {                // ProjMats or ProjTable
        return nearest_launch(ctx, pl, d_sparse, st, [&](dim3 grid, unsigned* keys) {
            hipLaunchKernelGGL(k_project_nearest_scatter<decltype(src)>, grid, dim3(256), 0, st, d_points, d_offsets, n_points, batch, src, keys, rows, cols);
        });
    };
    return d_table ? launch(ProjTable{d_table}) : launch(proj_mats(T, P));
}

// params / d_table as for reproject_depth
static int reproject_depth_nearest(dcmt_ctx* ctx, const float* d_depth, int rows, int cols, int batch, const dcmt_reproject_params* params,
                                   const dcmt_reproject_params* d_table, float* d_out, int out_rows, int out_cols, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || (!params && !d_table)) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch) || !dims_ok(ctx, out_rows, out_cols, batch)) return DCMT_E_INVALID;
    if (params && !reproject_params_ok(params)) return DCMT_E_INVALID;
    const plan::NearestPlan pl = plan::plan_reproject_nearest(rows, cols, out_rows, out_cols, batch, (uintptr_t)d_depth, d_table != nullptr,
                                                              (uintptr_t)d_table, (uintptr_t)d_out);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = (uint32_t)rows * (uint32_t)cols;
    const auto launch = [&](auto src) {                // ReprojK or ReprojTable
        return nearest_launch(ctx, pl, d_out, st, [&](dim3 grid, unsigned* keys) {
            hipLaunchKernelGGL(k_reproject_nearest_scatter<decltype(src)>, grid, dim3(256), 0, st, d_depth, n, (uint32_t)cols, src, keys, (uint32_t)out_rows,
                               (uint32_t)out_cols);
        });
    };
    return d_table ? launch(ReprojTable{d_table}) : launch(reproject_k(params));
}

extern "C" {

int dcmt_project_points_nearest_dev(dcmt_ctx* ctx, const float* d_points, const int32_t* d_offsets, int n_points, int batch,
                                    const float T[16], const float P[12], float* d_sparse, int rows, int cols, void* stream)
{
    if (!T || !P) return DCMT_E_INVALID;
    return project_points_nearest(ctx, d_points, d_offsets, n_points, batch, T, P, nullptr, d_sparse, rows, cols, stream);
}

int dcmt_project_points_nearest_calib_dev(dcmt_ctx* ctx, const float* d_points, const int32_t* d_offsets, int n_points, int batch,
                                          const dcmt_project_calib* d_calib, float* d_sparse, int rows, int cols, void* stream)
{
    if (!d_calib) return DCMT_E_INVALID;
    return project_points_nearest(ctx, d_points, d_offsets, n_points, batch, nullptr, nullptr, d_calib, d_sparse, rows, cols, stream);
}

int dcmt_reproject_depth_nearest_dev(dcmt_ctx* ctx, const float* d_depth, int rows, int cols, int batch, const dcmt_reproject_params* params,
                                     float* d_out, int out_rows, int out_cols, void* stream)
{
    if (!params) return DCMT_E_INVALID;
    return reproject_depth_nearest(ctx, d_depth, rows, cols, batch, params, nullptr, d_out, out_rows, out_cols, stream);
}

int dcmt_reproject_depth_nearest_calib_dev(dcmt_ctx* ctx, const float* d_depth, int rows, int cols, int batch, const dcmt_reproject_params* d_params,
                                           float* d_out, int out_rows, int out_cols, void* stream)
{
    if (!d_params) return DCMT_E_INVALID;
    return reproject_depth_nearest(ctx, d_depth, rows, cols, batch, nullptr, d_params, d_out, out_rows, out_cols, stream);
}

// k_bgr_convert (dcmt_kernels_bgr.h) over the batch as one flat run of pixels, a launch per segment (plan_bgr_convert)
int dcmt_bgr_convert_dev(dcmt_ctx* ctx, const uint8_t* d_bgr, int rows, int cols, int batch, uint8_t* d_lab, uint8_t* d_gray, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !d_bgr || (!d_lab && !d_gray)) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const plan::BgrPlan pl = plan::plan_bgr_convert((size_t)batch * rows * cols, (uintptr_t)d_bgr, (uintptr_t)d_lab, (uintptr_t)d_gray);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    for (size_t i = 0; i < pl.count; ++i) {
        const plan::BgrSegment sg = pl.segment(i);
        const uint8_t* src = d_bgr + 3 * sg.first;
        uint8_t* lab = d_lab ? d_lab + 3 * sg.first : nullptr;
        uint8_t* gray = d_gray ? d_gray + sg.first : nullptr;
        with_value<7, 6, 5, 3, 2, 1>((d_lab ? 1 : 0) | (d_gray ? 2 : 0) | (pl.aligned ? 4 : 0), [&](auto v) {
            constexpr int m = decltype(v)::value;
            hipLaunchKernelGGL((k_bgr_convert<(m & 1) != 0, (m & 2) != 0, (m & 4) != 0>), dim3(sg.grid), dim3(kBgrThreads), 0, st, src, sg.total, pl.passes, lab, gray);
        });
        DCMT_HIP(ctx, hipGetLastError());
    }
    return DCMT_OK;
}

// k_crop_frames (dcmt_kernels_crop.h): one launch, the frame's record read and tested by the kernel (plan_crop)
int dcmt_crop_frames_dev(dcmt_ctx* ctx, const void* d_src, size_t src_bytes, const dcmt_crop_src* d_table, int elem_bytes, void* d_dst,
                         int out_rows, int out_cols, int batch, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !d_src || !d_table || !d_dst) return DCMT_E_INVALID;
    if (!dims_ok(ctx, out_rows, out_cols, batch)) return DCMT_E_INVALID;
    const plan::CropPlan pl = plan::plan_crop(out_rows, out_cols, batch, elem_bytes, (uintptr_t)d_src, src_bytes, (uintptr_t)d_table, (uintptr_t)d_dst);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipLaunchKernelGGL(k_crop_frames, dim3(pl.grid_x, pl.grid_y), dim3(kCropThreads), 0, (hipStream_t)stream, (const uint8_t*)d_src, (uint64_t)src_bytes,
                       d_table, (uint32_t)elem_bytes, (uint8_t*)d_dst, (uint32_t)out_rows, (uint32_t)out_cols, pl.band);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

// k_depth_to_u16 (dcmt_kernels_crop.h) over the batch as one flat run of pixels, a launch per segment (plan_depth_to_u16)
int dcmt_depth_to_u16_dev(dcmt_ctx* ctx, const float* d_depth, float scale, uint16_t* d_out, int rows, int cols, int batch, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !d_depth || !d_out) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    volatile float sv = scale;                       // on the bits, read through memory (finite_bits): finite, sign clear, not zero
    const float sc = sv;
    uint32_t sb;
    std::memcpy(&sb, &sc, sizeof sb);
    if (!finite_bits(scale) || (sb >> 31) != 0 || (sb << 1) == 0) return DCMT_E_INVALID;
    const plan::U16Plan pl = plan::plan_depth_to_u16((size_t)batch * rows * cols, (uintptr_t)d_depth, (uintptr_t)d_out);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    for (size_t i = 0; i < pl.count; ++i) {
        const plan::U16Segment sg = pl.segment(i);
        if (pl.aligned) hipLaunchKernelGGL(k_depth_to_u16<true>, dim3(sg.grid), dim3(kU16Threads), 0, st, d_depth + sg.first, sg.total, scale, d_out + sg.first);
        else hipLaunchKernelGGL(k_depth_to_u16<false>, dim3(sg.grid), dim3(kU16Threads), 0, st, d_depth + sg.first, sg.total, scale, d_out + sg.first);
        DCMT_HIP(ctx, hipGetLastError());
    }
    return DCMT_OK;
}

void dcmt_lab_tables(uint16_t gamma[256], uint16_t cbrt[3072], int32_t coef[9])
{
    static const LabTables t = {{DCMT_LAB_GAMMA}, {DCMT_LAB_CBRT}};
    static const int32_t c[9] = {DCMT_LAB_COEF};
    if (gamma) std::memcpy(gamma, t.gamma, sizeof t.gamma);
    if (cbrt) std::memcpy(cbrt, t.cbrt, sizeof t.cbrt);
    if (coef) std::memcpy(coef, c, sizeof c);
}

}  // extern "C"

// ---- the bilateral finish (dcmt_kernels_bilateral.h) ---------------------------------------------------------------------------
namespace dcmt {

// the kernel's constants of (sigma_color, sigma_space); false for a sigma that is not finite and positive, or whose square leaves
// no finite f32 factor gc
static bool bilateral_k(float sigma_color, float sigma_space, BilK* k)
{
    if (!finite_bits(sigma_color) || !finite_bits(sigma_space) || !(sigma_color > 0.0f) || !(sigma_space > 0.0f)) return false;
    const float sc2 = sigma_color * sigma_color;
    if (!finite_bits(sc2) || !(sc2 > 0.0f)) return false;
    k->gc = -0.5f / sc2;
    if (!finite_bits(k->gc)) return false;
    const double gs = -0.5 / ((double)sigma_space * (double)sigma_space);
    k->ws1 = (float)std::exp(gs);
    k->ws2 = (float)std::exp(2.0 * gs);
    k->ws4 = (float)std::exp(4.0 * gs);
    return true;
}

// (dcmt_ctx.h)
int bilateral5_enqueue(dcmt_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int batch, float sigma_color, float sigma_space,
                       bool invert, float max_depth, float thr, hipStream_t st)
{
    BilK k;
    if (!bilateral_k(sigma_color, sigma_space, &k)) return DCMT_E_INVALID;
    const plan::GaussPlan pl = plan::plan_bilateral5(rows, cols, batch);
    const dim3 grid(pl.grid_x, batch);
    if (invert)
        hipLaunchKernelGGL(k_bilateral5<true>, grid, dim3(256), 0, st, d_src, d_dst, rows, cols, pl.strips, pl.bands, pl.band_rows, k, max_depth, thr);
    else
        hipLaunchKernelGGL(k_bilateral5<false>, grid, dim3(256), 0, st, d_src, d_dst, rows, cols, pl.strips, pl.bands, pl.band_rows, k, max_depth, thr);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

// (dcmt_ctx.h)
int gauss5_valid_enqueue(dcmt_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int batch, float thr, bool invert, float max_depth,
                         hipStream_t st)
{
    const plan::GaussPlan pl = plan::plan_gauss5(rows, cols, batch);
    const dim3 grid(pl.grid_x, batch);
    if (invert)
        hipLaunchKernelGGL((k_gauss5<true, true>), grid, dim3(256), 0, st, d_src, d_dst, rows, cols, pl.strips, pl.bands, pl.band_rows, thr, max_depth);
    else
        hipLaunchKernelGGL((k_gauss5<true, false>), grid, dim3(256), 0, st, d_src, d_dst, rows, cols, pl.strips, pl.bands, pl.band_rows, thr, max_depth);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

}  // namespace dcmt

extern "C" {

// as dcmt_gaussian5_dev: an in-place call writes to pp[0] and copies the result over the source
int dcmt_bilateral5_dev(dcmt_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int batch, float sigma_color, float sigma_space,
                        void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !d_src || !d_dst) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    if ((uintptr_t)d_src % 4 != 0 || (uintptr_t)d_dst % 4 != 0) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = sizeof(float) * (size_t)batch * rows * cols;
    const bool in_place = d_dst == d_src;
    if (!in_place && plan::ranges_overlap((uintptr_t)d_src, bytes, (uintptr_t)d_dst, bytes)) return DCMT_E_INVALID;
    float* out = in_place ? ctx->pp[0] : d_dst;
    DCMT_TRY(bilateral5_enqueue(ctx, d_src, out, rows, cols, batch, sigma_color, sigma_space, false, 0.0f, 0.0f, st));
    if (in_place) DCMT_HIP(ctx, hipMemcpyAsync(d_dst, out, bytes, hipMemcpyDeviceToDevice, st));
    return DCMT_OK;
}

}  // extern "C"

// ---- Slic::create_connectivity (dcmt_kernels_connect.h) -------------------------------------------------------------------------
namespace dcmt {

// The first three stages of a component labelling on the planes A and B: the tile-local kernel, the border kernel where a frame is
// more than one tile, k_conn_flatten.  rel: what the two kernels of a relation take between kbits and the planes.
template <class Local, class Border, class Src, class... Rel>
static void conn_label_enqueue(Local local, Border border, const ConnGeom& g, const Src* src, uint32_t rows, uint32_t cols, int batch, uint32_t* A,
                               uint32_t* B, hipStream_t st, Rel... rel)
{
    hipLaunchKernelGGL(local, dim3(g.local_x, batch), dim3(256), 0, st, src, rows, cols, g.tiles_x, g.kbits, rel..., A, B);
    if (g.border_x > 0) hipLaunchKernelGGL(border, dim3(g.border_x, batch), dim3(256), 0, st, src, rows, cols, g.pairs_v, g.pairs, g.kbits, rel..., A);
    hipLaunchKernelGGL(k_conn_flatten, dim3(g.px_x, batch), dim3(256), 0, st, g.n, cols, g.kbits, A, B);
}

}  // namespace dcmt

extern "C" {

int dcmt_slic_connectivity_max_labels(int rows, int cols, int n_centers)
{
    const int bound = plan::connectivity_max_labels(rows, cols, n_centers);
    return bound == plan::kInvalid ? DCMT_E_INVALID : bound;
}

// The launches plan_connectivity names, on pp[0] and pp[1] (scratch every completion call rewrites before it reads it) and the
// context's strip slab, which the first call of this kind allocates for the context's maxima before it enqueues anything.  None of
// the context's carried state is read or written.
int dcmt_slic_connectivity_dev(dcmt_ctx* ctx, const int32_t* d_labels, int rows, int cols, int batch, int n_centers, int32_t* d_out,
                               int32_t* d_counts, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const plan::ConnPlan pl = plan::plan_connectivity(rows, cols, batch, n_centers, (uintptr_t)d_labels, (uintptr_t)d_out, (uintptr_t)d_counts);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    DCMT_TRY(ctx->conn_slab.reserve(ctx, plan::connectivity_slab_words(ctx->max_cols, ctx->max_batch)));
    hipStream_t st = (hipStream_t)stream;
    uint32_t* A = reinterpret_cast<uint32_t*>(ctx->pp[0].p);
    uint32_t* B = reinterpret_cast<uint32_t*>(ctx->pp[1].p);
    const uint32_t r = (uint32_t)rows, c = (uint32_t)cols;
    conn_label_enqueue(k_conn_local, k_conn_border, pl.g, d_labels, r, c, batch, A, B, st);
    hipLaunchKernelGGL(k_conn_seed, dim3(pl.strips, batch), dim3(256), 0, st, A, B, r, c, pl.g.kbits, pl.band_rows, pl.lim4, ctx->conn_slab.p);
    hipLaunchKernelGGL(k_conn_scan, dim3(batch), dim3(256), 0, st, ctx->conn_slab.p, pl.strips, d_counts);
    hipLaunchKernelGGL(k_conn_rank, dim3(pl.strips, batch), dim3(256), 0, st, B, r, c, pl.band_rows, ctx->conn_slab.p);
    hipLaunchKernelGGL(k_conn_relabel, dim3(pl.g.px_x, batch), dim3(256), 0, st, A, B, pl.g.n, c, pl.g.kbits, d_out);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

}  // extern "C"

// ---- the speckle filter of a disparity map (dcmt_kernels_speckle.h) ----------------------------------------------------------------
extern "C" {

void dcmt_default_speckle_params(dcmt_speckle_params* p)
{
    if (!p) return;
    p->max_size = 200;      // main_sl.cpp:1301, :1315: speckleWindowSize
    p->max_diff = 32;       // :1302, :1316: 16 * speckleRange, in the sixteenths disp16 is in
    p->new_val = -16;       // what dcmt_sgm_dev writes for "none"
}

// The launches plan_speckles names, on pp[0] and pp[1] (scratch every completion call rewrites before it reads it).  None of the
// context's carried state is read or written, and nothing is allocated.
int dcmt_filter_speckles_dev(dcmt_ctx* ctx, const int16_t* d_disp16, int16_t* d_out, float* d_depth, int rows, int cols, int batch,
                             const dcmt_speckle_params* params, uint32_t* d_removed, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !params || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const plan::SpecklePlan pl = plan::plan_speckles(rows, cols, batch, params->max_size, params->max_diff, params->new_val, (uintptr_t)d_disp16,
                                                     (uintptr_t)d_out, (uintptr_t)d_depth, (uintptr_t)d_removed);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    uint32_t* A = reinterpret_cast<uint32_t*>(ctx->pp[0].p);
    uint32_t* B = reinterpret_cast<uint32_t*>(ctx->pp[1].p);
    const uint32_t r = (uint32_t)rows, c = (uint32_t)cols, max_size = (uint32_t)params->max_size;
    const int32_t nv = params->new_val, md = params->max_diff;
    if (pl.clear_bytes) DCMT_HIP(ctx, hipMemsetAsync(d_removed, 0, pl.clear_bytes, st));
    conn_label_enqueue(k_spk_local, k_spk_border, pl.g, d_disp16, r, c, batch, A, B, st, nv, md);
    if (pl.vec == 4)
        hipLaunchKernelGGL(k_spk_apply<4>, dim3(pl.apply_x, batch), dim3(256), 0, st, d_disp16, A, B, pl.g.n, c, pl.g.kbits, nv, max_size, d_out, d_depth, d_removed);
    else
        hipLaunchKernelGGL(k_spk_apply<1>, dim3(pl.apply_x, batch), dim3(256), 0, st, d_disp16, A, B, pl.g.n, c, pl.g.kbits, nv, max_size, d_out, d_depth, d_removed);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

}  // extern "C"

// ---- Slic::display_contours, Slic::colour_with_cluster_means (dcmt_kernels_contour.h) ---------------------------------------------
extern "C" {

// The launches plan_contours names, on pp[0] (code bytes) and pp[1] (taken bytes): scratch every completion call rewrites before it
// reads it.  None of the context's carried state is read or written, and nothing is allocated.
int dcmt_slic_contours_dev(dcmt_ctx* ctx, const int32_t* d_labels, int rows, int cols, int batch, uint8_t* d_bgr, const uint8_t colour_bgr[3],
                           uint8_t* d_mask, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const plan::ContourPlan pl = plan::plan_contours(rows, cols, batch, (uintptr_t)d_labels, (uintptr_t)d_bgr, (uintptr_t)d_mask, (uintptr_t)colour_bgr);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* codes = reinterpret_cast<uint8_t*>(ctx->pp[0].p);
    uint8_t* taken = reinterpret_cast<uint8_t*>(ctx->pp[1].p);
    const uint32_t r = (uint32_t)rows, c = (uint32_t)cols;
    hipLaunchKernelGGL(k_cont_classify, dim3(pl.tile_grid, batch), dim3(256), 0, st, d_labels, r, c, pl.tiles_x, codes);
    hipLaunchKernelGGL(k_cont_walk, dim3(batch), dim3(64), pl.walk_lds, st, codes, taken, r, c, pl.chunks);
    hipLaunchKernelGGL(k_cont_paint, dim3(pl.tile_grid, batch), dim3(256), 0, st, taken, r, c, pl.tiles_x, d_mask, d_bgr, (uint32_t)colour_bgr[0],
                       (uint32_t)colour_bgr[1], (uint32_t)colour_bgr[2]);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

// The launches plan_cluster_means names; the sums are the caller's d_sums or, without one, the head of pp[0].
int dcmt_slic_cluster_means_dev(dcmt_ctx* ctx, const int32_t* d_labels, int rows, int cols, int batch, int n_labels, uint8_t* d_bgr,
                                int32_t* d_sums, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const size_t plane_bytes = sizeof(float) * ctx->frame_elems * (size_t)ctx->max_batch;
    const plan::MeansPlan pl = plan::plan_cluster_means(rows, cols, batch, n_labels, plane_bytes, (uintptr_t)d_labels, (uintptr_t)d_bgr, (uintptr_t)d_sums);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    uint32_t* sums = d_sums ? reinterpret_cast<uint32_t*>(d_sums) : reinterpret_cast<uint32_t*>(ctx->pp[0].p);
    const uint32_t r = (uint32_t)rows, c = (uint32_t)cols, nl = (uint32_t)n_labels;
    hipLaunchKernelGGL(k_means_clear, dim3(pl.clear_grid), dim3(256), 0, st, sums, pl.words);
    hipLaunchKernelGGL(k_means_sum, dim3(pl.sum_grid, batch), dim3(256), 0, st, d_labels, d_bgr, r, c, pl.tiles_x, nl, sums);
    hipLaunchKernelGGL(k_means_paint, dim3(pl.px_x, batch), dim3(256), 0, st, d_labels, pl.n, nl, sums, d_bgr);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

}  // extern "C"

// ---- per-superpixel plane fitting of sparse depth (dcmt_kernels_planes.h) ----------------------------------------------------------
static uint32_t planes_bits(const float* v)
{
    uint32_t b;
    std::memcpy(&b, v, sizeof b);                     // the bits as they lie in the struct: nothing the compiler may assume finite
    return b;
}

extern "C" {

void dcmt_default_planes_params(dcmt_planes_params* p)
{
    if (!p) return;
    p->valid_thresh = 0.1f;
    p->max_depth = 100.0f;
    p->min_points = 3;
    p->min_extent = 2;
    p->refit_tol = 0.0f;
    p->keep_returns = 1;
}

int dcmt_superpixel_planes_max_labels(int max_rows, int max_cols, int max_batch, int batch)
{
    if (max_rows < 1 || max_cols < 1 || max_batch < 1 || batch < 1 || batch > max_batch) return 0;
    return plan::planes_max_labels(sizeof(float) * (size_t)max_rows * (size_t)max_cols * (size_t)max_batch, batch);
}

// The launches plan_superpixel_planes names: the moment records on pp[0], the fits in the caller's d_fits or, without one, on pp[1]
// (scratch every completion call rewrites before it reads it).  None of the context's carried state is read or written, and
// nothing is allocated.
int dcmt_superpixel_planes_dev(dcmt_ctx* ctx, const float* d_depth, const int32_t* d_labels, int rows, int cols, int batch, int n_labels,
                               const dcmt_planes_params* params, float* d_out, dcmt_plane_fit* d_fits, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !params || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const uint32_t lo = planes_bits(&params->valid_thresh), hi = planes_bits(&params->max_depth), tb = planes_bits(&params->refit_tol);
    const bool ok = plan::planes_params_ok(lo, hi, params->min_points, params->min_extent, tb, params->keep_returns);
    const size_t plane_bytes = sizeof(float) * ctx->frame_elems * (size_t)ctx->max_batch;
    const plan::PlanesPlan pl = plan::plan_superpixel_planes(rows, cols, batch, n_labels, plane_bytes, ok, ok && (tb << 1) != 0u, (uintptr_t)d_depth,
                                                             (uintptr_t)d_labels, (uintptr_t)d_out, (uintptr_t)d_fits);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* mom = reinterpret_cast<unsigned long long*>(ctx->pp[0].p);
    dcmt_plane_fit* fits = d_fits ? d_fits : reinterpret_cast<dcmt_plane_fit*>(ctx->pp[1].p);
    const uint32_t* depth = reinterpret_cast<const uint32_t*>(d_depth);
    const uint32_t r = (uint32_t)rows, c = (uint32_t)cols, nl = (uint32_t)n_labels;
    const uint32_t mp = (uint32_t)params->min_points, me = (uint32_t)params->min_extent;
    const double tol = (double)params->refit_tol;
    hipLaunchKernelGGL(k_planes_clear, dim3(pl.clear_grid), dim3(256), 0, st, reinterpret_cast<uint32_t*>(mom), pl.words);
    hipLaunchKernelGGL(k_planes_sum<false>, dim3(pl.sum_grid, batch), dim3(256), 0, st, depth, d_labels, r, c, pl.tiles_x, nl, lo, hi, fits, tol, mom);
    hipLaunchKernelGGL(k_planes_solve<false>, dim3(pl.solve_grid), dim3(256), 0, st, mom, pl.records, mp, me, fits);
    if (pl.refit) {
        hipLaunchKernelGGL(k_planes_clear, dim3(pl.clear_grid), dim3(256), 0, st, reinterpret_cast<uint32_t*>(mom), pl.words);
        hipLaunchKernelGGL(k_planes_sum<true>, dim3(pl.sum_grid, batch), dim3(256), 0, st, depth, d_labels, r, c, pl.tiles_x, nl, lo, hi, fits, tol, mom);
        hipLaunchKernelGGL(k_planes_solve<true>, dim3(pl.solve_grid), dim3(256), 0, st, mom, pl.records, mp, me, fits);
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(d_out);
    if (pl.vec == 4)
        hipLaunchKernelGGL(k_planes_paint<4>, dim3(pl.paint_x, batch), dim3(256), 0, st, depth, d_labels, pl.n, c, nl, lo, hi, params->keep_returns, fits, out);
    else
        hipLaunchKernelGGL(k_planes_paint<1>, dim3(pl.paint_x, batch), dim3(256), 0, st, depth, d_labels, pl.n, c, nl, lo, hi, params->keep_returns, fits, out);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

}  // extern "C"

// ---- the occlusion filter of a sparse depth plane (dcmt_kernels_occlusion.h) ------------------------------------------------------
// The launches plan_sparse_occlusion names, for an f32 plane (T = its bits) or the uint16 payload: the mask of an in-place call on
// pp[0] (scratch every completion call rewrites before it reads it).  None of the context's carried state is read or written, and
// nothing is allocated.
template <typename T>
static int sparse_occlusion_enqueue(dcmt_ctx* ctx, const T* d_sparse, float scale, bool scale_ok, T* d_out, int rows, int cols, int batch,
                                    const dcmt_occlusion_params* params, uint32_t* d_removed, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !params || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const uint32_t lo = planes_bits(&params->valid_thresh), hi = planes_bits(&params->max_depth);
    const bool ok = scale_ok && plan::occlusion_params_ok(params->rx, params->ry, params->tol_code, lo, hi);
    const plan::OcclusionPlan pl = plan::plan_sparse_occlusion(rows, cols, batch, (int)sizeof(T), ok, params->rx, params->ry, (uintptr_t)d_sparse,
                                                               (uintptr_t)d_out, (uintptr_t)d_removed);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t r = (uint32_t)rows, c = (uint32_t)cols, tol = (uint32_t)params->tol_code;
    if (pl.clear_bytes) DCMT_HIP(ctx, hipMemsetAsync(d_removed, 0, pl.clear_bytes, st));
    if (pl.in_place) {
        uint32_t* mask = reinterpret_cast<uint32_t*>(ctx->pp[0].p);
        hipLaunchKernelGGL((k_occl<T, false>), dim3(pl.grid, batch), dim3(256), pl.lds_bytes, st, d_sparse, r, c, pl.tiles_x, params->rx, params->ry, tol, lo, hi,
                           scale, (T*)nullptr, mask, pl.words_x, (uint32_t*)nullptr);
        hipLaunchKernelGGL((k_occl_apply<T>), dim3(pl.apply_x, batch), dim3(256), 0, st, mask, r, c, pl.words_x, d_out, d_removed);
    } else {
        hipLaunchKernelGGL((k_occl<T, true>), dim3(pl.grid, batch), dim3(256), pl.lds_bytes, st, d_sparse, r, c, pl.tiles_x, params->rx, params->ry, tol, lo, hi,
                           scale, d_out, (uint32_t*)nullptr, pl.words_x, d_removed);
    }
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

extern "C" {

void dcmt_default_occlusion_params(dcmt_occlusion_params* p)
{
    if (!p) return;
    p->rx = 3;              // dcmt.h derives the three: an HDL-64's azimuth step is at most 2.3 columns at f = 721.5,
    p->ry = 6;              // its ring spacing 5.04 rows,
    p->tol_code = 655;      // and 0.01 / m is twice what a 1.65 m ground plane changes over ry rows
    p->valid_thresh = 0.1f; // the planes' defaults
    p->max_depth = 100.0f;
}

int dcmt_sparse_occlusion_dev(dcmt_ctx* ctx, const float* d_sparse, float* d_out, int rows, int cols, int batch, const dcmt_occlusion_params* params,
                              uint32_t* d_removed, void* stream)
{
    return sparse_occlusion_enqueue(ctx, reinterpret_cast<const uint32_t*>(d_sparse), 1.0f, true, reinterpret_cast<uint32_t*>(d_out), rows, cols, batch,
                                    params, d_removed, stream);
}

int dcmt_sparse_occlusion_u16_dev(dcmt_ctx* ctx, const uint16_t* d_sparse, float scale, uint16_t* d_out, int rows, int cols, int batch,
                                  const dcmt_occlusion_params* params, uint32_t* d_removed, void* stream)
{
    volatile float m = scale;                         // read through memory, as finite_bits does: the compiler may assume an argument finite
    const float s = m;
    return sparse_occlusion_enqueue(ctx, d_sparse, s, plan::occlusion_scale_ok(planes_bits(&s)), d_out, rows, cols, batch, params, d_removed, stream);
}

}  // extern "C"

// ---- the distance to the nearest return and the trust mask (dcmt_kernels_support.h) -----------------------------------------------
// The launches plan_support_distance names, for an f32 sparse plane (T = its bits) or the uint16 payload: the column distances on
// pp[0] (scratch every completion call rewrites before it reads it), then the row pass, which writes every output.  None of the
// context's carried state is read or written, and nothing is allocated.
template <typename T>
static int support_distance_enqueue(dcmt_ctx* ctx, const T* d_sparse, float scale, bool scale_ok, const float* d_dense, const float* d_fallback, float* d_out,
                                    uint16_t* d_dist2, int rows, int cols, int batch, const dcmt_support_params* params, uint32_t* d_beyond, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !params || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const uint32_t lo = planes_bits(&params->valid_thresh), hi = planes_bits(&params->max_depth);
    const bool ok = scale_ok && plan::support_params_ok(params->max_radius, lo, hi);
    const plan::SupportPlan pl = plan::plan_support_distance(rows, cols, batch, (int)sizeof(T), ok, params->max_radius, (uintptr_t)d_sparse, (uintptr_t)d_dense,
                                                             (uintptr_t)d_fallback, (uintptr_t)d_out, (uintptr_t)d_dist2, (uintptr_t)d_beyond);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t r = (uint32_t)rows, c = (uint32_t)cols, cap = (uint32_t)params->max_radius + 1u;
    uint16_t* g = reinterpret_cast<uint16_t*>(ctx->pp[0].p);
    if (pl.clear_bytes) DCMT_HIP(ctx, hipMemsetAsync(d_beyond, 0, pl.clear_bytes, st));
    if (pl.ballots)
        hipLaunchKernelGGL((k_support_cols<T, true>), dim3(pl.cols_grid, batch), dim3(kSupportColsWave), pl.cols_lds, st, d_sparse, r, c, cap, lo, hi, scale, g);
    else
        hipLaunchKernelGGL((k_support_cols<T, false>), dim3(pl.cols_grid, batch), dim3(kSupportColsWave), 0, st, d_sparse, r, c, cap, lo, hi, scale, g);
    hipLaunchKernelGGL(k_support_rows, dim3(pl.rows_grid, batch), dim3(256), pl.rows_lds, st, g, r, c, pl.tiles_x, (int)params->max_radius,
                       reinterpret_cast<const uint32_t*>(d_dense), reinterpret_cast<const uint32_t*>(d_fallback), reinterpret_cast<uint32_t*>(d_out), d_dist2,
                       d_beyond);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

extern "C" {

void dcmt_default_support_params(dcmt_support_params* p)
{
    if (!p) return;
    p->max_radius = 9;      // the reach of H3..H5 per axis (2 + 4 + 3): dcmt.h says what that bounds
    p->valid_thresh = 0.1f; // the planes' and the occlusion filter's defaults
    p->max_depth = 100.0f;
}

int dcmt_support_distance_dev(dcmt_ctx* ctx, const float* d_sparse, const float* d_dense, const float* d_fallback, float* d_out, uint16_t* d_dist2, int rows,
                              int cols, int batch, const dcmt_support_params* params, uint32_t* d_beyond, void* stream)
{
    return support_distance_enqueue(ctx, reinterpret_cast<const uint32_t*>(d_sparse), 1.0f, true, d_dense, d_fallback, d_out, d_dist2, rows, cols, batch, params,
                                    d_beyond, stream);
}

int dcmt_support_distance_u16_dev(dcmt_ctx* ctx, const uint16_t* d_sparse, float scale, const float* d_dense, const float* d_fallback, float* d_out,
                                  uint16_t* d_dist2, int rows, int cols, int batch, const dcmt_support_params* params, uint32_t* d_beyond, void* stream)
{
    volatile float m = scale;                         // read through memory, as finite_bits does: the compiler may assume an argument finite
    const float s = m;
    return support_distance_enqueue(ctx, d_sparse, s, plan::occlusion_scale_ok(planes_bits(&s)), d_dense, d_fallback, d_out, d_dist2, rows, cols, batch, params,
                                    d_beyond, stream);
}

}  // extern "C"

// ---- the joint bilateral filter (dcmt_kernels_joint.h) ---------------------------------------------------------------------------
// The clear of the counts and the one kernel plan_joint_bilateral names.  Nothing of the context is read or written but its device
// and its limits: no scratch, no state, no allocation.
extern "C" {

void dcmt_default_joint_params(dcmt_joint_params* p)
{
    if (!p) return;
    p->radius = 6;           // DESIGN.md section 37 says how radius and the sigmas of dcmt_make_joint_tables were picked
    p->flags = DCMT_JOINT_FILL;
    p->min_weight = 1;
    p->valid_thresh = 0.1f;  // the support map's defaults
    p->max_depth = 100.0f;
}

int dcmt_make_joint_tables(int radius, double sigma_space, double sigma_guide, dcmt_joint_tables* tables)
{
    if (!tables || radius < 1 || radius > kJointMaxRadius) return DCMT_E_INVALID;
    if (!finite_bits64(sigma_space) || !finite_bits64(sigma_guide) || !(sigma_space > 0.0) || !(sigma_guide > 0.0)) return DCMT_E_INVALID;
    for (int d2 = 0; d2 < kJointSpace; ++d2)
        tables->w_space[d2] = d2 <= radius * radius ? (uint16_t)std::nearbyint(255.0 * std::exp(-(double)d2 / (2.0 * sigma_space * sigma_space))) : (uint16_t)0;
    for (int s = 0; s < kJointGuide; ++s)
        tables->w_guide[s] = (uint16_t)std::nearbyint(255.0 * std::exp(-((double)s * (double)s) / (2.0 * sigma_guide * sigma_guide)));
    return DCMT_OK;
}

int dcmt_joint_bilateral_dev(dcmt_ctx* ctx, const float* d_depth, const uint8_t* d_guide, int guide_channels, const dcmt_joint_tables* d_tables, float* d_out,
                             int rows, int cols, int batch, const dcmt_joint_params* params, uint32_t* d_counts, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !params || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const uint32_t lo = planes_bits(&params->valid_thresh), hi = planes_bits(&params->max_depth);
    const plan::JointPlan pl = plan::plan_joint_bilateral(rows, cols, batch, guide_channels, params->radius, params->flags, params->min_weight, lo, hi,
                                                          (uintptr_t)d_depth, (uintptr_t)d_guide, (uintptr_t)d_tables, (uintptr_t)d_out, (uintptr_t)d_counts);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (pl.clear_bytes) DCMT_HIP(ctx, hipMemsetAsync(d_counts, 0, pl.clear_bytes, st));
    hipLaunchKernelGGL(k_joint, dim3(pl.grid, batch), dim3(256), pl.lds_bytes, st, reinterpret_cast<const uint32_t*>(d_depth), d_guide, guide_channels, d_tables,
                       reinterpret_cast<uint32_t*>(d_out), (uint32_t)rows, (uint32_t)cols, pl.tiles_x, (int)params->radius, params->flags, params->min_weight, lo,
                       hi, d_counts);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

}  // extern "C"

// ---- surface normals and the flying-pixel filter (dcmt_kernels_normals.h) ---------------------------------------------------------
static uint64_t normals_bits64(const double* v)
{
    uint64_t b;
    std::memcpy(&b, v, sizeof b);                     // the bits as they lie in the struct: nothing the compiler may assume finite
    return b;
}

// The launches plan_depth_normals names: the clear of the counts, k_normals and, in place, k_occl_apply on the mask the kernel left
// on pp[0] (scratch every completion call rewrites before it reads it).  None of the context's carried state is read or written,
// and nothing is allocated.  cloud / d_table as for depth_to_cloud
static int depth_normals(dcmt_ctx* ctx, const float* d_depth, int rows, int cols, int batch, const dcmt_cloud_params* cloud,
                         const dcmt_cloud_params* d_table, const dcmt_normals_params* params, dcmt_normal* d_normals, float* d_out, uint32_t* d_counts,
                         void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !params || (!cloud && !d_table) || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const uint32_t db = planes_bits(&params->min_plane_dist), lo = planes_bits(&params->valid_thresh), hi = planes_bits(&params->max_depth);
    const bool ok = plan::normals_params_ok(db, lo, hi) &&
                    (!cloud || normals_intrinsics_ok(normals_bits64(&cloud->fx), normals_bits64(&cloud->fy), normals_bits64(&cloud->cx), normals_bits64(&cloud->cy)));
    const plan::NormalsPlan pl = plan::plan_depth_normals(rows, cols, batch, ok, (uintptr_t)d_depth, d_table != nullptr, (uintptr_t)d_table, (uintptr_t)d_normals,
                                                          (uintptr_t)d_out, (uintptr_t)d_counts);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    volatile float dm = params->min_plane_dist;       // one f32 product, rounded once: never contracted, never widened
    volatile float dmin2 = dm * dm;
    const uint32_t* depth = reinterpret_cast<const uint32_t*>(d_depth);
    uint32_t* out = reinterpret_cast<uint32_t*>(d_out);
    uint32_t* mask = pl.in_place ? reinterpret_cast<uint32_t*>(ctx->pp[0].p) : nullptr;
    uint4* recs = reinterpret_cast<uint4*>(d_normals);
    const uint32_t r = (uint32_t)rows, c = (uint32_t)cols;
    if (pl.clear_bytes) DCMT_HIP(ctx, hipMemsetAsync(d_counts, 0, pl.clear_bytes, st));
    const auto launch = [&](auto src) {                // NormK or NormTable
        with_value<true, false>(d_normals != nullptr, [&](auto nrm) {
            with_value<kNormOutNone, kNormOutFused, kNormOutMask>(pl.out_mode, [&](auto om) {
                if constexpr (decltype(nrm)::value || decltype(om)::value != kNormOutNone)
                    hipLaunchKernelGGL((k_normals<decltype(nrm)::value, decltype(om)::value, decltype(src)>), dim3(pl.grid_x, batch), dim3(256), 0, st, depth, r, c,
                                       pl.strips, pl.bands, pl.band_rows, src, lo, hi, (float)dmin2, recs, out, mask, pl.words_x, d_counts);
            });
        });
    };
    if (d_table) launch(NormTable{d_table});
    else launch(NormK{(float)cloud->fx, (float)cloud->fy, (float)cloud->cx, (float)cloud->cy});
    if (pl.in_place) hipLaunchKernelGGL((k_occl_apply<uint32_t>), dim3(pl.apply_x, batch), dim3(256), 0, st, mask, r, c, pl.words_x, out, (uint32_t*)nullptr);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

extern "C" {

void dcmt_default_normals_params(dcmt_normals_params* p)
{
    if (!p) return;
    p->min_plane_dist = 0.4f;   // measured on the cascade's output, whose ground bends to 0.50 m at the frame's sides: DESIGN.md section 38
    p->valid_thresh = 0.1f;     // the planes' defaults
    p->max_depth = 100.0f;
}

int dcmt_depth_normals_dev(dcmt_ctx* ctx, const float* d_depth, int rows, int cols, int batch, const dcmt_cloud_params* cloud,
                           const dcmt_normals_params* params, dcmt_normal* d_normals, float* d_out, uint32_t* d_counts, void* stream)
{
    if (!cloud) return DCMT_E_INVALID;
    return depth_normals(ctx, d_depth, rows, cols, batch, cloud, nullptr, params, d_normals, d_out, d_counts, stream);
}

int dcmt_depth_normals_calib_dev(dcmt_ctx* ctx, const float* d_depth, int rows, int cols, int batch, const dcmt_cloud_params* d_cloud,
                                 const dcmt_normals_params* params, dcmt_normal* d_normals, float* d_out, uint32_t* d_counts, void* stream)
{
    if (!d_cloud) return DCMT_E_INVALID;
    return depth_normals(ctx, d_depth, rows, cols, batch, nullptr, d_cloud, params, d_normals, d_out, d_counts, stream);
}

}  // extern "C"

// ---- get_initial_error (dcmt_kernels_photo.h) ------------------------------------------------------------------------------------
// The clear of the statistics and the one kernel plan_photo_error names.  Nothing of the context is read or written but its device
// and its limits: no scratch, no state, no allocation.
template <typename G>
static void photo_launch(const plan::PhotoPlan& pl, const uint32_t* depth, const uint8_t* left, const uint8_t* right, uint8_t* err,
                         unsigned long long* stats, int rows, int cols, int window, G P, hipStream_t st)
{
    const dim3 grid(pl.grid_x, pl.grid_y);
    if (!pl.lds_route) {
        hipLaunchKernelGGL(k_photo_error_global<G>, grid, dim3(kPhotoThreads), 0, st, depth, left, right, err, stats, rows, cols, window, P);
        return;
    }
    with_value<1, 2, 3, 4>(window, [&](auto w) {
        hipLaunchKernelGGL((k_photo_error<decltype(w)::value, G>), grid, dim3(kPhotoThreads), pl.lds, st, depth, left, right, err, stats, rows, cols,
                           pl.band, pl.pitch, pl.vec ? 1 : 0, P);
    });
}

// params: baseline and focal of the uniform call, or (table) only the window, with the device's [batch] records
static int photo_error(dcmt_ctx* ctx, const float* d_depth, const uint8_t* d_left, const uint8_t* d_right, int rows, int cols, int batch,
                       const dcmt_photo_error_params* params, const dcmt_stereo_calib* d_table, bool table, uint8_t* d_err, uint64_t* d_stats,
                       void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !params || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    if (!table && (!finite_bits(params->baseline) || !finite_bits(params->focal) || !(params->baseline > 0.0f) || !(params->focal > 0.0f)))
        return DCMT_E_INVALID;
    const plan::PhotoPlan pl = plan::plan_photo_error(rows, cols, batch, params->window, (uintptr_t)d_depth, (uintptr_t)d_left, (uintptr_t)d_right, table,
                                                      (uintptr_t)d_table, (uintptr_t)d_err, (uintptr_t)d_stats);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (pl.clear_bytes) DCMT_HIP(ctx, hipMemsetAsync(d_stats, 0, pl.clear_bytes, st));
    const uint32_t* depth = reinterpret_cast<const uint32_t*>(d_depth);
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(d_stats);
    if (table) photo_launch(pl, depth, d_left, d_right, d_err, stats, rows, cols, params->window, PhotoTable{d_table}, st);
    else photo_launch(pl, depth, d_left, d_right, d_err, stats, rows, cols, params->window, PhotoK{params->baseline, params->focal}, st);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

extern "C" {

void dcmt_default_photo_error_params(dcmt_photo_error_params* p)
{
    if (!p) return;
    p->baseline = 0.54f;          // main_sl.cpp:632
    p->focal = 9.597910e+02f;     // :634
    p->window = 2;                // :638
}

int dcmt_photo_error_dev(dcmt_ctx* ctx, const float* d_depth, const uint8_t* d_left, const uint8_t* d_right, int rows, int cols, int batch,
                         const dcmt_photo_error_params* params, uint8_t* d_err, uint64_t* d_stats, void* stream)
{
    return photo_error(ctx, d_depth, d_left, d_right, rows, cols, batch, params, nullptr, false, d_err, d_stats, stream);
}

int dcmt_photo_error_calib_dev(dcmt_ctx* ctx, const float* d_depth, const uint8_t* d_left, const uint8_t* d_right, int rows, int cols, int batch,
                               const dcmt_photo_error_params* params, const dcmt_stereo_calib* d_calib, uint8_t* d_err, uint64_t* d_stats,
                               void* stream)
{
    return photo_error(ctx, d_depth, d_left, d_right, rows, cols, batch, params, d_calib, true, d_err, d_stats, stream);
}

}  // extern "C"
