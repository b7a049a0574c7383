// dcmt_rectify.hip -- the kernels of dcmt_kernels_rectify.h, a code object of their own, and the two entry points that launch them:
// dcmt_rectify_map_dev and dcmt_rectify_dev.  The context and the checks they share with the other translation units come from
// dcmt_ctx.h; the single-frame host form dcmt_rectify is in dcmt_host.hip.
#include "dcmt_plan_side.h"
#include "dcmt_ctx.h"
#include "dcmt_kernels_rectify.h"

using namespace dcmt;

extern "C" {

// k_rectify_map: one launch (plan_rectify_map), the records read and tested by the kernel
int dcmt_rectify_map_dev(dcmt_ctx* ctx, const dcmt_rectify_calib* d_table, int n_maps, int rows, int cols, int32_t* d_map, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const plan::RectifyMapPlan pl = plan::plan_rectify_map(rows, cols, n_maps, (uintptr_t)d_table, (uintptr_t)d_map);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipLaunchKernelGGL(k_rectify_map, dim3(pl.grid_x, pl.grid_y), dim3(kRectifyThreads), 0, (hipStream_t)stream, d_table, (uint32_t)rows, (uint32_t)cols,
                       d_map);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

// k_rectify: one launch (plan_rectify).  What stays behind is the probe dcmt_last_path reads: the call's id here, and on the device
// the id in the word of every route a tile took.
int dcmt_rectify_dev(dcmt_ctx* ctx, const uint8_t* d_src, int src_rows, int src_cols, int channels, const int32_t* d_map, int n_maps,
                     const int32_t* d_map_index, uint32_t flags, uint8_t* d_dst, int rows, int cols, int batch, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    const plan::RectifyPlan pl = plan::plan_rectify(src_rows, src_cols, channels, rows, cols, batch, n_maps, flags, (uintptr_t)d_src, (uintptr_t)d_map,
                                                    (uintptr_t)d_map_index, (uintptr_t)d_dst);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    if (++ctx->rectify_call == 0) ctx->rectify_call = 1;
    std::strcpy(ctx->last_path, "k_rectify");
    const dim3 grid(pl.grid_x, pl.grid_y, pl.grid_z);
    const uint32_t force = (flags & DCMT_RECTIFY_FORCE_GATHER) ? 1u : 0u;
    with_value<1, 3>(channels, [&](auto ch) {
        hipLaunchKernelGGL(k_rectify<decltype(ch)::value>, grid, dim3(kRectifyThreads), 0, (hipStream_t)stream, d_src, (uint32_t)src_rows, (uint32_t)src_cols,
                           d_map, (uint32_t)n_maps, d_map_index, d_dst, (uint32_t)rows, (uint32_t)cols, (uint32_t)batch, pl.tiles_x, pl.per_chunk, force,
                           ctx->rectify_route.p, ctx->rectify_call);
    });
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

}  // extern "C"
