// dcmt_sgm.hip -- semi-global stereo matching (dcmt_kernels_sgm.h), a code object of its own: dcmt_default_sgm_params,
// dcmt_sgm_workspace_bytes, dcmt_sgm_dev, dcmt_sgm_paths_dev, dcmt_sgm_guided_dev and dcmt_sgm_cost_dev (of which dcmt_sgm_guided_dev is the
// absolute-difference case, dcmt_sgm_paths_dev the case of that without a guide, and dcmt_sgm_dev the four-path case of that).  The plan (dcmt_sgm.h: plan_sgm) checks the arguments, lays the caller's
// workspace out and cuts the batch into chunks; this file launches what it says: per chunk the instance of k_sgm_rows<NPL, LDS, GUIDED, COST>
// that the plan's (per_lane, lds_route, guided, cost) name, k_sgm_cols, with eight paths k_sgm_diag twice, and k_sgm_winner.
// The single-pair host forms, dcmt_sgm, dcmt_sgm_paths, dcmt_sgm_guided and dcmt_sgm_cost, are in dcmt_host.hip.
#include <initializer_list>

#include "dcmt.h"
#include "dcmt_ctx.h"
#include "dcmt_sgm.h"
#include "dcmt_kernels_sgm.h"

using namespace dcmt;

// the instance of k_sgm_rows the plan asks for
using SgmRowsKernel = void (*)(const uint8_t*, const uint8_t*, uint16_t*, int, int, int, int, int, SgmGuide);
template <int NPL>
static SgmRowsKernel sgm_rows_kernel(const plan::SgmPlan& pl)
{
    constexpr int A = kSgmCostAbsdiff, C = kSgmCostCensus;
    static constexpr SgmRowsKernel table[2][2][2] = {                                   // [cost][lds_route][guided]
        {{k_sgm_rows<NPL, false, false, A>, k_sgm_rows<NPL, false, true, A>}, {k_sgm_rows<NPL, true, false, A>, k_sgm_rows<NPL, true, true, A>}},
        {{k_sgm_rows<NPL, false, false, C>, k_sgm_rows<NPL, false, true, C>}, {k_sgm_rows<NPL, true, false, C>, k_sgm_rows<NPL, true, true, C>}},
    };
    return table[pl.cost == kSgmCostCensus][pl.lds_route][pl.guided];
}

template <int NPL>
static void sgm_chunk(const plan::SgmPlan& pl, const uint8_t* left, const uint8_t* right, const float* guide, int16_t* disp16, float* depth,
                      uint16_t* vol, int rows, int cols, int frames, const dcmt_sgm_params& P, hipStream_t st)
{
    const int D = P.num_disparities;
    const float bf = P.baseline * P.focal;                  // rounded once: the hint's and step 9's
    const dim3 rows_grid(pl.rows_grid_x, (unsigned)frames), cols_grid(pl.cols_grid_x, (unsigned)frames), winner_grid(pl.winner_grid_x, (unsigned)frames);
    const SgmGuide g = {reinterpret_cast<const uint32_t*>(guide), bf, pl.guide_weight, pl.guide_cap};     // all zero but bf without a guide
    hipLaunchKernelGGL(sgm_rows_kernel<NPL>(pl), rows_grid, dim3(kSgmRowThreads), pl.lds, st, left, right, vol, rows, cols, D, P.p1, P.p2, g);
    hipLaunchKernelGGL((k_sgm_cols<NPL>), cols_grid, dim3(64 * kSgmWaves), 0, st, vol, rows, cols, D, P.p1, P.p2);
    if (pl.paths == 8) {                                    // one launch per orientation: a "\" line and a "/" line cross
        const dim3 diag_grid(pl.diag_grid_x, (unsigned)frames);
        hipLaunchKernelGGL((k_sgm_diag<NPL, +1>), diag_grid, dim3(64 * kSgmWaves), 0, st, vol, rows, cols, D, P.p1, P.p2);
        hipLaunchKernelGGL((k_sgm_diag<NPL, -1>), diag_grid, dim3(64 * kSgmWaves), 0, st, vol, rows, cols, D, P.p1, P.p2);
    }
    const SgmK K = {D, P.uniqueness, P.disp12_max_diff, bf, P.max_depth};
    hipLaunchKernelGGL((k_sgm_winner<NPL>), winner_grid, dim3(64 * kSgmWaves), 0, st, (const uint16_t*)vol, disp16, depth, rows, cols, pl.segments, K);
}

extern "C" {

void dcmt_default_sgm_params(dcmt_sgm_params* p)
{
    if (!p) return;
    p->num_disparities = 64;      // main_sl.cpp:1306: numDisparity * 16
    p->p1 = 200;
    p->p2 = 800;
    p->uniqueness = 10;
    p->disp12_max_diff = 1;
    p->baseline = 0.54f;          // :632
    p->focal = 9.597910e+02f;     // :634
    p->max_depth = 100.0f;
}

size_t dcmt_sgm_workspace_bytes(int rows, int cols, int num_disparities, int frames)
{
    if (rows < 1 || cols < 1 || frames < 1 || !plan::sgm_disparities_ok(num_disparities)) return 0;
    return (size_t)frames * plan::sgm_frame_bytes(rows, cols, num_disparities);
}

int dcmt_sgm_cost_dev(dcmt_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, const float* d_guide, int16_t* d_disp16, float* d_depth, int rows,
                      int cols, int batch, const dcmt_sgm_params* params, int paths, int guide_weight, int guide_cap, int cost, void* d_work,
                      size_t work_bytes, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !params || !dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    if (d_depth)
        for (const float v : {params->baseline, params->focal, params->max_depth})
            if (!finite_bits(v) || !(v > 0.0f)) return DCMT_E_INVALID;
    if (d_guide)                                            // the hint needs them, with or without a depth plane
        for (const float v : {params->baseline, params->focal})
            if (!finite_bits(v) || !(v > 0.0f)) return DCMT_E_INVALID;
    const plan::SgmPlan pl = plan::plan_sgm(rows, cols, batch, params->num_disparities, params->p1, params->p2, params->uniqueness, (uintptr_t)d_left,
                                            (uintptr_t)d_right, (uintptr_t)d_disp16, (uintptr_t)d_depth, (uintptr_t)d_work, work_bytes, paths,
                                            (uintptr_t)d_guide, guide_weight, guide_cap, cost);
    if (pl.status != plan::kOk) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t px = (size_t)rows * (size_t)cols;
    for (int i = 0; i < pl.n_chunks; ++i) {
        const size_t first = (size_t)i * (size_t)pl.chunk * px;
        const int frames = plan::sgm_chunk_frames(pl, batch, i);
        int16_t* disp = d_disp16 ? d_disp16 + first : nullptr;
        float* depth = d_depth ? d_depth + first : nullptr;
        const float* guide = d_guide ? d_guide + first : nullptr;
        if (pl.per_lane == 1) sgm_chunk<1>(pl, d_left + first, d_right + first, guide, disp, depth, (uint16_t*)d_work, rows, cols, frames, *params, st);
        else sgm_chunk<2>(pl, d_left + first, d_right + first, guide, disp, depth, (uint16_t*)d_work, rows, cols, frames, *params, st);
    }
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

int dcmt_sgm_guided_dev(dcmt_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, const float* d_guide, int16_t* d_disp16, float* d_depth, int rows,
                        int cols, int batch, const dcmt_sgm_params* params, int paths, int guide_weight, int guide_cap, void* d_work, size_t work_bytes,
                        void* stream)
{
    return dcmt_sgm_cost_dev(ctx, d_left, d_right, d_guide, d_disp16, d_depth, rows, cols, batch, params, paths, guide_weight, guide_cap,
                             DCMT_SGM_COST_ABSDIFF, d_work, work_bytes, stream);
}

int dcmt_sgm_paths_dev(dcmt_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int16_t* d_disp16, float* d_depth, int rows, int cols, int batch,
                       const dcmt_sgm_params* params, int paths, void* d_work, size_t work_bytes, void* stream)
{
    return dcmt_sgm_guided_dev(ctx, d_left, d_right, nullptr, d_disp16, d_depth, rows, cols, batch, params, paths, 0, 0, d_work, work_bytes, stream);
}

int dcmt_sgm_dev(dcmt_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int16_t* d_disp16, float* d_depth, int rows, int cols, int batch,
                 const dcmt_sgm_params* params, void* d_work, size_t work_bytes, void* stream)
{
    return dcmt_sgm_paths_dev(ctx, d_left, d_right, d_disp16, d_depth, rows, cols, batch, params, 4, d_work, work_bytes, stream);
}

}  // extern "C"
