// dcmt_occlusion.h -- what the kernels of dcmt_kernels_occlusion.h (compiled in dcmt_cloud.hip) share with the host code that plans
// their launches (dcmt_plan_side.h): the tile and the bounds of dcmt_occlusion_params (include/dcmt.h, dcmt_sparse_occlusion_dev).
// No HIP.  The return test and the code of a depth are the planes' (dcmt_planes.h, dcmt_kernels_planes.h), not restated here.
#pragma once
#include <cstdint>

namespace dcmt {

constexpr int kOcclTile = 64;                   // k_occl: one workgroup per tile of 64 x 64 pixels, lane = column of the tile
constexpr int kOcclRun = 16;                    // ... a wave takes 16 rows of it
constexpr int kOcclMaxRx = 8;                   // rx at most: the tile with its halo is 80 columns wide
constexpr int kOcclMaxRy = 16;                  // ry at most: ... and 96 rows high (30 KiB of codes)
constexpr int32_t kOcclMaxTol = 1 << 20;        // tol_code at most: the largest code, beyond which nothing is ever removed

// dynamic LDS of k_occl: the codes of the tile with its halo (the horizontal maxima of a row then replace its codes)
constexpr uint32_t occl_lds_bytes(int rx, int ry)
{
    return 4u * (uint32_t)(kOcclTile + 2 * ry) * (uint32_t)(kOcclTile + 2 * rx);
}

}  // namespace dcmt
