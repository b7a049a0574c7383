// dcmt_contour.h -- what the kernels of dcmt_kernels_contour.h (compiled in dcmt_cloud.hip) share with the host code that plans
// their launches (dcmt_plan_side.h).  No HIP.
#pragma once
#include <cstdint>

namespace dcmt {

constexpr int kContTile = 64;                   // k_cont_classify, k_cont_paint, k_means_sum: one workgroup per tile of 64 x 64 pixels;
                                                // k_cont_walk: one step is 64 rows of a column, one lane per row
constexpr int kContMaxChunks = 4096;            // k_cont_walk keeps one 64-bit mask per 64 rows of a column in LDS (32 KiB at most)
constexpr int kContAhead = 16;                  // steps of k_cont_walk whose code bytes are loaded together, one block ahead

// a pixel's code byte (k_cont_classify -> k_cont_walk)
constexpr uint32_t kCodeLater = 7u;             // bits 0..2: A, its in-frame later neighbours with another label
constexpr uint32_t kCodeWestUp = 8u;            // (x-1, y-1) is in the frame and has another label
constexpr uint32_t kCodeWest = 16u;             // (x-1, y)
constexpr uint32_t kCodeWestDown = 32u;         // (x-1, y+1)
constexpr uint32_t kCodeNorth = 64u;            // (x, y-1)

constexpr int kMeansSlots = 512;                // k_means_sum: labels [tile minimum, + kMeansSlots) are summed in LDS, the others in global memory
constexpr int kMeansRun = 16;                   // ... a thread walks 16 rows of one column of the tile

}  // namespace dcmt
