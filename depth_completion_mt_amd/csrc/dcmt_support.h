// dcmt_support.h -- what the kernels of dcmt_kernels_support.h (compiled in dcmt_cloud.hip) share with the host code that plans
// their launches (dcmt_plan_side.h): the tiles, the marker and the bounds of dcmt_support_params (include/dcmt.h,
// dcmt_support_distance_dev).  No HIP.  The return test is the planes' (dcmt_planes.h, dcmt_kernels_planes.h), not restated here.
#pragma once
#include <cstdint>

namespace dcmt {

constexpr int kSupportMaxRadius = 255;          // max_radius at most: 255^2 = 65025 < 65535, so the marker is never a distance
constexpr uint32_t kSupportBeyond = 65535u;     // d_dist2 where D2 > max_radius^2
constexpr int kSupportColsWave = 64;            // k_support_cols: one wave (one workgroup) per strip of 64 columns, lane = column
constexpr int kSupportChunk = 8;                // ... its loads are issued 8 rows at a time
constexpr int kSupportLdsRows = 4096;           // ... and keeps the ballots of at most this many rows in LDS (8 bytes a row: 32 KiB);
                                                // a taller frame takes the route that reads the sparse plane twice
constexpr int kSupportTile = 256;               // k_support_rows: one workgroup per segment of 256 columns, lane = pixel,
constexpr int kSupportBand = 4;                 // ... of 4 consecutive rows at a time,
constexpr int kSupportGroup = 4;                // ... 4 such bands one after another (the next one's loads behind this one's work)
constexpr int kSupportSlots = (kSupportTile + 2 * kSupportMaxRadius + kSupportTile - 1) / kSupportTile;        // ... a lane stages at most 3
                                                // columns of a row: the segment with its halo is at most 766 wide

// dynamic LDS of k_support_cols: one 64-bit ballot a row, none on the route that reads the plane twice
constexpr uint32_t support_cols_lds_bytes(int rows) { return rows <= kSupportLdsRows ? 8u * (uint32_t)rows : 0u; }

// dynamic LDS of k_support_rows: the squared column distances of the band's segments with a halo of max_radius columns either side
constexpr uint32_t support_rows_lds_bytes(int max_radius)
{
    return 4u * (uint32_t)kSupportBand * (uint32_t)(kSupportTile + 2 * max_radius);
}

}  // namespace dcmt
