// dcmt_connect.h -- what the kernels of dcmt_kernels_connect.h and dcmt_kernels_speckle.h (compiled in dcmt_cloud.hip) share with the host code that plans
// their launches (dcmt_plan_side.h).  No HIP.
#pragma once
#include <cstdint>

namespace dcmt {

constexpr int kConnTW = 64, kConnTH = 16;       // k_conn_local: one workgroup per tile of kConnTW columns x kConnTH rows
constexpr int kConnPad = kConnTH + 1;           // its LDS arrays hold pixel (lx, ly) of the tile at lx * kConnPad + ly
constexpr int kConnStripCols = 64;              // k_conn_seed / k_conn_rank: one workgroup per strip of columns, one lane per column
constexpr int kConnWaves = 4;                   // ... its waves each walk a band of ceil(rows / kConnWaves) rows
constexpr uint32_t kConnNone = 0x7fffffffu;     // a small component's link: no labelled neighbour (the component of pixel (0, 0))
constexpr uint32_t kConnRank = 0x80000000u;     // a non-small seed's word: this bit | its label

// A pixel's key: (x << kbits) | y with 2^kbits >= rows -- ordered as the reference's scan order s = x * rows + y (column outer, row
// inner), and taken apart with a shift and a mask instead of a division.  Below 2^30 for every frame dcmt_create admits.
inline int conn_key_bits(int rows)
{
    int k = 0;
    while ((1 << k) < rows) ++k;
    return k;
}

}  // namespace dcmt
