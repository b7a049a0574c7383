// dcmt_rectify.h -- the constants of k_rectify_map and k_rectify (dcmt_kernels_rectify.h, compiled in dcmt_rectify.hip) and what the
// kernel does with a tile's bounding box, as plain functions.  No HIP: plan_rectify (dcmt_plan_side.h) and tests/plan_rectify_test.cpp
// use the same statements as the kernel.
#pragma once
#include <cstdint>

#include "dcmt_chunks.h"       // DCMT_HD

namespace dcmt {

constexpr int kRectifyThreads = 256;             // both kernels
// k_rectify: a workgroup owns one destination tile of one map, a lane kRectifyPxPerLane consecutive pixels of one of its rows
constexpr uint32_t kRectifyTileW = 64, kRectifyTileH = 16, kRectifyPxPerLane = 4;
static_assert(kRectifyTileW * kRectifyTileH == kRectifyPxPerLane * kRectifyThreads, "k_rectify tile");
// the LDS a workgroup stages a frame's bounding box in.  16 KB: eight workgroups (the 32 waves a CU holds) use 128 of its 160 KB,
// so the budget never costs occupancy; at KITTI's calibration a tile's box is at most 51 x 23 pixels, 4.4 KB as BGR
constexpr uint32_t kRectifyLdsBytes = 16384;
constexpr int kRectifyMaxSrcSide = 16384;
constexpr uint32_t kRectifyTargetWgs = 2048;     // plan_rectify splits a map's frames over grid.z until the call has this many workgroups
constexpr uint32_t kRectifyRouteLds = 0, kRectifyRouteGather = 1;      // words of the route probe (dcmt_ctx::rectify_route)

// The pitch of the staged box's rows in LDS: a row is loaded as the naturally aligned 16-byte quads that hold its w * ch bytes,
// which start at byte 0..15 of the first, so (w * ch + 15) bytes rounded up to quads -- and an ODD number of quads, so that taps a
// row apart fall into different 16-byte slots of the bank row.
DCMT_HD inline uint32_t rectify_pitch(uint32_t w, uint32_t ch) { return 16u * ((((w * ch + 15u) + 15u) / 16u) | 1u); }

// whether a box of w x h source pixels goes through LDS
DCMT_HD inline bool rectify_box_fits(uint32_t w, uint32_t h, uint32_t ch)
{
    return (uint64_t)h * rectify_pitch(w, ch) <= kRectifyLdsBytes;
}

}  // namespace dcmt
