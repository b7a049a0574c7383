// dcmt_joint.h -- what the kernel of dcmt_kernels_joint.h (compiled in dcmt_cloud.hip) shares with the host code that plans its
// launch (dcmt_plan_side.h): the tile, the bounds of dcmt_joint_params and the layout of its LDS (include/dcmt.h,
// dcmt_joint_bilateral_dev).  No HIP.  The validity test is the planes' (dcmt_planes.h, dcmt_kernels_planes.h), not restated here.
#pragma once
#include <cstdint>

namespace dcmt {

constexpr int kJointMaxRadius = 9;              // radius at most: 253 taps * 255 * 255 < 2^24, so (float) sw is exact
constexpr int kJointTileX = 64;                 // k_joint: one workgroup of four waves per tile of 64 x 16 outputs, lane = column,
constexpr int kJointTileY = 16;                 // ... wave w owns the tile's rows w, w + 4, w + 8, w + 12
constexpr int kJointPix = 4;                    // ... four pixels a lane
constexpr int kJointSpace = 128;                // entries of w_space
constexpr int kJointGuide = 768;                // entries of w_guide; the LDS copy is extended to kJointGuideLds with zeros, and a
constexpr int kJointGuideLds = 1024;            // tap on a hole reads entry kJointGuide: w = 0 without a branch
constexpr uint32_t kJointFlags = 3u;            // DCMT_JOINT_FILL | DCMT_JOINT_SMOOTH
constexpr int kJointPitch = kJointTileX + 2 * kJointMaxRadius;       // pixels between two rows of the staged tile, whatever R
constexpr uint32_t kJointBias = 1u << 24;       // above any sw: 253 * 255 * 255 = 16 451 325

constexpr uint32_t kJointTableLds = (uint32_t)(kJointGuideLds + kJointSpace);          // static LDS of k_joint: the two tables clamped to
                                                // 255, a byte an entry

// dynamic LDS of k_joint: the tile with a halo of R as one pair of dwords per pixel (the depth's bits, 0 on a hole or outside the
// frame; the guide's bytes), its rows kJointPitch pixels apart
constexpr uint32_t joint_lds_bytes(int radius) { return 8u * (uint32_t)kJointPitch * (uint32_t)(kJointTileY + 2 * radius); }

}  // namespace dcmt
