// dcmt_normals.h -- what the kernel of dcmt_kernels_normals.h (compiled in dcmt_cloud.hip) shares with the host code that plans its
// launch (dcmt_plan_side.h) and fills its arguments: the strip and band of a wave, the intrinsics as the kernel takes them, and the
// bounds of dcmt_depth_normals_dev (include/dcmt.h) on the bits of a dcmt_cloud_params record.  No HIP.  The return test and its
// bounds are the planes' (dcmt_planes.h, dcmt_kernels_planes.h), not restated here.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DCMT_NORMALS_HD __host__ __device__
#else
#define DCMT_NORMALS_HD
#endif

namespace dcmt {

constexpr int kNormCols = 64;                   // k_normals: a wave's strip is 64 columns, lane = column, every lane an output
constexpr int kNormRows = 32;                   // ... and its band this many output rows at most
constexpr uint64_t kNormMinFocalBits = 0x3f50000000000000ull;    // |fx|, |fy| >= 2^-10, as f64
constexpr uint64_t kNormMaxIntrBits = 0x4130000000000000ull;     // |fx|, |fy|, |cx|, |cy| <= 2^20, as f64
constexpr uint32_t kNormMaxDistBits = 0x44800000u;               // min_plane_dist <= 1024.0f

// fx, fy, cx, cy rounded once to f32: what the kernel computes with, by value (the uniform call) or from the frame's record
struct NormK { float fx, fy, cx, cy; };

// dcmt.h's bounds on the intrinsics, on the bits of the four doubles: NaN and Inf lie above every bound, -0.0 is zero
DCMT_NORMALS_HD inline bool normals_intrinsics_ok(uint64_t fx, uint64_t fy, uint64_t cx, uint64_t cy)
{
    const uint64_t m = 0x7fffffffffffffffull;
    return (fx & m) >= kNormMinFocalBits && (fx & m) <= kNormMaxIntrBits && (fy & m) >= kNormMinFocalBits && (fy & m) <= kNormMaxIntrBits &&
           (cx & m) <= kNormMaxIntrBits && (cy & m) <= kNormMaxIntrBits;
}

}  // namespace dcmt
