// dcmt_calib.h -- per-frame calibration tables as the kernels' table instances read them (dcmt_project_points_calib_dev,
// dcmt_depth_to_cloud_calib_dev, dcmt_reproject_depth_calib_dev, dcmt_stereo_refine_calib_dev): device arrays of [batch] records in
// the layouts of include/dcmt.h, only ever read.
//
// A record is loaded as INTEGER words and tested in the integer domain before any of it becomes a float: the library is built
// with -ffinite-math-only, so a float compare against NaN or Inf is one the compiler may remove, while a load of an integer tells
// it nothing.  A record that fails the test (the host checks of the uniform entry points, per frame) makes its frame EMPTY: the
// scatter kernels leave no tag of the call's generation in the frame's part of the winner plane, the cloud's count pass counts
// nothing, the stereo kernel writes zeros.  Nothing is ever addressed with a value derived from such a record.
//
// Where the record's index is wave-uniform (blockIdx, or a readfirstlane behind a ballot) the loads go through the scalar cache:
// s_load_dwordx*, issued once per wave in front of the pixel loop, the values in SGPRs exactly where the uniform kernels hold
// their by-value argument.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dcmt.h"
#include "dcmt_cloud.h"

namespace dcmt {

static_assert(sizeof(dcmt_project_calib) == 96 && offsetof(dcmt_project_calib, P) == 48, "dcmt_project_calib layout");
static_assert(sizeof(dcmt_stereo_calib) == 8 && offsetof(dcmt_stereo_calib, focal) == 4, "dcmt_stereo_calib layout");
static_assert(sizeof(dcmt_cloud_params) == 32, "dcmt_cloud_params layout");
static_assert(sizeof(dcmt_reproject_params) == 136 && offsetof(dcmt_reproject_params, M) == 32 && offsetof(dcmt_reproject_params, K) == 96,
              "dcmt_reproject_params layout");

constexpr uint32_t kReprojRecWords = sizeof(dcmt_reproject_params) / 4;      // 34 dwords: fx fy cx cy (8), M (16), K (9), one pad
constexpr uint32_t kProjRecWords = sizeof(dcmt_project_calib) / 4;           // 24 dwords: T rows 0..2, P

__device__ __forceinline__ bool bits_finite32(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool bits_finite64(uint64_t b) { return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
__device__ __forceinline__ bool bits_nonzero64(uint64_t b) { return (b << 1) != 0; }      // neither +0.0 nor -0.0

// fx, fy, cx, cy: the 32 bytes of a dcmt_cloud_params and the head of a dcmt_reproject_params.  intrinsics_ok (dcmt_ctx.h) on bits
__device__ __forceinline__ bool load_intrinsics(const uint64_t* __restrict__ q, double& fx, double& fy, double& cx, double& cy)
{
    const uint64_t a = q[0], b = q[1], c = q[2], d = q[3];
    fx = __longlong_as_double((long long)a); fy = __longlong_as_double((long long)b);
    cx = __longlong_as_double((long long)c); cy = __longlong_as_double((long long)d);
    return bits_finite64(a) && bits_finite64(b) && bits_finite64(c) && bits_finite64(d) && bits_nonzero64(a) && bits_nonzero64(b);
}

__device__ __forceinline__ bool load_cloud_record(const dcmt_cloud_params* __restrict__ table, uint32_t f, CloudK& k)
{
    return load_intrinsics(reinterpret_cast<const uint64_t*>(table) + 4 * (size_t)f, k.fx, k.fy, k.cx, k.cy);
}

// the whole record the scatter needs, checked as dcmt_reproject_depth_dev checks it: the intrinsics, rows 0..2 of M, rows 0..1 of K.
// On the scalar unit, some ninety instructions per wave in front of a thousand of pixel arithmetic.  (The same test spread over 22
// lanes and a ballot is a handful of instructions, but its vector load stands in front of the depth loads: the call was 3.7 %
// slower with it than with this, measured.)
__device__ __forceinline__ bool load_reproject_record(const dcmt_reproject_params* __restrict__ table, uint32_t f, ReprojK& k)
{
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(table) + kReprojRecWords * (size_t)f;
    bool ok = load_intrinsics(reinterpret_cast<const uint64_t*>(w), k.fx, k.fy, k.cx, k.cy);
#pragma unroll
    for (int i = 0; i < 12; ++i) { const uint32_t b = w[8 + i]; ok = ok && bits_finite32(b); k.M[i] = __uint_as_float(b); }
#pragma unroll
    for (int i = 0; i < 6; ++i) { const uint32_t b = w[24 + i]; ok = ok && bits_finite32(b); k.K[i] = __uint_as_float(b); }
    return ok;
}

// what reproject_t2 reads, for the resolve: a pixel that holds a tag of the call's generation lies in a frame whose record the
// scatter has accepted, so nothing is tested again
__device__ __forceinline__ void load_reproject_t2_record(const dcmt_reproject_params* __restrict__ table, uint32_t f, ReprojK& k)
{
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(table) + kReprojRecWords * (size_t)f;
    const uint64_t* __restrict__ q = reinterpret_cast<const uint64_t*>(w);
    k.fx = __longlong_as_double((long long)q[0]); k.fy = __longlong_as_double((long long)q[1]);
    k.cx = __longlong_as_double((long long)q[2]); k.cy = __longlong_as_double((long long)q[3]);
#pragma unroll
    for (int i = 8; i < 12; ++i) k.M[i] = __uint_as_float(w[8 + i]);
}

}  // namespace dcmt
