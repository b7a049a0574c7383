// dcmt_kernels_nearest.h -- the two geometric scatter calls under the rule every producer of sparse depth uses: a pixel hit by
// several points (dcmt_project_points_nearest*_dev) or source pixels (dcmt_reproject_depth_nearest*_dev) keeps the NEAREST, the
// smallest of the values the last-wins kernels (k_project_scatter, dcmt_kernels_v1.h; k_reproject_scatter,
// dcmt_kernels_reproject.h) would have stored there.  A point or pixel is transformed, accepted and rejected by the very statements
// of those kernels -- project_point / project_scatter_calib_run (dcmt_project.h), reproject_scatter_run -- so the set of occupied
// pixels is the same; only the store differs.
//
// The depth is the payload, so there is no index and no winner plane: an order-preserving integer key (dcmt_depth_key.h) goes into
// the OUTPUT plane itself.
//   hipMemsetAsync           zeroes the output: key 0 = nothing landed (no finite value has key 0);
//   k_*_nearest_scatter      per source: one integer atomicMax (no value returned) of key(v) at the landing pixel.  The largest key
//                            is the smallest value in the total order of finite f32 (-0 below +0); an integer max does not depend
//                            on arrival order, so the result is the same bits on every run.  No float atomics.  The address is
//                            formed only after the bound has held in the integer domain;
//   k_nearest_fixup          in place over the whole batch: key -> the value's bits, 0 -> 0.0f, 16 / 8 / 4 bytes per thread as
//                            plan::resolve_vec allows.
// Bytes per source (s) and destination pixel (d): projection 16 s (the record) + 4 per landing point (atomics) + 12 d (clear, key
// read, value write); reprojection 4 s + 4 per landing pixel + 12 d.  Against last-wins: 4 d more for the clear; the winner's gather
// (16 B resp. 4 B per occupied pixel) and the recomputation of its depth are gone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcmt_depth_key.h"
#include "dcmt_kernels_reproject.h"
#include "dcmt_project.h"

namespace dcmt {

// what every scatter kernel here does at a landing pixel of the key plane
__device__ __forceinline__ void nearest_store(unsigned* __restrict__ keys, size_t px, float v)
{
    atomicMax(&keys[px], depth_key(__float_as_uint(v)));
}

// k_project_scatter's shape: one point per thread, the workgroup's frame search over d_offsets.  keys: the output plane,
// [batch][rows][cols], zeroed
__global__ __launch_bounds__(256)
void k_project_nearest_scatter(const float* __restrict__ pts, const int* __restrict__ offsets, int n_points, int batch,
                               ProjMats M, unsigned* __restrict__ keys, int rows, int cols)
{
    const int i0 = blockIdx.x * 256;
    const int lo_wg = project_wg_frame(offsets, batch, i0);
    const int i = i0 + threadIdx.x;
    if (i >= n_points) return;
    int lo = lo_wg;
    while (lo + 1 < batch && offsets[lo + 1] <= i) ++lo;            // lo_wg <= lo < batch whatever the offsets hold
    const float4 p = *reinterpret_cast<const float4*>(pts + 4 * (size_t)i);       // x, y, z, reflectance (16-byte records)
    int u, v; float d;
    if (!project_point(M, p.x, p.y, p.z, rows, cols, u, v, d)) return;
    if ((unsigned)u < (unsigned)cols && (unsigned)v < (unsigned)rows)             // (as project_scatter_calib_run explains)
        nearest_store(keys, ((size_t)lo * rows + (unsigned)v) * cols + (unsigned)u, d);
}

// k_project_scatter_calib's: the scalar-cache record path with its ballot test and its per-lane fallback.  A frame with a bad
// record scatters nothing: its part of the plane stays zero
__global__ __launch_bounds__(256)
void k_project_nearest_scatter_calib(const float* __restrict__ pts, const int* __restrict__ offsets, int n_points, int batch,
                                     const dcmt_project_calib* __restrict__ table, unsigned* __restrict__ keys, int rows, int cols)
{
    project_scatter_calib_run(pts, offsets, n_points, batch, table, rows, cols,
                              [&](size_t px, unsigned, float d) { nearest_store(keys, px, d); });
}

// k_reproject_scatter's: grid (ceil(n / 1024), frames), four loads in flight per thread.  The stored value is t_2 > 0
__device__ __forceinline__ auto reproject_nearest_store(unsigned* __restrict__ keys, uint32_t dst_rows, uint32_t dst_cols)
{
    unsigned* __restrict__ plane = keys + (size_t)blockIdx.y * dst_rows * dst_cols;
    return [=](size_t px, uint32_t, float t2) { nearest_store(plane, px, t2); };
}

__global__ __launch_bounds__(256)
void k_reproject_nearest_scatter(const float* __restrict__ depth, uint32_t n, uint32_t cols, ReprojK k, unsigned* __restrict__ keys,
                                 uint32_t dst_rows, uint32_t dst_cols)
{
    reproject_scatter_run(depth, n, cols, k, dst_rows, dst_cols, reproject_nearest_store(keys, dst_rows, dst_cols));
}

__global__ __launch_bounds__(256)
void k_reproject_nearest_scatter_calib(const float* __restrict__ depth, uint32_t n, uint32_t cols, const dcmt_reproject_params* __restrict__ table,
                                       unsigned* __restrict__ keys, uint32_t dst_rows, uint32_t dst_cols)
{
    ReprojK k;
    if (!load_reproject_record(table, blockIdx.y, k)) return;
    reproject_scatter_run(depth, n, cols, k, dst_rows, dst_cols, reproject_nearest_store(keys, dst_rows, dst_cols));
}

// One thread per PW neighbouring pixels of the whole batch, in place: n_px is a multiple of PW and the plane aligned to 4 * PW bytes
// (plan::resolve_vec), so an access is inside the plane or the thread has left.  A pixel's word depends on that pixel alone.
template <int PW>
__global__ __launch_bounds__(256)
void k_nearest_fixup(unsigned* __restrict__ plane, size_t n_px)
{
    const size_t i = (blockIdx.x * (size_t)256 + threadIdx.x) * PW;
    if (i >= n_px) return;
    if constexpr (PW == 4) {
        uint4 w = *reinterpret_cast<const uint4*>(plane + i);
        w.x = depth_key_to_bits(w.x); w.y = depth_key_to_bits(w.y); w.z = depth_key_to_bits(w.z); w.w = depth_key_to_bits(w.w);
        *reinterpret_cast<uint4*>(plane + i) = w;
    } else if constexpr (PW == 2) {
        uint2 w = *reinterpret_cast<const uint2*>(plane + i);
        w.x = depth_key_to_bits(w.x); w.y = depth_key_to_bits(w.y);
        *reinterpret_cast<uint2*>(plane + i) = w;
    } else plane[i] = depth_key_to_bits(plane[i]);
}

}  // namespace dcmt
