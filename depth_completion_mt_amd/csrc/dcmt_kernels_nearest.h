// dcmt_kernels_nearest.h -- the two geometric scatter calls under the rule every producer of sparse depth uses: a pixel hit by
// several points (dcmt_project_points_nearest*_dev) or source pixels (dcmt_reproject_depth_nearest*_dev) keeps the NEAREST, the
// smallest of the values the last-wins kernels (k_project_scatter, dcmt_kernels_project.h; k_reproject_scatter,
// dcmt_kernels_reproject.h) would have stored there.  A point or pixel is transformed, accepted and rejected by the very statements
// of those kernels -- project_scatter_run / project_scatter_calib_run (dcmt_project.h), reproject_scatter_run -- so the set of occupied
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

#include <type_traits>

#include "dcmt_depth_key.h"
#include "dcmt_kernels_reproject.h"
#include "dcmt_project.h"

namespace dcmt {

// what every scatter kernel here does at a landing pixel of the key plane
__device__ __forceinline__ void nearest_store(unsigned* __restrict__ keys, size_t px, float v)
{
    atomicMax(&keys[px], depth_key(__float_as_uint(v)));
}

// k_project_scatter's shape, instance by instance: ProjMats -- one point per thread, the workgroup's frame search over d_offsets
// (project_scatter_run); ProjTable -- the scalar-cache record path with its ballot test and its per-lane fallback
// (project_scatter_calib_run), where a frame with a bad record scatters nothing: its part of the plane stays zero.  keys: the output
// plane, [batch][rows][cols], zeroed
template <typename MSrc = ProjMats>
__global__ __launch_bounds__(256)
void k_project_nearest_scatter(const float* __restrict__ pts, const int* __restrict__ offsets, int n_points, int batch,
                               MSrc geo, unsigned* __restrict__ keys, int rows, int cols)
{
    if constexpr (std::is_same_v<MSrc, ProjTable>)
        project_scatter_calib_run(pts, offsets, n_points, batch, geo.records, rows, cols,
                                  [&](size_t px, unsigned, float d) { nearest_store(keys, px, d); });
    else
        project_scatter_run(pts, offsets, n_points, batch, geo, rows, cols, [=](int lo, int u, int v, int, float d) {
            if ((unsigned)u < (unsigned)cols && (unsigned)v < (unsigned)rows)     // (as project_scatter_calib_run explains)
                nearest_store(keys, ((size_t)lo * rows + (unsigned)v) * cols + (unsigned)u, d);
        });
}

// k_reproject_scatter's: grid (ceil(n / 1024), frames), four loads in flight per thread.  The stored value is t_2 > 0
__device__ __forceinline__ auto reproject_nearest_store(unsigned* __restrict__ keys, uint32_t dst_rows, uint32_t dst_cols)
{
    unsigned* __restrict__ plane = keys + (size_t)blockIdx.y * dst_rows * dst_cols;
    return [=](size_t px, uint32_t, float t2) { nearest_store(plane, px, t2); };
}

template <typename KSrc = ReprojK>
__global__ __launch_bounds__(256)
void k_reproject_nearest_scatter(const float* __restrict__ depth, uint32_t n, uint32_t cols, KSrc geo, unsigned* __restrict__ keys,
                                 uint32_t dst_rows, uint32_t dst_cols)
{
    [[maybe_unused]] ReprojK rec;
    if constexpr (std::is_same_v<KSrc, ReprojTable>)
        if (!load_reproject_record(geo.records, blockIdx.y, rec)) return;
    reproject_scatter_run(depth, n, cols, reproj_k(geo, rec), dst_rows, dst_cols, reproject_nearest_store(keys, dst_rows, dst_cols));
}

// One thread per PW neighbouring pixels of the whole batch, in place: n_px is a multiple of PW and the plane aligned to 4 * PW bytes
// (plan::resolve_vec), so an access is inside the plane or the thread has left.  A pixel's word depends on that pixel alone.
template <int PW>
__global__ __launch_bounds__(256)
void k_nearest_fixup(unsigned* __restrict__ plane, size_t n_px)
{
    const size_t i = (blockIdx.x * (size_t)256 + threadIdx.x) * PW;
    if (i >= n_px) return;
    uint32_t w[PW];
    load_words<PW>(plane + i, w);
#pragma unroll
    for (int j = 0; j < PW; ++j) w[j] = depth_key_to_bits(w[j]);
    store_words<PW>(plane + i, w);
}

}  // namespace dcmt
