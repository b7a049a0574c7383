// dcmt_kernels_reproject.h -- the data part of unrectify_sol (DC_stereo_lidar/main_sl.cpp:967-1028, called at :1228): a dense
// depth plane seen by one camera, forward-warped into the depth plane another camera sees.  Per source pixel (row y, column x),
// exactly the reference's statements:
//     z  = depth                                                                                     (:986-988)
//     x_ = (float)(((double)x - cx) * (double)z / fx),  y_ likewise with y, cy, fy                    (:989-990)  unproject_axis
//     t_i = ((M[i][0]*x_ + M[i][1]*y_) + M[i][2]*z) + M[i][3]        i = 0, 1, 2                     (:993)      dot4_rn
//     skip unless t_2 > 0            -- the only validity test: there is no depth > 0 filter          (:999)
//     c_i = (K[i][0]*t_0 + K[i][1]*t_1) + K[i][2]*t_2                i = 0, 1                        (:1000)     dot3_rn
//     uf = c_0 / t_2,  vf = c_1 / t_2                                ("* 1.f" is exact)               (:1001)     __fdiv_rn
//     skip unless 0 <= uf < (float)dst_cols and 0 <= vf < (float)dst_rows                             (:1008-1009)
//     dst[(int)vf][(int)uf] = t_2                                                                    (:1011-1015)
// in row-major source order, so a later source pixel overwrites an earlier one that fell into the same destination pixel.
//
// Two passes, the shape of N2 (k_project_scatter / k_project_resolve, dcmt_kernels_project.h), on the same winner plane:
//   k_reproject_scatter   per source pixel: atomicMax of the tag generation | frame-local source pixel index into the winner plane
//                         at the destination pixel (no value returned).  The largest index is the last writer; an integer max does
//                         not depend on arrival order, so the result is the same bits on every run.
//   k_reproject_resolve   per destination pixel: a tag of this call's generation -> reload the winner's depth and recompute t_2
//                         (the same operations in the same order); anything else -> 0.  The destination is written completely.
// The library is built with -ffinite-math-only, so the compiler may reason about uf and vf as if they were finite: the address is
// formed only after (unsigned)u < dst_cols && (unsigned)v < dst_rows has held in the integer domain as well.
// Bytes per source pixel (s) and destination pixel (d): 4 s (read) + 4 per landing pixel (atomics) + 8 d (tag read, result write)
// + 4 per destination pixel that has a winner (the gather of its depth).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dcmt_calib.h"
#include "dcmt_cloud.h"
#include "dcmt_dot_rn.h"
#include "dcmt_kernels_cloud.h"

namespace dcmt {

// t_2 of a source pixel: what the scatter stores the index of and the resolve writes
__device__ __forceinline__ float reproject_t2(const ReprojK& k, uint32_t x, uint32_t y, float z, float& x_, float& y_)
{
    x_ = unproject_axis(x, k.cx, (double)z, k.fx);
    y_ = unproject_axis(y, k.cy, (double)z, k.fy);
    return dot4_rn(k.M + 8, x_, y_, z);
}

// grid (ceil(n / 1024), frames), 256 threads; n = src_rows * src_cols.  A workgroup owns 1024 consecutive pixels of its frame and
// thread t takes pixels t, t + 256, t + 512, t + 768 of them: four independent coalesced dword loads in flight per thread (the
// pattern of k_minmax), and the 64 atomics of a wave instruction start from 64 consecutive source pixels, so under a near-identity
// warp they hit runs of consecutive dwords of the winner plane.  store(pixel, q, t_2): what is done at the landing pixel (its index in
// the frame's destination plane) -- the tag here, the depth's key in the nearest-wins kernels (dcmt_kernels_nearest.h).
template <typename Store>
__device__ __forceinline__ void reproject_scatter_run(const float* __restrict__ depth, uint32_t n, uint32_t cols, const ReprojK& k,
                                                      uint32_t dst_rows, uint32_t dst_cols, Store store)
{
    const uint32_t q0 = blockIdx.x * (uint32_t)kReprojectPxPerWg + threadIdx.x;
    const float* __restrict__ p = depth + (size_t)blockIdx.y * n;
    float zr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) zr[r] = q0 + 256u * r < n ? p[q0 + 256u * r] : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float z = zr[r];
        const uint32_t q = q0 + 256u * r;                     // frame-local source pixel index
        if (q >= n) continue;
        const uint32_t y = q / cols, x = q - y * cols;
        float x_, y_;
        const float t2 = reproject_t2(k, x, y, z, x_, y_);
        if (!(t2 > 0.0f)) continue;                                                               // :999
        const float t0 = dot4_rn(k.M, x_, y_, z), t1 = dot4_rn(k.M + 4, x_, y_, z);
        const float uf = __fdiv_rn(dot3_rn(k.K, t0, t1, t2), t2), vf = __fdiv_rn(dot3_rn(k.K + 3, t0, t1, t2), t2);
        if (!(uf >= 0.0f && uf < (float)dst_cols && vf >= 0.0f && vf < (float)dst_rows)) continue;   // :1008-1009
        const int u = (int)uf, v = (int)vf;
        if ((unsigned)u < dst_cols && (unsigned)v < dst_rows)
            store((size_t)v * dst_cols + (unsigned)u, q, t2);
    }
}

// the store of the last-wins kernels: the tag of the call's generation and the source pixel's index
__device__ __forceinline__ auto reproject_tag_store(unsigned* __restrict__ winner, uint32_t dst_rows, uint32_t dst_cols, unsigned gen_tag)
{
    unsigned* __restrict__ win = winner + (size_t)blockIdx.y * dst_rows * dst_cols;
    return [=](size_t px, uint32_t q, float) { atomicMax(&win[px], gen_tag | q); };
}

// The record as the kernels' argument `geo`, the idiom of k_cloud_scatter (dcmt_kernels_cloud.h): ReprojK itself, by value
// (dcmt_reproject_depth*_dev), or a table of per-frame records (dcmt_reproject_depth*_calib_dev, dcmt_calib.h)
struct ReprojTable { const dcmt_reproject_params* __restrict__ records; };
__device__ __forceinline__ const ReprojK& reproj_k(const ReprojK& arg, const ReprojK&) { return arg; }
__device__ __forceinline__ const ReprojK& reproj_k(const ReprojTable&, const ReprojK& rec) { return rec; }

// ReprojTable: the frame's own record, record blockIdx.y of the table, loaded once per wave through the scalar cache in front of the
// pixel loop.  A frame with a bad record scatters nothing: its part of the winner plane keeps no tag of this generation and
// k_reproject_resolve writes zeros there
template <typename KSrc = ReprojK>
__global__ __launch_bounds__(256)
void k_reproject_scatter(const float* __restrict__ depth, uint32_t n, uint32_t cols, KSrc geo, unsigned* __restrict__ winner,
                         uint32_t dst_rows, uint32_t dst_cols, unsigned gen_tag)
{
    [[maybe_unused]] ReprojK rec;
    if constexpr (std::is_same_v<KSrc, ReprojTable>)
        if (!load_reproject_record(geo.records, blockIdx.y, rec)) return;
    reproject_scatter_run(depth, n, cols, reproj_k(geo, rec), dst_rows, dst_cols, reproject_tag_store(winner, dst_rows, dst_cols, gen_tag));
}

// One thread per PW neighbouring destination pixels of the whole batch (a thread's pixels may lie in two frames): 8- / 16-byte
// accesses where the batch's pixel count and d_out's alignment allow, the scheme of k_project_resolve.  dst_n = dst_rows * dst_cols,
// n_px = frames * dst_n.
// ReprojTable: the record of each pixel's OWN frame, the scheme of k_project_resolve<PW, ProjTable> (dcmt_kernels_project.h): the
// frame of the wave's first pixel and that pixel's place in it from one division per wave on the scalar unit; where the wave's
// 64 * PW pixels end inside that frame -- almost always -- its record comes through the scalar cache once per wave, as the by-value
// argument of the uniform instance does, and no lane divides.  Otherwise each lane finds the frame of its first pixel and each pixel
// that holds a winner gathers the 48 bytes reproject_t2 reads from its own frame's record.  Either way the arithmetic is
// reproject_t2's.
template <int PW, typename KSrc = ReprojK>
__global__ __launch_bounds__(256)
void k_reproject_resolve(const float* __restrict__ depth, uint32_t n, uint32_t cols, KSrc geo, const unsigned* __restrict__ winner,
                         float* __restrict__ out, uint32_t dst_n, size_t n_px, unsigned gen_tag, int idx_bits)
{
    constexpr bool kTable = std::is_same_v<KSrc, ReprojTable>;
    const uint32_t l = threadIdx.x & 63;
    const size_t i_wave = (blockIdx.x * (size_t)256 + __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u)) * PW;     // the wave's first pixel
    const size_t i = kTable ? i_wave + (size_t)l * PW : (blockIdx.x * (size_t)256 + threadIdx.x) * PW;
    if (i >= n_px) return;
    uint32_t w[PW], o[PW];
    load_words<PW>(winner + i, w);
    const unsigned mask = (1u << idx_bits) - 1u;
    std::conditional_t<kTable, uint32_t, size_t> f;           // the frame of the thread's first pixel (as wide as the division it comes
    uint32_t r;                                               // from: 32 bits behind the wave's, 64 without), and the pixel's place in it
    bool one_frame = false;                                   // (table) the wave's pixels lie in one frame, whose record is in `rec`
    [[maybe_unused]] ReprojK rec;
    if constexpr (kTable) {
        const uint32_t f_wave = (uint32_t)(i_wave / dst_n);                       // i_wave < n_px here, so f_wave < frames
        const uint32_t r_wave = (uint32_t)(i_wave - (size_t)f_wave * dst_n);
        one_frame = r_wave + 64u * PW <= dst_n;                                   // (a frame has < 2^29 pixels: no overflow)
        f = f_wave; r = r_wave + l * PW;                                          // r < dst_n + 256
        if (one_frame) load_reproject_t2_record(geo.records, f_wave, rec);
        else { const uint32_t df = r / dst_n; f += df; r -= df * dst_n; }         // i < n_px, so f < frames, and so is every frame below:
    } else {                                                                      // i + PW <= n_px (the pixel count is a multiple of PW)
        f = i / dst_n;
        r = (uint32_t)(i - f * dst_n);
    }
#pragma unroll
    for (int j = 0; j < PW; ++j) {
        if (!one_frame && j > 0 && ++r == dst_n) { r = 0; ++f; }
        o[j] = 0u;
        const uint32_t q = w[j] & mask;
        if ((w[j] & ~mask) == gen_tag && q < n) {             // (q < n holds for every tag this call's scatter wrote)
            if constexpr (kTable)
                if (!one_frame) load_reproject_t2_record(geo.records, f, rec);
            const float z = depth[(size_t)f * n + q];
            const uint32_t y = q / cols, x = q - y * cols;
            float x_, y_;
            o[j] = __float_as_uint(reproject_t2(reproj_k(geo, rec), x, y, z, x_, y_));
        }
    }
    store_words<PW>(reinterpret_cast<uint32_t*>(out) + i, o);
}

}  // namespace dcmt
