// dcmt_kernels_normals.h -- the kernel of dcmt_depth_normals_dev and dcmt_depth_normals_calib_dev (include/dcmt.h): the unit normal
// and the plane distance of every pixel of a depth plane from the gradient of its inverse depth, and the flying-pixel filter that
// removes a pixel whose local plane passes closer to the camera centre than min_plane_dist.  Compiled in dcmt_cloud.hip; the return
// test is the planes' (dcmt_kernels_planes.h), a frame's record comes through load_cloud_record (dcmt_calib.h).
//   k_normals<NORMALS, OUT, KSrc>  in the shape of k_gauss5 and k_bilateral5: a wave streams down a strip of 64 columns over a band of
//                     band_rows rows, lane l on column 64 strip + l, EVERY lane an output: a wave's 64 records of a row are 1 KiB
//                     of consecutive 16-byte stores, and its 64 decisions one ballot = two whole words of the mask.  A row is one
//                     coalesced load per lane; the columns left of lane 0 and right of lane 63 come from a second load that only
//                     those two lanes execute.  w = 1 / z is computed once per loaded element (0 for a hole or outside the frame:
//                     a valid w is >= 2^-14) and kept: the row neighbours come through two DPP wave shifts, whose vacated lane
//                     keeps the edge element's w; the rows above and below are rolling registers (the band's two halo rows are
//                     read again by the neighbouring bands: 2 rows in band_rows + 2).  No LDS, no barrier.  The loads of
//                     kNormBatch rows go out together.
//                     NORMALS: the records are written.  OUT: kNormOutNone; kNormOutFused, the filtered plane is written (not over
//                     the input); kNormOutMask, the decisions go to the mask plane [frame][row][words_x] that k_occl_apply
//                     (dcmt_kernels_occlusion.h) then applies to the input itself.  counts: the wave's two sums, one atomic each
//                     where there is something to add.  A pixel's arithmetic does not depend on the strip or the band it falls into.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "dcmt.h"
#include "dcmt_calib.h"
#include "dcmt_kernels_planes.h"
#include "dcmt_normals.h"

namespace dcmt {

constexpr int kNormBatch = 4;                   // (kNormCols, kNormRows: dcmt_normals.h)
enum { kNormOutNone = 0, kNormOutFused = 1, kNormOutMask = 2 };

// the intrinsics as the argument `geo` of k_normals: NormK itself, by value, or the table of per-frame dcmt_cloud_params records
struct NormTable { const dcmt_cloud_params* __restrict__ records; };

// the w of the lane to the left / right; the lane without one (0 / 63) keeps `edge`: the w of the element beyond the strip
__device__ __forceinline__ float norm_left(float w, float edge)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, w), 0x138 /*wave_shr:1*/, 0xf, 0xf, false));
}
__device__ __forceinline__ float norm_right(float w, float edge)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, w), 0x130 /*wave_shl:1*/, 0xf, 0xf, false));
}

// dcmt.h's GRADIENT of one axis: wf / wb the w of the next / previous pixel (0: none).  False where the axis has neither difference
__device__ __forceinline__ bool norm_gradient(float w, float wf, float wb, float& g)
{
    const float F = __fsub_rn(wf, w), B = __fsub_rn(w, wb);
    const bool hf = wf > 0.0f, hb = wb > 0.0f;
    g = hf && (!hb || fabsf(F) <= fabsf(B)) ? F : B;
    return hf || hb;
}

// fsqrt_rn: the correctly rounded f32 square root.  The compiler's own sqrtf, which hipcc rounds correctly by default; the header's
// __fsqrt_rn is the hardware's approximation here (one ulp off at some inputs)
__device__ __forceinline__ float norm_sqrt_rn(float x) { return __builtin_sqrtf(x); }

// a row of a wave as it is kept: the element's bits, its w and the w of its row neighbours
struct NormRow { uint32_t zb; float w, wl, wr; };

// grid (ceil(strips * bands / 4), frames), 256 threads: one wave per (strip, band); strips = ceil(cols / kNormCols),
// bands = ceil(rows / band_rows)
template <bool NORMALS, int OUT, typename KSrc>
__global__ __launch_bounds__(256)
void k_normals(const uint32_t* __restrict__ depth, uint32_t rows, uint32_t cols, uint32_t strips, uint32_t bands, uint32_t band_rows, KSrc geo,
               uint32_t lo_bits, uint32_t hi_bits, float dmin2, uint4* __restrict__ normals, uint32_t* out, uint32_t* __restrict__ mask,
               uint32_t words_x, uint32_t* counts)
{
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), l = threadIdx.x & 63;
    const uint32_t id = blockIdx.x * 4 + wv;
    if (id >= strips * bands) return;
    NormK k;
    bool rec_ok = true;                         // a frame whose record is bad: every valid pixel without a normal, nothing removed
    if constexpr (std::is_same_v<KSrc, NormTable>) {
        CloudK rec;
        rec_ok = load_cloud_record(geo.records, blockIdx.y, rec) &&          // wave-uniform: scalar loads, once per wave
                 normals_intrinsics_ok((uint64_t)__double_as_longlong(rec.fx), (uint64_t)__double_as_longlong(rec.fy),
                                       (uint64_t)__double_as_longlong(rec.cx), (uint64_t)__double_as_longlong(rec.cy));
        k.fx = rec_ok ? __double2float_rn(rec.fx) : 1.0f; k.fy = rec_ok ? __double2float_rn(rec.fy) : 1.0f;
        k.cx = rec_ok ? __double2float_rn(rec.cx) : 0.0f; k.cy = rec_ok ? __double2float_rn(rec.cy) : 0.0f;
    } else {
        k = geo;
    }
    const uint32_t band = id / strips, strip = id - band * strips;
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    const uint32_t* __restrict__ s = depth + fo;
    const uint32_t x = strip * kNormCols + l;
    const bool in_col = x < cols;
    const uint32_t xc = min(x, cols - 1u);
    // the element beyond the strip: column x - 1 for lane 0, x + 1 for lane 63; every other lane holds 0 and never uses it
    const bool is_edge = l == 0u || l == 63u;
    const uint32_t ex = l == 0u ? x - 1u : x + 1u;                     // (x - 1 wraps above cols for x = 0)
    const bool edge_in = is_edge && ex < cols;
    const uint32_t exc = min(ex, cols - 1u);
    const uint32_t y0 = band * band_rows, R = min(band_rows, rows - y0);
    const float dx = __fsub_rn((float)x, k.cx);
    float wp = 0.0f;
    NormRow c = {0u, 0.0f, 0.0f, 0.0f}, n = {0u, 0.0f, 0.0f, 0.0f};
    uint32_t n_removed = 0u, n_none = 0u;
    for (uint32_t i0 = 0; i0 < R + 2u; i0 += kNormBatch) {             // input row i of the band is frame row y0 + i - 1
        uint32_t v[kNormBatch], e[kNormBatch];
        // rows beyond the frame are clamped to something readable; their w is 0
#pragma unroll
        for (int j = 0; j < kNormBatch; ++j) {
            const uint32_t yy = y0 + i0 + (uint32_t)j;                 // frame row + 1
            const size_t ro = (size_t)min(max(yy, 1u) - 1u, rows - 1u) * cols;
            v[j] = s[ro + xc];
            e[j] = edge_in ? s[ro + exc] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kNormBatch; ++j) {
            const uint32_t i = i0 + (uint32_t)j;
            if (i < R + 2u) {                                          // wave-uniform
                const uint32_t yy = y0 + i;
                const bool in_row = yy >= 1u && yy <= rows;
                wp = c.w; c = n;
                n.zb = v[j];
                n.w = in_row && in_col && planes_is_return(v[j], lo_bits, hi_bits) ? __fdiv_rn(1.0f, __uint_as_float(v[j])) : 0.0f;
                const float we = in_row && edge_in && planes_is_return(e[j], lo_bits, hi_bits) ? __fdiv_rn(1.0f, __uint_as_float(e[j])) : 0.0f;
                n.wl = norm_left(n.w, we);
                n.wr = norm_right(n.w, we);
                if (i >= 2u) {                                         // row c: frame row y0 + i - 2
                    const uint32_t y = yy - 2u;
                    const bool valid = c.w > 0.0f;
                    float gx, gy;
                    const bool okx = norm_gradient(c.w, c.wr, c.wl, gx), oky = norm_gradient(c.w, n.w, wp, gy);
                    const bool has = valid && okx && oky && rec_ok;
                    const float a = __fmul_rn(k.fx, gx), b = __fmul_rn(k.fy, gy);
                    const float dy = __fsub_rn((float)y, k.cy);
                    const float cc = __fsub_rn(__fsub_rn(c.w, __fmul_rn(gx, dx)), __fmul_rn(gy, dy));
                    const float len2 = __fadd_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)), __fmul_rn(cc, cc));
                    const bool removed = has && __fmul_rn(len2, dmin2) > 1.0f;
                    n_removed += removed ? 1u : 0u;
                    n_none += valid && !has ? 1u : 0u;
                    const size_t at = fo + (size_t)y * cols + x;
                    if constexpr (NORMALS) {
                        uint4 r = {0u, 0u, 0u, 0u};
                        if (has) {
                            const float dist = __fdiv_rn(1.0f, norm_sqrt_rn(len2));
                            r.x = __float_as_uint(__fmul_rn(-a, dist));
                            r.y = __float_as_uint(__fmul_rn(-b, dist));
                            r.z = __float_as_uint(__fmul_rn(-cc, dist));
                            r.w = __float_as_uint(dist);
                        }
                        if (in_col) normals[at] = r;
                    }
                    if constexpr (OUT == kNormOutFused) {
                        if (in_col) out[at] = removed ? 0u : c.zb;
                    }
                    if constexpr (OUT == kNormOutMask) {
                        const unsigned long long bal = __ballot(removed);
                        uint32_t* word = mask + ((size_t)blockIdx.y * rows + y) * words_x + 2u * strip;
                        if (l == 0u) word[0] = (uint32_t)bal;
                        if (l == 32u && 2u * strip + 1u < words_x) word[1] = (uint32_t)(bal >> 32);
                    }
                }
            }
        }
    }
    if (counts) {                                                      // (the kernel's argument: uniform)
        for (int m = 32; m >= 1; m >>= 1) {
            n_removed += (uint32_t)__shfl_xor((int)n_removed, m, 64);
            n_none += (uint32_t)__shfl_xor((int)n_none, m, 64);
        }
        if (l == 0u && n_removed != 0u) atomicAdd(counts + 2 * (size_t)blockIdx.y, n_removed);
        if (l == 0u && n_none != 0u) atomicAdd(counts + 2 * (size_t)blockIdx.y + 1, n_none);
    }
}

}  // namespace dcmt
