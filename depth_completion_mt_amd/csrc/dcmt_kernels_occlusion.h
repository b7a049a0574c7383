// dcmt_kernels_occlusion.h -- the kernels of dcmt_sparse_occlusion_dev and dcmt_sparse_occlusion_u16_dev (include/dcmt.h): a return of
// a sparse depth plane is removed where a nearer return in the clipped window (2 rx + 1) x (2 ry + 1) around it has a code more than
// tol_code above its own.  Compiled in dcmt_cloud.hip; the return test and the code are the planes' (dcmt_kernels_planes.h).
//   k_occl<T, FUSED>  one workgroup per tile of 64 x 64 pixels, lane = column, a wave 16 rows.  A lane reads its 16 pixels once and
//                     keeps them and their codes in registers; the codes of the tile and of its halo are staged in LDS (0 for a
//                     pixel that is no return or lies outside the frame: the window is clipped, and 0 never wins a maximum).  A
//                     wave then takes the maximum over 2 rx + 1 columns of every fourth row of that block, in place, and after a barrier
//                     lane x takes the maximum over 2 ry + 1 of those row maxima for its 16 pixels.  Integer maxima on codes: NaN
//                     handling never enters.  FUSED (out of place): the pixel is written, 0 where it is occluded, and the
//                     workgroup's count goes to removed with one atomic.  Not FUSED (in place): the decision of 64 pixels of a row is one
//                     ballot, stored as two 32-bit words of the mask plane [frame][row][words_x]; nothing of `in` is written,
//                     so a neighbouring workgroup's halo is the input whatever the order.
//   k_occl_apply<T>   one lane per mask word: a set bit zeroes its pixel, the words' population counts go to removed, one atomic a workgroup.  A pixel
//                     that stays is not touched at all.
// T: uint32_t (the bits of an f32 plane) or uint16_t (the KITTI payload, metres = value * scale as dcmt_complete_u16_dev ingests it).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dcmt.h"
#include "dcmt_kernels_planes.h"
#include "dcmt_occlusion.h"

namespace dcmt {

// the bits of an element's depth: its own (an f32 plane), or of the payload's ingest, the f32 product rounded once
template <typename T>
__device__ __forceinline__ uint32_t occl_depth_bits(T v, float scale)
{
    if constexpr (sizeof(T) == 4) return v;
    else return __float_as_uint(__fmul_rn((float)v, scale));
}

// an element is a return: the planes' test on its depth (dcmt_kernels_support.h shares it)
template <typename T>
__device__ __forceinline__ bool occl_is_return(T v, float scale, uint32_t lo_bits, uint32_t hi_bits)
{
    return planes_is_return(occl_depth_bits<T>(v, scale), lo_bits, hi_bits);
}

// the code of an element: the planes' code of its depth where that is a return, else 0
template <typename T>
__device__ __forceinline__ uint32_t occl_code(T v, float scale, uint32_t lo_bits, uint32_t hi_bits)
{
    const uint32_t zb = occl_depth_bits<T>(v, scale);
    return planes_is_return(zb, lo_bits, hi_bits) ? planes_code(zb) : 0u;
}

// the workgroup's sum of cnt into *total: reduced per wave, the four waves' sums added in LDS (*wg, which thread 0 cleared in front
// of an earlier barrier), then one global atomic where there is something to add.  Every thread of the workgroup calls it.
__device__ __forceinline__ void occl_count(uint32_t cnt, uint32_t* wg, uint32_t* total)
{
    for (int m = 32; m >= 1; m >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, m, 64);
    if ((threadIdx.x & 63) == 0 && cnt != 0u) atomicAdd(wg, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && *wg != 0u) atomicAdd(total, *wg);
}

// grid (tiles_x * tiles_y, frames), 256 threads, occl_lds_bytes(rx, ry) of dynamic LDS
template <typename T, bool FUSED>
__global__ __launch_bounds__(256)
void k_occl(const T* __restrict__ in, uint32_t rows, uint32_t cols, uint32_t tiles_x, int rx, int ry, uint32_t tol, uint32_t lo_bits,
            uint32_t hi_bits, float scale, T* __restrict__ out, uint32_t* __restrict__ mask, uint32_t words_x, uint32_t* removed)
{
    extern __shared__ uint32_t occl_lds[];
    __shared__ uint32_t wg_count;
    if (threadIdx.x == 0) wg_count = 0u;
    const uint32_t W = (uint32_t)(kOcclTile + 2 * rx), Ht = (uint32_t)(kOcclTile + 2 * ry);
    uint32_t* C = occl_lds;                     // [Ht][W] codes; then, in the first 64 columns of every row, the maxima over 2 rx + 1 columns
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = (int)(tx * kOcclTile) - rx, y0 = (int)(ty * kOcclTile) - ry;
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t x = tx * kOcclTile + lane, r0 = wave * kOcclRun, ytop = ty * kOcclTile + r0;
    const T* fin = in + fo;
    // the code of pixel (gy, gx), 0 outside the frame: the load is clamped into the frame and unconditional, so that the loads of an
    // unrolled loop are all in flight before the first of them is used
    auto code_at = [&](int gy, int gx) -> uint32_t {
        const bool inside = gx >= 0 && gx < (int)cols && gy >= 0 && gy < (int)rows;
        const T e = fin[(size_t)min(max(gy, 0), (int)rows - 1) * cols + (uint32_t)min(max(gx, 0), (int)cols - 1)];
        return inside ? occl_code<T>(e, scale, lo_bits, hi_bits) : 0u;
    };
    // the lane's own 16 pixels: read once, kept for the store, their codes kept for the decision
    T v[kOcclRun];
    uint32_t w[kOcclRun];
    const uint32_t xc = min(x, cols - 1u);
#pragma unroll
    for (int i = 0; i < kOcclRun; ++i) v[i] = fin[(size_t)min(ytop + (uint32_t)i, rows - 1u) * cols + xc];
#pragma unroll
    for (int i = 0; i < kOcclRun; ++i) {
        w[i] = x < cols && ytop + (uint32_t)i < rows ? occl_code<T>(v[i], scale, lo_bits, hi_bits) : 0u;
        C[(r0 + (uint32_t)(i + ry)) * W + lane + (uint32_t)rx] = w[i];
    }
    // the ry rows above and the ry rows below the tile, its own 64 columns: a wave takes every fourth of them
#pragma unroll 4
    for (uint32_t hr = wave; hr < 2u * (uint32_t)ry; hr += 4u) {
        const uint32_t yy = hr < (uint32_t)ry ? hr : hr + kOcclTile;
        C[yy * W + lane + (uint32_t)rx] = code_at(y0 + (int)yy, (int)x);
    }
    // the rx columns left and the rx columns right of it, all rows of the block, row-major over the 2 rx columns of a row
    if (rx > 0) {
        const uint32_t n2 = 2u * (uint32_t)rx, dy = 256u / n2, dx = 256u - dy * n2;
        uint32_t yy = threadIdx.x / n2, j = threadIdx.x - yy * n2;
#pragma unroll 2
        while (yy < Ht) {
            const uint32_t xx = j < (uint32_t)rx ? j : j + kOcclTile;
            C[yy * W + xx] = code_at(y0 + (int)yy, x0 + (int)xx);
            j += dx; yy += dy;
            if (j >= n2) { j -= n2; ++yy; }
        }
    }
    __syncthreads();
    // the maxima over 2 rx + 1 columns, four rows of the block at a time (independent reads), written over the codes of the row: a row
    // is one wave's alone here, and the wave has read all of it before it writes (the lanes' own codes are in w by now)
    for (uint32_t yy = wave; yy < Ht; yy += 16u) {
        uint32_t m[4] = {0u, 0u, 0u, 0u}, at[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) at[q] = min(yy + 4u * (uint32_t)q, Ht - 1u) * W + lane;
        for (int k = 0; k <= 2 * rx; ++k) {
#pragma unroll
            for (int q = 0; q < 4; ++q) m[q] = max(m[q], C[at[q] + (uint32_t)k]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (yy + 4u * (uint32_t)q < Ht) C[(yy + 4u * (uint32_t)q) * W + lane] = m[q];
    }
    __syncthreads();
    // the maxima over 2 ry + 1 of those, for the lane's 16 pixels at once
    uint32_t m[kOcclRun];
#pragma unroll
    for (int i = 0; i < kOcclRun; ++i) m[i] = 0u;
    const uint32_t* h = C + r0 * W + lane;
    for (int k = 0; k <= 2 * ry; ++k) {
#pragma unroll
        for (int i = 0; i < kOcclRun; ++i) m[i] = max(m[i], h[(uint32_t)(k + i) * W]);
    }
    uint32_t cnt = 0u;
#pragma unroll
    for (int i = 0; i < kOcclRun; ++i) {
        const uint32_t y = ytop + (uint32_t)i;
        const bool occluded = w[i] != 0u && m[i] - w[i] > tol;        // w is 0 outside the frame: never occluded
        if constexpr (FUSED) {
            if (x < cols && y < rows) out[fo + (size_t)y * cols + x] = occluded ? (T)0 : v[i];
            cnt += occluded ? 1u : 0u;
        } else {
            const unsigned long long b = __ballot(occluded);
            if (y < rows) {                     // the whole wave
                uint32_t* word = mask + ((size_t)blockIdx.y * rows + y) * words_x + 2u * tx;
                if (lane == 0u) word[0] = (uint32_t)b;
                if (lane == 32u && 2u * tx + 1u < words_x) word[1] = (uint32_t)(b >> 32);
            }
        }
    }
    if constexpr (FUSED)
        if (removed) occl_count(cnt, &wg_count, removed + blockIdx.y);         // (removed is the whole grid's: the barrier inside is uniform)
}

// grid (ceil(rows * words_x / 256), frames), 256 threads
template <typename T>
__global__ __launch_bounds__(256)
void k_occl_apply(const uint32_t* __restrict__ mask, uint32_t rows, uint32_t cols, uint32_t words_x, T* __restrict__ out, uint32_t* removed)
{
    __shared__ uint32_t wg_count;
    if (threadIdx.x == 0) wg_count = 0u;
    __syncthreads();
    const size_t n = (size_t)rows * words_x, i = (size_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t bits = i < n ? mask[(size_t)blockIdx.y * n + i] : 0u;
    const uint32_t cnt = (uint32_t)__popc(bits);
    if (bits != 0u) {
        const uint32_t y = (uint32_t)(i / words_x), xw = (uint32_t)(i - (size_t)y * words_x);
        T* o = out + ((size_t)blockIdx.y * rows + y) * cols + 32u * xw;
        do {
            o[__ffs((int)bits) - 1] = (T)0;     // a set bit is a return of the frame: below cols
            bits &= bits - 1u;
        } while (bits != 0u);
    }
    if (removed) occl_count(cnt, &wg_count, removed + blockIdx.y);
}

}  // namespace dcmt
