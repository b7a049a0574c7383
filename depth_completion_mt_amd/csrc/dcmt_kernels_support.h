// dcmt_kernels_support.h -- the kernels of dcmt_support_distance_dev and dcmt_support_distance_u16_dev (include/dcmt.h): for every
// pixel the exact squared Euclidean distance D2 to the nearest return of its frame's sparse plane, where that is at most R^2
// (R = max_radius), and what hangs on it: the trust mask of a dense plane and the count of the pixels beyond R.  Compiled in
// dcmt_cloud.hip; the return test is the occlusion filter's (dcmt_kernels_occlusion.h), which is the planes'.
// The transform separates exactly: D2(y, x) = min over k of k^2 + g(y, x + k)^2, where g(y, x) is the distance in rows to the nearest
// return of column x.  A g above R can never give a D2 <= R^2, so g is capped at R + 1 <= 256 and kept as uint16: one route for
// every R, and 255 is told from "none within reach" (256) without a second plane.
//   k_support_cols<T, BALLOTS>  pass A, one wave per strip of 64 columns, lane = column, rows in order, row reads coalesced, issued
//                     kSupportChunk rows at a time.  Down: "rows since the last return", capped, written as g_down; each row's
//                     ballot of returns is left in LDS (8 bytes a row).  Up: the same count from below over those ballots, and
//                     g = min(g_down, g_up) over the g_down the lane wrote itself, stored where it is smaller.  So the sparse plane
//                     is read once.  Not BALLOTS (more than kSupportLdsRows rows): the up sweep reads the plane again instead; the
//                     same bytes.
//   k_support_rows    pass B, one workgroup per segment of kSupportTile columns, lane = pixel, a band of kSupportBand consecutive rows
//                     at a time and kSupportGroup bands one after another: the next band's loads are in flight while this one is
//                     worked on.  G = g^2 of the band's segments with a halo of R columns either side is staged in LDS (65536 for
//                     a column outside the frame: skipped, as it can never win), and the smallest of all of it, F, is kept.  A lane
//                     starts with best = G of its own column and for k = 1, 2, ... takes min(best, k^2 + G(x - k), k^2 + G(x + k))
//                     while k <= R and k^2 + F < min(best, R^2 + 1): exact for every D2 <= R^2, because a column k away gives
//                     at least k^2 + F, and a pixel that cannot come within R any more is written as the marker whatever its
//                     distance.  The band's rows run side by side (independent LDS reads), until the last of them stops; a
//                     candidate past a row's own stop changes nothing.  The same kernel writes dist2, selects into out and counts:
//                     integer adds, reduced per wave, one atomic a wave.  In place (out == dense) a pixel within reach is neither
//                     read nor written.
// T: uint32_t (the bits of an f32 plane) or uint16_t (the KITTI payload, metres = value * scale as dcmt_complete_u16_dev ingests it).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dcmt.h"
#include "dcmt_kernels_occlusion.h"
#include "dcmt_support.h"

namespace dcmt {

// grid (ceil(cols / 64), frames), 64 threads, support_cols_lds_bytes(rows) of dynamic LDS; cap = R + 1
template <typename T, bool BALLOTS>
__global__ __launch_bounds__(64)
void k_support_cols(const T* __restrict__ in, uint32_t rows, uint32_t cols, uint32_t cap, uint32_t lo_bits, uint32_t hi_bits, float scale,
                    uint16_t* __restrict__ g)
{
    extern __shared__ unsigned long long support_ballots[];
    const uint32_t lane = threadIdx.x, x = blockIdx.x * kSupportColsWave + lane;
    const bool incol = x < cols;
    const size_t fo = (size_t)blockIdx.y * rows * cols + min(x, cols - 1u);          // loads are unconditional, from clamped addresses
    const T* fin = in + fo;
    uint16_t* fg = g + fo;
    uint32_t d = cap;
    for (uint32_t y0 = 0; y0 < rows; y0 += kSupportChunk) {
        T v[kSupportChunk];
#pragma unroll
        for (int i = 0; i < kSupportChunk; ++i) v[i] = fin[(size_t)min(y0 + (uint32_t)i, rows - 1u) * cols];
#pragma unroll
        for (int i = 0; i < kSupportChunk; ++i) {
            const uint32_t y = y0 + (uint32_t)i;
            if (y < rows) {                     // the whole wave
                const bool ret = incol && occl_is_return<T>(v[i], scale, lo_bits, hi_bits);
                if constexpr (BALLOTS) {
                    const unsigned long long b = __ballot(ret);
                    if (lane == 0u) support_ballots[y] = b;
                }
                d = ret ? 0u : min(d + 1u, cap);
                if (incol) fg[(size_t)y * cols] = (uint16_t)d;
            }
        }
    }
    __syncthreads();                            // (one wave: the ballots are its own)
    uint32_t u = cap;
    for (uint32_t c = (rows + kSupportChunk - 1u) / kSupportChunk; c-- > 0u;) {
        const uint32_t y0 = c * kSupportChunk;
        uint32_t gd[kSupportChunk];
        unsigned long long b[kSupportChunk];
        T v[kSupportChunk];
#pragma unroll
        for (int i = 0; i < kSupportChunk; ++i) {
            const uint32_t yy = min(y0 + (uint32_t)i, rows - 1u);
            gd[i] = fg[(size_t)yy * cols];      // a lane outside the frame reads the last column's, and stores nothing
            if constexpr (BALLOTS) b[i] = support_ballots[yy];
            else v[i] = fin[(size_t)yy * cols];
        }
#pragma unroll
        for (int i = kSupportChunk - 1; i >= 0; --i) {
            const uint32_t y = y0 + (uint32_t)i;
            if (y < rows) {
                bool ret;
                if constexpr (BALLOTS) ret = ((b[i] >> lane) & 1ull) != 0ull;
                else ret = incol && occl_is_return<T>(v[i], scale, lo_bits, hi_bits);
                u = ret ? 0u : min(u + 1u, cap);
                if (incol && u < gd[i]) fg[(size_t)y * cols] = (uint16_t)u;
            }
        }
    }
}

// grid (tiles_x * groups, frames), 256 threads, support_rows_lds_bytes(R) of dynamic LDS.  dense, fallback, out: the bits of f32
// planes, copied opaquely; out may be dense (neither is restrict).  Any of dist2, out, beyond may be null; dense is given with out.
__global__ __launch_bounds__(256)
void k_support_rows(const uint16_t* __restrict__ g, uint32_t rows, uint32_t cols, uint32_t tiles_x, int R, const uint32_t* dense,
                    const uint32_t* __restrict__ fallback, uint32_t* out, uint16_t* __restrict__ dist2, uint32_t* beyond)
{
    extern __shared__ uint32_t support_sq[];
    __shared__ uint32_t wave_min[4];
    const uint32_t W = (uint32_t)(kSupportTile + 2 * R);
    const uint32_t tg = blockIdx.x / tiles_x, tx = blockIdx.x - tg * tiles_x;
    const int x0 = (int)(tx * kSupportTile) - R;
    const uint32_t bands = (rows + kSupportBand - 1u) / kSupportBand, band0 = tg * kSupportGroup;
    const uint32_t nb = min((uint32_t)kSupportGroup, bands - band0);
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    const uint32_t x = tx * kSupportTile + threadIdx.x, rr = (uint32_t)(R * R);
    // W <= 256 + 2 * 255: at most kSupportSlots columns of a row per lane.  All loads of a band are issued before the first of them
    // is used (from clamped addresses; a slot past W is skipped by whole waves but the one it ends in)
    uint32_t v[kSupportBand][kSupportSlots];
    auto load_band = [&](uint32_t band) {
#pragma unroll
        for (int r = 0; r < kSupportBand; ++r) {
            const uint16_t* row = g + fo + (size_t)min(band * kSupportBand + (uint32_t)r, rows - 1u) * cols;
#pragma unroll
            for (int j = 0; j < kSupportSlots; ++j) {
                const uint32_t c = threadIdx.x + 256u * (uint32_t)j;
                v[r][j] = c < W ? (uint32_t)row[min(max(x0 + (int)c, 0), (int)cols - 1)] : 0u;
            }
        }
    };
    load_band(band0);
    const uint32_t* s = support_sq + threadIdx.x + (uint32_t)R;          // the lane's own column in the band's first row
    uint32_t cnt = 0u;
    for (uint32_t b = 0; b < nb; ++b) {
        uint32_t lo = 65536u;
#pragma unroll
        for (int r = 0; r < kSupportBand; ++r) {
#pragma unroll
            for (int j = 0; j < kSupportSlots; ++j) {
                const uint32_t c = threadIdx.x + 256u * (uint32_t)j;
                const int gx = x0 + (int)c;
                if (c < W) {
                    const uint32_t sq = gx >= 0 && gx < (int)cols ? v[r][j] * v[r][j] : 65536u;
                    support_sq[(uint32_t)r * W + c] = sq;
                    lo = min(lo, sq);
                }
            }
        }
        for (int m = 32; m >= 1; m >>= 1) lo = min(lo, (uint32_t)__shfl_xor((int)lo, m, 64));
        if ((threadIdx.x & 63u) == 0u) wave_min[threadIdx.x >> 6] = lo;
        __syncthreads();
        if (b + 1u < nb) load_band(band0 + b + 1u);                      // in flight while this band is worked on
        const uint32_t floor_sq = min(min(wave_min[0], wave_min[1]), min(wave_min[2], wave_min[3]));
        uint32_t best[kSupportBand];
#pragma unroll
        for (int r = 0; r < kSupportBand; ++r) best[r] = s[(uint32_t)r * W];
        for (int k = 1; k <= R; ++k) {
            const uint32_t kk = (uint32_t)(k * k);
            uint32_t open = min(best[0], rr + 1u);
#pragma unroll
            for (int r = 1; r < kSupportBand; ++r) open = max(open, min(best[r], rr + 1u));
            if (kk + floor_sq >= open) break;
#pragma unroll
            for (int r = 0; r < kSupportBand; ++r) best[r] = min(best[r], kk + min(s[(int)((uint32_t)r * W) - k], s[(int)((uint32_t)r * W) + k]));
        }
        const uint32_t y0 = (band0 + b) * kSupportBand;
#pragma unroll
        for (int r = 0; r < kSupportBand; ++r) {
            const uint32_t y = y0 + (uint32_t)r;
            if (x < cols && y < rows) {
                const bool far = best[r] > rr;
                const size_t i = fo + (size_t)y * cols + x;
                if (dist2) dist2[i] = (uint16_t)(far ? kSupportBeyond : best[r]);
                if (out) {
                    if (out == dense) {
                        if (far) out[i] = fallback ? fallback[i] : 0u;
                    } else {
                        out[i] = far ? (fallback ? fallback[i] : 0u) : dense[i];
                    }
                }
                cnt += far ? 1u : 0u;
            }
        }
        __syncthreads();                        // the next band overwrites what this one read
    }
    if (beyond) {                               // (the whole grid's)
        for (int m = 32; m >= 1; m >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, m, 64);
        if ((threadIdx.x & 63u) == 0u && cnt != 0u) atomicAdd(beyond + blockIdx.y, cnt);
    }
}

}  // namespace dcmt
