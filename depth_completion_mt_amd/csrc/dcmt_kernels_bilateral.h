// dcmt_kernels_bilateral.h -- the bilateral finish of img_completion.cpp:174, cv::bilateralFilter(dense, copy of dense, 5, sigma_color,
// sigma_space), as this project states it (OpenCV's interpolated exp table is not restated):
//   taps     the 13 offsets (dy, dx) with dy*dy + dx*dx <= 4, BORDER_REFLECT_101 on both axes (reflect101, dcmt_gauss.h)
//   weights  ws(dy, dx) = (float)exp(-(dy*dy + dx*dx) / (2 sigma_space^2)), computed in double by the host (BilK);
//            wc = exp(gc * d * d), d = v(tap) - v(centre), gc = -0.5f / sigma_color^2, all in f32
//   output   y = c + (sum ws wc d) / (sum ws wc), both sums in tap order (row-major); the centre tap adds d = 0, w = 1.  A constant
//            plane comes back bit for bit.
// Compiled into the code object of dcmt_cloud.hip, in the shape of k_gauss5 (dcmt_kernels_cloud.h): a wave streams down a strip of 64
// columns (60 outputs, 2 halo columns either side; lane l holds column x0 - 2 + l, reflected into the frame) over a band of
// band_rows output rows; a row is one coalesced load per lane, the loads of kBilBatch rows go out together; the last five rows stay in
// registers, each with the horizontal neighbours it was given when it entered (4 DPP wave shifts per row step).  No LDS, no barrier.
// A pixel's arithmetic does not depend on the strip or the band it falls into.  src and dst must not overlap.
#pragma once
#include <hip/hip_runtime.h>

#include "dcmt_cloud.h"
#include "dcmt_gauss.h"

namespace dcmt {

constexpr int kBilBatch = 6;        // (kBilCols, kBilRows: dcmt_cloud.h)

// value held by the lane to the left / right (column c-1 / c+1); lanes without a source get 0: halo lanes, whose results are
// never stored
__device__ __forceinline__ float bil_left(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x138 /*wave_shr:1*/, 0xf, 0xf, true));
}
__device__ __forceinline__ float bil_right(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x130 /*wave_shl:1*/, 0xf, 0xf, true));
}

// a row of the ring: the lane's own column and its neighbours at -1, +1, -2, +2
struct BilRow { float c, l1, r1, l2, r2; };

__device__ __forceinline__ void bil_tap(float v, float c, float ws, float gc, float& num, float& den)
{
    const float d = __fsub_rn(v, c);
    const float w = __fmul_rn(ws, __expf(__fmul_rn(gc, __fmul_rn(d, d))));
    num = __fadd_rn(num, __fmul_rn(w, d));
    den = __fadd_rn(den, w);
}

// grid (ceil(strips * bands / 4), frames), 256 threads: one wave per (strip, band); strips = ceil(cols / kBilCols),
// bands = ceil(rows / band_rows).  INVERT: the cascade's final invert (y >= thr ? max_depth - y : y) in the store.
template <bool INVERT>
__global__ __launch_bounds__(256)
void k_bilateral5(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols, int strips, int bands, int band_rows, BilK k,
                  float max_depth, float thr)
{
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), l = threadIdx.x & 63;
    const int id = blockIdx.x * 4 + w;
    if (id >= strips * bands) return;
    const int band = id / strips, strip = id - band * strips;
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    const float* __restrict__ s = src + fo;
    const int gx = strip * kBilCols - 2 + l;
    // columns and rows beyond the frame's own reflection zone are clamped to something readable; no output depends on them
    const int cx = reflect101(min(gx, cols + 1), cols);
    const bool out_col = l >= 2 && l < 62 && gx < cols;
    const int y0 = band * band_rows, R = min(band_rows, rows - y0);
    BilRow q0 = {}, q1 = {}, q2 = {}, q3 = {}, q4 = {};
    for (int i0 = 0; i0 < R + 4; i0 += kBilBatch) {            // input row i of the band is frame row y0 + i - 2
        float v[kBilBatch];
#pragma unroll
        for (int j = 0; j < kBilBatch; ++j) {
            const int sy = reflect101(min(y0 + i0 + j - 2, rows + 1), rows);
            v[j] = s[(size_t)sy * cols + cx];
        }
#pragma unroll
        for (int j = 0; j < kBilBatch; ++j) {
            const int i = i0 + j;
            if (i < R + 4) {                                   // wave-uniform
                q0 = q1; q1 = q2; q2 = q3; q3 = q4;
                q4.c = v[j];
                q4.l1 = bil_left(v[j]); q4.r1 = bil_right(v[j]);
                q4.l2 = bil_left(q4.l1); q4.r2 = bil_right(q4.r1);
                if (i >= 4) {
                    const float c = q2.c;
                    float num = 0.0f, den = 0.0f;
                    bil_tap(q0.c, c, k.ws4, k.gc, num, den);
                    bil_tap(q1.l1, c, k.ws2, k.gc, num, den);
                    bil_tap(q1.c, c, k.ws1, k.gc, num, den);
                    bil_tap(q1.r1, c, k.ws2, k.gc, num, den);
                    bil_tap(q2.l2, c, k.ws4, k.gc, num, den);
                    bil_tap(q2.l1, c, k.ws1, k.gc, num, den);
                    den = __fadd_rn(den, 1.0f);                // the centre: d = 0, w = 1
                    bil_tap(q2.r1, c, k.ws1, k.gc, num, den);
                    bil_tap(q2.r2, c, k.ws4, k.gc, num, den);
                    bil_tap(q3.l1, c, k.ws2, k.gc, num, den);
                    bil_tap(q3.c, c, k.ws1, k.gc, num, den);
                    bil_tap(q3.r1, c, k.ws2, k.gc, num, den);
                    bil_tap(q4.c, c, k.ws4, k.gc, num, den);
                    float y = __fadd_rn(c, __fdiv_rn(num, den));
                    if (INVERT) y = y >= thr ? __fsub_rn(max_depth, y) : y;
                    if (out_col) dst[fo + (size_t)(y0 + i - 4) * cols + gx] = y;
                }
            }
        }
    }
}

}  // namespace dcmt
