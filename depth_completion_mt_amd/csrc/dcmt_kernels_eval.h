// dcmt_kernels_eval.h -- accuracy metrics of a dense depth plane against ground truth, batched on the device: the
// evaluate_performance(s) functions every reference main runs after the path (DC_lidar_only/main.cpp:16-34,
// DC_lidar_camera/main_lc.cpp:85-116, DC_stereo_lidar/main_sl.cpp:1031-1061), plus the inverse-depth terms
// main_lc.cpp:96 names.  Per frame it produces the 7 sums of dcmt_eval_frame (include/dcmt.h); the final divisions are
// the caller's.
//
// The mask does not depend on position, so a frame is a flat run of n = rows * cols pixels, cut into groups of 4
// consecutive pixels (the last one partial when n % 4 != 0) and into eval_chunks(n) chunks of eval_chunk_groups(n)
// groups.  One workgroup per (chunk, frame):
//   k_eval_partial  lane t of chunk c takes groups c * G + t, c * G + t + 256, ... in that order and pixels 0..3 of each
//                   group in order; counts as integers, sums in f64.  The lane sums meet in a fixed butterfly inside the
//                   wave and in wave order across the workgroup; one slab entry per (chunk, frame);
//   k_eval_combine  one wave per frame: lane l adds chunks l, l + 64, ... in order, the same butterfly, one dcmt_eval_frame.
// Which lane adds which pixel in which order is a function of n alone -- not of the frame's position, its alignment or the
// batch -- so a frame's sums are the same bits at every position in every batch (no float atomics anywhere).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "dcmt_chunks.h"

namespace dcmt {

constexpr int kEvalSlabStride = 8;                  // doubles per slab entry (7 used): 64-byte entries

struct EvalAcc {
    int n = 0, n_inv = 0;
    double err = 0.0, abs = 0.0, sq = 0.0, inv_abs = 0.0, inv_sq = 0.0;
};

// one pixel, the reference's statements: e = gt - pred, d = fabs(e), d * d in f32 (LO main.cpp:27, LC main_lc.cpp:106-108);
// the inverse terms in f64 (main_lc.cpp:96) only where pred > 0
__device__ __forceinline__ void eval_px(EvalAcc& a, float gt, float pr, float thresh, bool both)
{
    const bool m = gt > thresh && (!both || pr > thresh);
    if (m) {
        const float e = __fsub_rn(gt, pr);
        const float d = fabsf(e);
        const float s = __fmul_rn(d, d);
        a.n += 1;
        a.err = __dadd_rn(a.err, (double)e);
        a.abs = __dadd_rn(a.abs, (double)d);
        a.sq = __dadd_rn(a.sq, (double)s);
        if (pr > 0.0f) {
            const double di = fabs(__dsub_rn(__ddiv_rn(1.0, (double)gt), __ddiv_rn(1.0, (double)pr)));
            a.n_inv += 1;
            a.inv_abs = __dadd_rn(a.inv_abs, di);
            a.inv_sq = __dadd_rn(a.inv_sq, __dmul_rn(di, di));
        }
    }
}

// The 4 pixels of a full group, one 16-byte load (8 bytes for uint16 GT).  A frame starts wherever batch x rows x cols puts it
// (375 x 1242 frames alternate between 16- and 8-byte aligned starts), so these loads are only dword- (uint16: word-) aligned in
// general; gfx950's global loads run in the HSA runtime's unaligned mode and take them as they are (hipcc emits the same
// global_load_dwordx4 / _dwordx2 for every alignment), so there is no scalar head or tail per frame and no per-alignment
// variant of the loop.
__device__ __forceinline__ void eval_load4(const float* __restrict__ p, float, float v[4])
{
    float4 t;
    __builtin_memcpy(&t, p, sizeof t);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
// the KITTI uint16 payload: metres = __fmul_rn((float)v, scale), as dcmt_complete_u16_dev converts
__device__ __forceinline__ void eval_load4(const uint16_t* __restrict__ p, float scale, float v[4])
{
    uint2 t;
    __builtin_memcpy(&t, p, sizeof t);
    v[0] = __fmul_rn((float)(t.x & 0xffffu), scale); v[1] = __fmul_rn((float)(t.x >> 16), scale);
    v[2] = __fmul_rn((float)(t.y & 0xffffu), scale); v[3] = __fmul_rn((float)(t.y >> 16), scale);
}
__device__ __forceinline__ float eval_load1(const float* __restrict__ p, float) { return *p; }
__device__ __forceinline__ float eval_load1(const uint16_t* __restrict__ p, float scale) { return __fmul_rn((float)*p, scale); }

// fixed butterfly over the 64 lanes of a wave; every lane ends with the same value (a + b == b + a in IEEE arithmetic)
__device__ __forceinline__ void eval_wave_sum(EvalAcc& a)
{
    for (int m = 32; m >= 1; m >>= 1) {
        a.n += __shfl_xor(a.n, m, 64);
        a.n_inv += __shfl_xor(a.n_inv, m, 64);
        a.err = __dadd_rn(a.err, __shfl_xor(a.err, m, 64));
        a.abs = __dadd_rn(a.abs, __shfl_xor(a.abs, m, 64));
        a.sq = __dadd_rn(a.sq, __shfl_xor(a.sq, m, 64));
        a.inv_abs = __dadd_rn(a.inv_abs, __shfl_xor(a.inv_abs, m, 64));
        a.inv_sq = __dadd_rn(a.inv_sq, __shfl_xor(a.inv_sq, m, 64));
    }
}

// grid (eval_chunks(n), batch), 256 threads.  slab: [batch][chunks][kEvalSlabStride] doubles.
template <typename TG>
__global__ __launch_bounds__(kEvalThreads)
void k_eval_partial(const TG* __restrict__ gt, float gt_scale, const float* __restrict__ pred, uint32_t n, float thresh, int both,
                    double* __restrict__ slab)
{
    const uint32_t c = blockIdx.x, chunks = gridDim.x;
    const size_t base = (size_t)blockIdx.y * n;
    const TG* __restrict__ g = gt + base;
    const float* __restrict__ p = pred + base;
    const uint32_t full = n / 4, G = eval_chunk_groups(n);
    const uint32_t g0 = c * G, g1 = min(g0 + G, (n + 3) / 4), gf = min(g1, full);
    const bool bth = both != 0;
    EvalAcc a;
    uint32_t k = g0 + threadIdx.x;
    // the full groups k, k + 256, ... below gf, in that order, two in flight per lane
    for (; k + kEvalThreads < gf; k += 2 * kEvalThreads) {
        float vg0[4], vp0[4], vg1[4], vp1[4];
        eval_load4(g + 4 * (size_t)k, gt_scale, vg0);
        eval_load4(p + 4 * (size_t)k, 0.0f, vp0);
        eval_load4(g + 4 * (size_t)(k + kEvalThreads), gt_scale, vg1);
        eval_load4(p + 4 * (size_t)(k + kEvalThreads), 0.0f, vp1);
        for (int i = 0; i < 4; ++i) eval_px(a, vg0[i], vp0[i], thresh, bth);
        for (int i = 0; i < 4; ++i) eval_px(a, vg1[i], vp1[i], thresh, bth);
    }
    if (k < gf) {
        float vg[4], vp[4];
        eval_load4(g + 4 * (size_t)k, gt_scale, vg);
        eval_load4(p + 4 * (size_t)k, 0.0f, vp);
        for (int i = 0; i < 4; ++i) eval_px(a, vg[i], vp[i], thresh, bth);
        k += kEvalThreads;
    }
    if (k == full && full < g1)                          // the partial last group (n % 4 pixels): its owner, after its full ones
        for (uint32_t i = 4 * full; i < n; ++i) eval_px(a, eval_load1(g + i, gt_scale), p[i], thresh, bth);
    eval_wave_sum(a);
    __shared__ double red[kEvalThreads / 64][7];
    const int w = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) {
        red[w][0] = (double)a.n; red[w][1] = a.err; red[w][2] = a.abs; red[w][3] = a.sq;
        red[w][4] = (double)a.n_inv; red[w][5] = a.inv_abs; red[w][6] = a.inv_sq;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        double s = red[0][threadIdx.x];
        for (int j = 1; j < kEvalThreads / 64; ++j) s = __dadd_rn(s, red[j][threadIdx.x]);
        slab[((size_t)blockIdx.y * chunks + c) * kEvalSlabStride + threadIdx.x] = s;
    }
}

// grid (batch), 64 threads: the chunks of a frame in a fixed order -> out[frame] (7 doubles, dcmt_eval_frame)
__global__ __launch_bounds__(64)
void k_eval_combine(const double* __restrict__ slab, uint32_t chunks, double* __restrict__ out)
{
    const double* s = slab + (size_t)blockIdx.x * chunks * kEvalSlabStride;
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t c = threadIdx.x; c < chunks; c += 64)
        for (int j = 0; j < 7; ++j) v[j] = __dadd_rn(v[j], s[(size_t)c * kEvalSlabStride + j]);
    for (int m = 32; m >= 1; m >>= 1)
        for (int j = 0; j < 7; ++j) v[j] = __dadd_rn(v[j], __shfl_xor(v[j], m, 64));
    if (threadIdx.x < 7) {
        double r = v[0];
        for (int j = 1; j < 7; ++j) if ((int)threadIdx.x == j) r = v[j];
        out[(size_t)blockIdx.x * 7 + threadIdx.x] = r;
    }
}

}  // namespace dcmt
