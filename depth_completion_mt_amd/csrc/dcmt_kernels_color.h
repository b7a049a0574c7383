// dcmt_kernels_color.h -- JET colourisation of dense depth planes, batched on the device: the reference mains' toColorImage
// (DC_lidar_only/main.cpp:6-14, repeated in utils.cpp:6-13 and main_sl.cpp:42-49), called after the path at main.cpp:97,
// main_lc.cpp:246-247, main_sl.cpp:389, :545, :1257, :1259:
//     cv::normalize(r_img, n, 1.0, 0, cv::NORM_MINMAX);  n.convertTo(u8, CV_8UC1, 255.0);  cv::applyColorMap(u8, out, COLORMAP_JET);
//
// Per frame, the NORM_MINMAX arithmetic of N1 (dcmt_kernels_v1.h, k_norm_coef / norm_apply) with (lo, hi) = (1, 0):
//     smin, smax = the frame's extrema;
//     scale = (dmax - dmin) * (smax - smin > DBL_EPSILON ? 1 / (smax - smin) : 0)  in double, rounded to f32;
//     shift = (float)dmin - (float)(smin * scale)                                    (dmin = 0, dmax = 1);
//     v     = __fadd_rn(__fmul_rn(x, scale), shift)                                 (norm_apply: two roundings);
//     idx   = sat_u8(__float2int_rn(__fmul_rn(v, 255.f)))                          (convertTo's saturate_cast: round half to even);
//     bgr   = kJetBgr[idx].
// An AVX2 build of OpenCV fuses x * scale + shift into one FMA.  The two forms differ only when shift != 0, i.e. the frame
// has no zero pixel (smin != 0), and then only where v * 255 lies within an ulp of a .5, by one index at most.  The second
// convertTo (beta = 0) is a single rounding of v * 255 in either form.
//
// The palette is cv::COLORMAP_JET as OpenCV's applyColorMap applies it to CV_8UC1 -- the recorded table of
// tests/golden/jet_lut.json (its ramp values are .5 ties of the closed form that OpenCV's float arithmetic decides one by one,
// so no formula gives it).
//
// Two kernels per segment of frames, no float atomics, no state carried from call to call:
//   k_color_minmax  one workgroup per (chunk, frame), the chunking of dcmt_kernels_eval.h (eval_chunks): the chunk's min and max
//                   to a slab entry.  min / max are exact, so the extrema do not depend on the order they are combined in;
//   k_color_map     the segment as ONE flat pixel run, cut into groups of 4 pixels, kColorGroupsPerLane groups per lane.  A
//                   workgroup first reduces the slab entries of the frames its pixels belong to (one wave per frame, chunks in a
//                   fixed order) into per-frame (scale, shift) in LDS and copies the palette to LDS (measured against
//                   reading it from constant memory with the pixel's index: 0.85 against 0.87 ms per 1024 frames of 352 x 1216,
//                   and further apart with more launches); every pixel finds its own
//                   frame, so a group may straddle two frames (375 x 1242 frames are not a multiple of 4 pixels).  Loads: one
//                   16-byte load per group; stores: one 12-byte store per group (4 BGR pixels), vector stores only.  Where the
//                   run's base pointers do not allow that (source not 16-byte or output not 4-byte aligned), per-pixel loads
//                   and byte stores; the bytes written are the same.
// Bytes per pixel: 4 (min/max read) + 4 (re-read) + 3 (write) = 11; 7 when the re-read hits the Infinity Cache.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "dcmt_kernels_eval.h"
#include "dcmt_tiles.h"        // kColorThreads, kColorGroupsPerLane, kColorPxPerWg, kColorSlabStride

namespace dcmt {

// cv::COLORMAP_JET, index order, packed b | g << 8 | r << 16 (tests/golden/jet_lut.json, which stores [B, G, R] triples)
#define DCMT_JET_BGR_PACKED \
    0x000080, 0x000084, 0x000088, 0x00008c, 0x000090, 0x000094, 0x000098, 0x00009c, \
    0x0000a0, 0x0000a4, 0x0000a8, 0x0000ac, 0x0000b0, 0x0000b4, 0x0000b8, 0x0000bc, \
    0x0000c0, 0x0000c4, 0x0000c8, 0x0000cc, 0x0000d0, 0x0000d4, 0x0000d8, 0x0000dc, \
    0x0000e0, 0x0000e4, 0x0000e8, 0x0000ec, 0x0000f0, 0x0000f4, 0x0000f8, 0x0000fc, \
    0x0000ff, 0x0004ff, 0x0008ff, 0x000cff, 0x0010ff, 0x0014ff, 0x0018ff, 0x001cff, \
    0x0020ff, 0x0024ff, 0x0028ff, 0x002cff, 0x0030ff, 0x0034ff, 0x0038ff, 0x003cff, \
    0x0040ff, 0x0044ff, 0x0048ff, 0x004cff, 0x0050ff, 0x0054ff, 0x0058ff, 0x005cff, \
    0x0060ff, 0x0064ff, 0x0068ff, 0x006cff, 0x0070ff, 0x0074ff, 0x0078ff, 0x007cff, \
    0x0080ff, 0x0084ff, 0x0088ff, 0x008cff, 0x0090ff, 0x0094ff, 0x0098ff, 0x009cff, \
    0x00a0ff, 0x00a4ff, 0x00a8ff, 0x00acff, 0x00b0ff, 0x00b4ff, 0x00b8ff, 0x00bcff, \
    0x00c0ff, 0x00c4ff, 0x00c8ff, 0x00ccff, 0x00d0ff, 0x00d4ff, 0x00d8ff, 0x00dcff, \
    0x00e0ff, 0x00e4ff, 0x00e8ff, 0x00ecff, 0x00f0ff, 0x00f4ff, 0x00f8ff, 0x00fcff, \
    0x02fffe, 0x06fffa, 0x0afff6, 0x0efff2, 0x12ffee, 0x16ffea, 0x1affe6, 0x1effe2, \
    0x22ffde, 0x26ffda, 0x2affd6, 0x2effd2, 0x32ffce, 0x36ffca, 0x3affc6, 0x3effc2, \
    0x42ffbe, 0x46ffba, 0x4affb6, 0x4effb2, 0x52ffae, 0x56ffaa, 0x5affa6, 0x5effa2, \
    0x62ff9e, 0x66ff9a, 0x6aff96, 0x6eff92, 0x72ff8e, 0x76ff8a, 0x7aff86, 0x7eff82, \
    0x82ff7e, 0x86ff7a, 0x8aff76, 0x8eff72, 0x92ff6e, 0x96ff6a, 0x9aff66, 0x9eff62, \
    0xa2ff5e, 0xa6ff5a, 0xaaff56, 0xaeff52, 0xb2ff4e, 0xb6ff4a, 0xbaff46, 0xbeff42, \
    0xc2ff3e, 0xc6ff3a, 0xcaff36, 0xceff32, 0xd2ff2e, 0xd6ff2a, 0xdaff26, 0xdeff22, \
    0xe2ff1e, 0xe6ff1a, 0xeaff16, 0xeeff12, 0xf2ff0e, 0xf6ff0a, 0xfaff06, 0xfeff01, \
    0xfffc00, 0xfff800, 0xfff400, 0xfff000, 0xffec00, 0xffe800, 0xffe400, 0xffe000, \
    0xffdc00, 0xffd800, 0xffd400, 0xffd000, 0xffcc00, 0xffc800, 0xffc400, 0xffc000, \
    0xffbc00, 0xffb800, 0xffb400, 0xffb000, 0xffac00, 0xffa800, 0xffa400, 0xffa000, \
    0xff9c00, 0xff9800, 0xff9400, 0xff9000, 0xff8c00, 0xff8800, 0xff8400, 0xff8000, \
    0xff7c00, 0xff7800, 0xff7400, 0xff7000, 0xff6c00, 0xff6800, 0xff6400, 0xff6000, \
    0xff5c00, 0xff5800, 0xff5400, 0xff5000, 0xff4c00, 0xff4800, 0xff4400, 0xff4000, \
    0xff3c00, 0xff3800, 0xff3400, 0xff3000, 0xff2c00, 0xff2800, 0xff2400, 0xff2000, \
    0xff1c00, 0xff1800, 0xff1400, 0xff1000, 0xff0c00, 0xff0800, 0xff0400, 0xff0000, \
    0xfc0000, 0xf80000, 0xf40000, 0xf00000, 0xec0000, 0xe80000, 0xe40000, 0xe00000, \
    0xdc0000, 0xd80000, 0xd40000, 0xd00000, 0xcc0000, 0xc80000, 0xc40000, 0xc00000, \
    0xbc0000, 0xb80000, 0xb40000, 0xb00000, 0xac0000, 0xa80000, 0xa40000, 0xa00000, \
    0x9c0000, 0x980000, 0x940000, 0x900000, 0x8c0000, 0x880000, 0x840000, 0x800000

__constant__ uint32_t kJetBgrDev[256] = {DCMT_JET_BGR_PACKED};

// grid (eval_chunks(n), frames), 256 threads.  slab: [frames][chunks][2] floats (min, max)
__global__ __launch_bounds__(kColorThreads)
void k_color_minmax(const float* __restrict__ src, uint32_t n, float* __restrict__ slab)
{
    const uint32_t c = blockIdx.x, chunks = gridDim.x;
    const float* __restrict__ p = src + (size_t)blockIdx.y * n;
    const uint32_t full = n / 4, G = eval_chunk_groups(n);
    const uint32_t g0 = c * G, g1 = min(g0 + G, (n + 3) / 4), gf = min(g1, full);
    float lo0 = FLT_MAX, hi0 = -FLT_MAX, lo1 = FLT_MAX, hi1 = -FLT_MAX;
    uint32_t k = g0 + threadIdx.x;
    // a frame starts at any dword: 16-byte loads that are only dword-aligned, as k_eval_partial reads them
    for (; k + kColorThreads < gf; k += 2 * kColorThreads) {
        float4 a, b;
        __builtin_memcpy(&a, p + 4 * (size_t)k, sizeof a);
        __builtin_memcpy(&b, p + 4 * (size_t)(k + kColorThreads), sizeof b);
        lo0 = fminf(lo0, fminf(fminf(a.x, a.y), fminf(a.z, a.w))); hi0 = fmaxf(hi0, fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)));
        lo1 = fminf(lo1, fminf(fminf(b.x, b.y), fminf(b.z, b.w))); hi1 = fmaxf(hi1, fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w)));
    }
    if (k < gf) {
        float4 a;
        __builtin_memcpy(&a, p + 4 * (size_t)k, sizeof a);
        lo0 = fminf(lo0, fminf(fminf(a.x, a.y), fminf(a.z, a.w))); hi0 = fmaxf(hi0, fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)));
        k += kColorThreads;
    }
    if (k == full && full < g1)                          // the partial last group (n % 4 pixels)
        for (uint32_t i = 4 * full; i < n; ++i) { lo0 = fminf(lo0, p[i]); hi0 = fmaxf(hi0, p[i]); }
    float lo = fminf(lo0, lo1), hi = fmaxf(hi0, hi1);
    for (int m = 32; m >= 1; m >>= 1) { lo = fminf(lo, __shfl_xor(lo, m, 64)); hi = fmaxf(hi, __shfl_xor(hi, m, 64)); }
    __shared__ float red[kColorThreads / 64][2];
    const int w = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) { red[w][0] = lo; red[w][1] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < kColorThreads / 64; ++j) { lo = fminf(lo, red[j][0]); hi = fmaxf(hi, red[j][1]); }
        float2 e;
        e.x = lo; e.y = hi;
        reinterpret_cast<float2*>(slab)[(size_t)blockIdx.y * chunks + c] = e;
    }
}

// (scale, shift) of cv::normalize(src, dst, 1.0, 0, NORM_MINMAX) into CV_32F, exactly as k_norm_coef computes them
__device__ __forceinline__ float2 color_coef(float fmin_, float fmax_)
{
    const double smin = (double)fmin_, smax = (double)fmax_, dmin = 0.0, dmax = 1.0;
    const double d = smax - smin;
    double scale = (dmax - dmin) * (d > 2.220446049250313e-16 ? __ddiv_rn(1.0, d) : 0.0);
    scale = (double)(float)scale;
    const double shift = (double)(float)dmin - (double)(float)__dmul_rn(smin, scale);
    float2 r;
    r.x = (float)scale; r.y = (float)shift;
    return r;
}

__device__ __forceinline__ uint32_t color_index(float x, float2 k)
{
    const float v = __fadd_rn(__fmul_rn(x, k.x), k.y);
    const int i = __float2int_rn(__fmul_rn(v, 255.0f));
    return (uint32_t)min(max(i, 0), 255);
}

// grid ceil(total / kColorPxPerWg), 256 threads, dynamic LDS 4 * 256 + 8 * (frames a workgroup can touch).
// src: the segment's frames [frames][n] as one run of total = frames * n pixels; bgr: [frames][n][3].
// kVec: src 16-byte and bgr 4-byte aligned.
template <bool kVec>
__global__ __launch_bounds__(kColorThreads)
void k_color_map(const float* __restrict__ src, uint32_t n, uint32_t total, const float* __restrict__ slab, uint32_t chunks,
                 uint8_t* __restrict__ bgr)
{
    extern __shared__ uint32_t color_lds[];
    uint32_t* lut = color_lds;                                        // [256] packed BGR
    float2* coef = reinterpret_cast<float2*>(color_lds + 256);       // [frames of this workgroup]
    const uint32_t p0 = blockIdx.x * kColorPxPerWg;
    const uint32_t pend = min(p0 + kColorPxPerWg, total);
    const uint32_t fa = p0 / n, span = (pend - 1) / n - fa + 1;
    const uint32_t gbase = blockIdx.x * (kColorPxPerWg / 4) + threadIdx.x;
    // workgroup-uniform: every pixel of the workgroup is in the run and the bases are aligned -> 16-byte loads, 12-byte stores
    const bool wide = kVec && p0 + kColorPxPerWg <= total;

    // the pixel loads go out first; the palette and the frames' coefficients arrive while they are in flight
    float x[kColorGroupsPerLane][4];
    if (wide) {
#pragma unroll
        for (int j = 0; j < kColorGroupsPerLane; ++j) {
            const float4 t = reinterpret_cast<const float4*>(src)[gbase + j * kColorThreads];
            x[j][0] = t.x; x[j][1] = t.y; x[j][2] = t.z; x[j][3] = t.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kColorGroupsPerLane; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t q = 4 * (gbase + j * kColorThreads) + i;
                x[j][i] = q < total ? src[q] : 0.0f;
            }
    }
    lut[threadIdx.x] = kJetBgrDev[threadIdx.x];
    const int w = threadIdx.x / 64, l = threadIdx.x & 63;
    for (uint32_t k = w; k < span; k += kColorThreads / 64) {
        const float2* s = reinterpret_cast<const float2*>(slab) + (size_t)(fa + k) * chunks;
        float lo = FLT_MAX, hi = -FLT_MAX;
        for (uint32_t c = l; c < chunks; c += 64) { const float2 e = s[c]; lo = fminf(lo, e.x); hi = fmaxf(hi, e.y); }
        for (int m = 32; m >= 1; m >>= 1) { lo = fminf(lo, __shfl_xor(lo, m, 64)); hi = fmaxf(hi, __shfl_xor(hi, m, 64)); }
        if (l == 0) coef[k] = color_coef(lo, hi);
    }
    __syncthreads();

#pragma unroll
    for (int j = 0; j < kColorGroupsPerLane; ++j) {
        const uint32_t g = gbase + j * kColorThreads, q = 4 * g;
        // each pixel's own frame: q / n once, then step over frame ends (a group crosses more than one when n < 4)
        uint32_t f = q / n, r = q - f * n;
        uint32_t c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i > 0 && ++r == n) { r = 0; ++f; }
            c[i] = lut[color_index(x[j][i], coef[min(f - fa, span - 1)])];
        }
        if (wide) {
            uint3 o;
            o.x = c[0] | (c[1] << 24);
            o.y = (c[1] >> 8) | (c[2] << 16);
            o.z = (c[2] >> 16) | (c[3] << 8);
            reinterpret_cast<uint3*>(bgr)[g] = o;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (q + i < total) {
                    uint8_t* o = bgr + 3 * (size_t)(q + i);
                    o[0] = (uint8_t)c[i]; o[1] = (uint8_t)(c[i] >> 8); o[2] = (uint8_t)(c[i] >> 16);
                }
        }
    }
}

}  // namespace dcmt
