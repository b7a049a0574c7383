// dcmt_kernels_bgr.h -- the camera image as the device entry points take it, batched on the device: what the reference mains do
// with every frame they read before anything else,
//     cv::cvtColor(image, lab_image, cv::COLOR_BGR2Lab)      DC_lidar_camera/main_lc.cpp:183, DC_stereo_lidar/main_sl.cpp:439
//     cv::cvtColor(..., cv::COLOR_BGR2GRAY)                  main_sl.cpp:1167, :1171
// on CV_8UC3 pixels B, G, R.  Both are integer-only per pixel, in the fixed-point scheme OpenCV uses for 8-bit images, restated
// from memory of its sources and never run against an OpenCV (OURS TO STATE):
//     grey  Y = (B * 3735 + G * 19235 + R * 9798 + 16384) >> 15
//     Lab   R' = gamma[R], G' = gamma[G], B' = gamma[B]                          (dcmt_lab_tables.h: sRGB curve, 0..2040)
//           fX = cbrt[D(R' * C00 + G' * C01 + B' * C02, 12)], fY, fZ with rows 1 and 2 of C        (index <= 2040: rows sum to 4096)
//           L = D(296 * fY - 1336934, 15),  a = D(500 * (fX - fY) + 128 * 32768, 15),  b = D(200 * (fY - fZ) + 128 * 32768, 15)
//     with D(v, n) = (v + (1 << (n - 1))) >> n.  Every intermediate fits in int32 and L, a, b lie in 0..255 for all 2^24 colours
//     (tests/test_bgr_convert.py), so nothing is clamped.
//
// One kernel, k_bgr_convert<Lab wanted, grey wanted, aligned>: the batch is ONE flat run of pixels, cut into groups of 4 (three
// dwords in; three dwords of Lab and / or one dword of grey out), kBgrGroupsPerLane groups per lane and pass, `passes` passes of
// kBgrPxPerPass consecutive pixels per workgroup.  The two tables (512 B + 6 KiB) go from constant memory into LDS once per
// workgroup; the six lookups of a pixel are 2-byte LDS reads at data-dependent addresses (equal addresses broadcast).
// A lane issues all loads of a pass before the first store of that pass, and no lane reads a pixel another lane writes: that is
// what lab == bgr (in place) rests on, and why neither pointer is __restrict__.  Where a base pointer is not dword-aligned, and in
// the run's last partial pass, byte loads and stores per pixel; the bytes written are the same.  Vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcmt_lab_tables.h"
#include "dcmt_tiles.h"        // kBgrThreads, kBgrGroupsPerLane, kBgrPxPerPass

namespace dcmt {

struct LabTables {
    uint16_t gamma[256];
    uint16_t cbrt[3072];
};
constexpr int kLabTableDwords = (int)(sizeof(LabTables) / 4);

__constant__ __attribute__((aligned(16))) LabTables kLabTablesDev = {{DCMT_LAB_GAMMA}, {DCMT_LAB_CBRT}};

// four pixels: 12 bytes that are only dword-aligned, moved as one access and indexed by group
static_assert(sizeof(uint3) == 12 && alignof(uint3) == 4, "uint3");

// p = B | G << 8 | R << 16  ->  Y
__device__ __forceinline__ uint32_t bgr_gray(uint32_t p)
{
    return ((p & 255u) * 3735u + ((p >> 8) & 255u) * 19235u + (p >> 16) * 9798u + 16384u) >> 15;
}

// p = B | G << 8 | R << 16  ->  L | a << 8 | b << 16
__device__ __forceinline__ uint32_t bgr_lab(uint32_t p, const uint16_t* gam, const uint16_t* cbr)
{
    constexpr int c[9] = {DCMT_LAB_COEF};
    const int b = gam[p & 255u], g = gam[(p >> 8) & 255u], r = gam[p >> 16];
    const int fx = cbr[(r * c[0] + g * c[1] + b * c[2] + 2048) >> 12];
    const int fy = cbr[(r * c[3] + g * c[4] + b * c[5] + 2048) >> 12];
    const int fz = cbr[(r * c[6] + g * c[7] + b * c[8] + 2048) >> 12];
    const int L = (296 * fy - 1336934 + 16384) >> 15;
    const int A = (500 * (fx - fy) + 128 * 32768 + 16384) >> 15;
    const int B = (200 * (fy - fz) + 128 * 32768 + 16384) >> 15;
    return (uint32_t)L | ((uint32_t)A << 8) | ((uint32_t)B << 16);
}

// grid ceil(total / (passes * kBgrPxPerPass)), kBgrThreads threads.  bgr, lab: [total][3] bytes; gray: [total] bytes; total < 2^31
// less a workgroup's share.  lab may be bgr.  kVec: bgr and the outputs wanted are 4-byte aligned.
template <bool kLab, bool kGray, bool kVec>
__global__ __launch_bounds__(kBgrThreads)
void k_bgr_convert(const uint8_t* bgr, uint32_t total, uint32_t passes, uint8_t* lab, uint8_t* gray)
{
    __shared__ __attribute__((aligned(16))) uint32_t tab[kLab ? kLabTableDwords : 1];
    const uint16_t* gam = reinterpret_cast<const uint16_t*>(tab);
    const uint16_t* cbr = gam + 256;
    if (kLab) {
        for (int i = threadIdx.x; i < kLabTableDwords; i += kBgrThreads) tab[i] = reinterpret_cast<const uint32_t*>(&kLabTablesDev)[i];
        __syncthreads();
    }
    for (uint32_t it = 0; it < passes; ++it) {
        const uint32_t p0 = (blockIdx.x * passes + it) * kBgrPxPerPass;
        if (p0 >= total) break;
        // workgroup-uniform: every pixel of the pass is in the run and the bases are aligned -> 12-byte loads, 12- and 4-byte stores
        const bool wide = kVec && p0 + kBgrPxPerPass <= total;
        const uint32_t gbase = p0 / 4 + threadIdx.x;

        uint32_t px[kBgrGroupsPerLane][4];                      // B | G << 8 | R << 16
        if (wide) {
#pragma unroll
            for (int j = 0; j < kBgrGroupsPerLane; ++j) {
                const uint3 t = reinterpret_cast<const uint3*>(bgr)[gbase + j * kBgrThreads];
                px[j][0] = t.x & 0xffffffu;
                px[j][1] = __builtin_amdgcn_alignbit(t.y, t.x, 24) & 0xffffffu;
                px[j][2] = __builtin_amdgcn_alignbit(t.z, t.y, 16) & 0xffffffu;
                px[j][3] = t.z >> 8;
            }
        } else {
#pragma unroll
            for (int j = 0; j < kBgrGroupsPerLane; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t q = 4 * (gbase + j * kBgrThreads) + i;
                    px[j][i] = 0;
                    if (q < total) {
                        const uint8_t* s = bgr + 3 * (size_t)q;
                        px[j][i] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
                    }
                }
        }

#pragma unroll
        for (int j = 0; j < kBgrGroupsPerLane; ++j) {
            const uint32_t g = gbase + j * kBgrThreads, q = 4 * g;
            uint32_t c[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (kLab) c[i] = bgr_lab(px[j][i], gam, cbr);
                if (kGray) y[i] = bgr_gray(px[j][i]);
            }
            if (wide) {
                if (kLab) {
                    uint3 o;
                    o.x = c[0] | (c[1] << 24);
                    o.y = (c[1] >> 8) | (c[2] << 16);
                    o.z = (c[2] >> 16) | (c[3] << 8);
                    reinterpret_cast<uint3*>(lab)[g] = o;
                }
                if (kGray) reinterpret_cast<uint32_t*>(gray)[g] = y[0] | (y[1] << 8) | (y[2] << 16) | (y[3] << 24);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (q + i < total) {
                        if (kLab) {
                            uint8_t* o = lab + 3 * (size_t)(q + i);
                            o[0] = (uint8_t)c[i]; o[1] = (uint8_t)(c[i] >> 8); o[2] = (uint8_t)(c[i] >> 16);
                        }
                        if (kGray) gray[q + i] = (uint8_t)y[i];
                    }
            }
        }
    }
}

}  // namespace dcmt
