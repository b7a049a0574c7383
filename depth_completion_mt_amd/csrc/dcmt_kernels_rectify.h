// dcmt_kernels_rectify.h -- k_rectify_map and k_rectify: the undistort-and-rectify map of a calibration record and the bilinear
// remap of a batch of 8-bit frames through such maps, as include/dcmt.h states them to the last bit (tests/rectify_restatement.py
// restates them in numpy).  Compiled in dcmt_rectify.hip, a code object of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dcmt.h"
#include "dcmt_calib.h"        // bits_finite64, bits_nonzero64
#include "dcmt_rectify.h"

namespace dcmt {

static_assert(sizeof(dcmt_rectify_calib) == 176 && offsetof(dcmt_rectify_calib, k1) == 32 && offsetof(dcmt_rectify_calib, R) == 72 &&
              offsetof(dcmt_rectify_calib, fxp) == 144, "dcmt_rectify_calib layout");
constexpr uint32_t kRectifyRecWords = sizeof(dcmt_rectify_calib) / 8;       // 22 doubles

// mx * 32 or my * 32 -> the fixed-point coordinate; false where it is outside: NaN, +-Inf or magnitude >= 2^30, on the bits.  The
// value goes through an empty asm first: the library is built with -ffinite-math-only, and what the compiler may assume of a product
// it must not assume of these bits.
__device__ __forceinline__ bool rectify_fixed(double t, int32_t& s)
{
    asm volatile("" : "+v"(t));
    const uint64_t b = (uint64_t)__double_as_longlong(t);
    const bool inside = (uint32_t)((b >> 52) & 0x7ffu) < 1023u + 30u;
    s = inside ? (int32_t)rint(t) : 0;
    return inside;
}

// One map element per lane, in f64, every operation in the order of dcmt.h (the build has -ffp-contract=off).  grid (ceil(rows * cols
// / 256), n_maps).  The record's index is the block's, so its 22 words come through the scalar cache and are tested once per wave.
__global__ __launch_bounds__(kRectifyThreads) void k_rectify_map(const dcmt_rectify_calib* __restrict__ table, uint32_t rows, uint32_t cols,
                                                                int32_t* __restrict__ map)
{
    const uint32_t m = blockIdx.y, n = rows * cols;
    const uint64_t* __restrict__ q = reinterpret_cast<const uint64_t*>(table) + kRectifyRecWords * (size_t)m;
    double k[kRectifyRecWords];
    bool ok = true;
#pragma unroll
    for (uint32_t i = 0; i < kRectifyRecWords; ++i) {
        const uint64_t b = q[i];
        ok = ok && bits_finite64(b);
        k[i] = __longlong_as_double((long long)b);
    }
    ok = ok && bits_nonzero64(q[18]) && bits_nonzero64(q[19]);
    const uint32_t idx = blockIdx.x * kRectifyThreads + threadIdx.x;
    if (idx >= n) return;
    int2 e = make_int2(INT32_MIN, INT32_MIN);
    if (ok) {
        const double fx = k[0], fy = k[1], cx = k[2], cy = k[3], k1 = k[4], k2 = k[5], p1 = k[6], p2 = k[7], k3 = k[8];
        const double* R = k + 9;
        const double fxp = k[18], fyp = k[19], cxp = k[20], cyp = k[21];
        const double u = (double)(idx % cols), v = (double)(idx / cols);
        const double x = (u - cxp) / fxp, y = (v - cyp) / fyp;
        const double X = (R[0] * x + R[3] * y) + R[6], Y = (R[1] * x + R[4] * y) + R[7], W = (R[2] * x + R[5] * y) + R[8];
        const double xn = X / W, yn = Y / W, x2 = xn * xn, y2 = yn * yn, r2 = x2 + y2, xy2 = (2.0 * xn) * yn;
        const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
        const double xd = (xn * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2);
        const double yd = (yn * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2;
        const double mx = fx * xd + cx, my = fy * yd + cy;
        int32_t sx, sy;
        const bool in_x = rectify_fixed(mx * 32.0, sx), in_y = rectify_fixed(my * 32.0, sy);
        if (in_x && in_y) e = make_int2(sx, sy);
    }
    reinterpret_cast<int2*>(map)[(size_t)m * n + idx] = e;
}

// ---- k_rectify --------------------------------------------------------------------------------------------------------------
// A workgroup owns one destination tile (kRectifyTileW x kRectifyTileH) of one map and the frames that use it; a lane
// kRectifyPxPerLane consecutive pixels of one tile row.  It reads its map elements ONCE, turns them into what the frame loop needs
// -- the four weights of a pixel (zero for a sample outside the source, which is all the border handling there is) and its sample
// positions clamped into the tile's source bounding box -- and reduces that box over the workgroup.  Then, per frame:
//   lds route     the box's rows are staged in LDS as the naturally aligned 16-byte quads that hold them (a quad that would reach
//                 outside the source batch, possible at its two ends only, is loaded byte by byte, range-checked), the taps are byte
//                 reads of LDS;
//   gather route  (the box does not fit kRectifyLdsBytes, or the call forces it) the taps are byte loads from global memory.
// Every address is formed from clamped positions: inside the box, which lies inside the source.  The lane stores its pixels with
// dword stores where its address allows (one for grey, three for BGR), byte stores otherwise.
// grid (tiles, groups, chunks).  Without an index table a group is a map m and its frames m, m + n_maps, ...; chunk z takes
// per_chunk of them.  With one a group is a frame f (chunks = 1) and its map is index[f]; a bad index zeroes the frame's tile.

struct RectifyPx {
    uint32_t oa, ob;            // byte offset of the sample rows iy, iy + 1: in the staged box (lds) or in the frame (gather), the box's origin included
    uint32_t xa, xb;            // byte offset of the sample columns ix, ix + 1 behind that
    uint32_t sh;                // lds: (row * source row bytes) & 15 of the two rows, 4 bits each
    uint32_t w;                 // 32 - ax, ax, 32 - ay, ay, a byte each; zero for a sample outside the source
};

__device__ __forceinline__ int32_t rectify_clamp(int32_t v, int32_t lo, int32_t hi) { return min(max(v, lo), hi); }

template <int CH, typename Tap>
__device__ __forceinline__ void rectify_blend(const RectifyPx& p, uint32_t sha, uint32_t shb, Tap tap, uint32_t out[CH])
{
    const uint32_t wx0 = p.w & 0xffu, wx1 = (p.w >> 8) & 0xffu, wy0 = (p.w >> 16) & 0xffu, wy1 = p.w >> 24;
    const uint32_t aa = p.oa + sha + p.xa, ab = p.oa + sha + p.xb, ba = p.ob + shb + p.xa, bb = p.ob + shb + p.xb;
#pragma unroll
    for (int c = 0; c < CH; ++c)
        out[c] = (wy0 * (wx0 * tap(aa + c) + wx1 * tap(ab + c)) + wy1 * (wx0 * tap(ba + c) + wx1 * tap(bb + c)) + 512u) >> 10;
}

// the lane's kRectifyPxPerLane pixels, v[pixel][channel], to d (the address of its first): n_px of them are inside the frame
template <int CH>
__device__ __forceinline__ void rectify_store(uint8_t* __restrict__ d, const uint32_t v[kRectifyPxPerLane][CH], uint32_t n_px)
{
    if (n_px == kRectifyPxPerLane && ((uintptr_t)d & 3u) == 0) {
        uint32_t* __restrict__ d4 = reinterpret_cast<uint32_t*>(d);
        if constexpr (CH == 1) {
            d4[0] = v[0][0] | (v[1][0] << 8) | (v[2][0] << 16) | (v[3][0] << 24);
        } else {
            d4[0] = v[0][0] | (v[0][1] << 8) | (v[0][2] << 16) | (v[1][0] << 24);
            d4[1] = v[1][1] | (v[1][2] << 8) | (v[2][0] << 16) | (v[2][1] << 24);
            d4[2] = v[2][2] | (v[3][0] << 8) | (v[3][1] << 16) | (v[3][2] << 24);
        }
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < kRectifyPxPerLane; ++k)
        if (k < n_px) {
#pragma unroll
            for (int c = 0; c < CH; ++c) d[k * CH + c] = (uint8_t)v[k][c];
        }
}

template <int CH>
__global__ __launch_bounds__(kRectifyThreads) void k_rectify(const uint8_t* __restrict__ src, uint32_t src_rows, uint32_t src_cols,
                                                            const int32_t* __restrict__ map, uint32_t n_maps,
                                                            const int32_t* __restrict__ index, uint8_t* __restrict__ dst, uint32_t rows,
                                                            uint32_t cols, uint32_t batch, uint32_t tiles_x, uint32_t per_chunk,
                                                            uint32_t force_gather, uint32_t* route, uint32_t call_id)
{
    __shared__ uint4 lds[kRectifyLdsBytes / 16];
    __shared__ int32_t red[kRectifyThreads / 64][4];
    const uint32_t t = threadIdx.x;
    const uint32_t py = (blockIdx.x / tiles_x) * kRectifyTileH + t / (kRectifyTileW / kRectifyPxPerLane);
    const uint32_t px = (blockIdx.x % tiles_x) * kRectifyTileW + kRectifyPxPerLane * (t % (kRectifyTileW / kRectifyPxPerLane));
    const uint32_t n_px = py < rows && px < cols ? min(cols - px, kRectifyPxPerLane) : 0u;
    const size_t frame_px = (size_t)rows * cols;

    // the group's frames: first, first + step, ... (count of them)
    uint32_t m, first, step, count;
    if (index) {
        first = blockIdx.y; step = 0; count = 1;
        const int32_t mi = index[first];
        if (mi < 0 || (uint32_t)mi >= n_maps) {                             // a bad index: the frame is all zero (uniform over the workgroup)
            if (n_px) {
                uint32_t zero[kRectifyPxPerLane][CH] = {};
                rectify_store<CH>(dst + ((size_t)first * frame_px + (size_t)py * cols + px) * CH, zero, n_px);
            }
            return;
        }
        m = (uint32_t)mi;
    } else {
        m = blockIdx.y;                                                     // < min(n_maps, batch)
        const uint32_t total = (batch - m + n_maps - 1) / n_maps, j0 = blockIdx.z * per_chunk;
        if (j0 >= total) return;
        first = m + j0 * n_maps; step = n_maps; count = min(per_chunk, total - j0);
    }

    // the lane's map elements
    int32_t ix[kRectifyPxPerLane], iy[kRectifyPxPerLane];
    uint32_t wts[kRectifyPxPerLane];
    int32_t lo_x = INT32_MAX, hi_x = INT32_MIN, lo_y = INT32_MAX, hi_y = INT32_MIN;
    const int32_t sc = (int32_t)src_cols, sr = (int32_t)src_rows;           // <= kRectifyMaxSrcSide
    const int2* __restrict__ mp = reinterpret_cast<const int2*>(map) + (size_t)m * frame_px + (size_t)py * cols + px;
#pragma unroll
    for (uint32_t k = 0; k < kRectifyPxPerLane; ++k) {
        ix[k] = iy[k] = 0; wts[k] = 0;
        if (k < n_px) {
            const int2 e = mp[k];
            const int32_t x = e.x >> 5, y = e.y >> 5;                       // in [-2^26, 2^26): x + 1 and y + 1 cannot wrap
            const uint32_t ax = (uint32_t)e.x & 31u, ay = (uint32_t)e.y & 31u;
            if (x >= -1 && x < sc && y >= -1 && y < sr) {                   // at least one of the four samples is inside the source
                const uint32_t wx0 = x >= 0 ? 32u - ax : 0u, wx1 = x + 1 < sc ? ax : 0u;
                const uint32_t wy0 = y >= 0 ? 32u - ay : 0u, wy1 = y + 1 < sr ? ay : 0u;
                wts[k] = wx0 | (wx1 << 8) | (wy0 << 16) | (wy1 << 24);
                ix[k] = x; iy[k] = y;
                lo_x = min(lo_x, x); hi_x = max(hi_x, x); lo_y = min(lo_y, y); hi_y = max(hi_y, y);
            }
        }
    }
    // the tile's bounding box: over the wave, then over the workgroup's waves
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo_x = min(lo_x, __shfl_xor(lo_x, d)); hi_x = max(hi_x, __shfl_xor(hi_x, d));
        lo_y = min(lo_y, __shfl_xor(lo_y, d)); hi_y = max(hi_y, __shfl_xor(hi_y, d));
    }
    if ((t & 63u) == 0) { red[t >> 6][0] = lo_x; red[t >> 6][1] = hi_x; red[t >> 6][2] = lo_y; red[t >> 6][3] = hi_y; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kRectifyThreads / 64; ++w) {
        lo_x = min(lo_x, red[w][0]); hi_x = max(hi_x, red[w][1]); lo_y = min(lo_y, red[w][2]); hi_y = max(hi_y, red[w][3]);
    }
    const bool empty = lo_x > hi_x;                                         // no sample of the tile inside the source: zeros, nothing is staged
    const int32_t x0 = empty ? 0 : max(lo_x, 0), x1 = empty ? 0 : min(hi_x + 1, sc - 1);
    const int32_t y0 = empty ? 0 : max(lo_y, 0), y1 = empty ? 0 : min(hi_y + 1, sr - 1);
    const uint32_t bw = (uint32_t)(x1 - x0) + 1u, bh = (uint32_t)(y1 - y0) + 1u;
    const bool use_lds = !force_gather && rectify_box_fits(bw, bh, CH);
    if (t == 0) {
        const uint32_t r = use_lds ? kRectifyRouteLds : kRectifyRouteGather;
        if (route[r] != call_id) route[r] = call_id;
    }
    const uint32_t pitch = rectify_pitch(bw, CH), quads = pitch / 16u;
    const uint32_t rb = src_cols * CH;                                      // source row bytes
    const size_t src_frame = (size_t)src_rows * rb;
    const size_t box0 = ((size_t)y0 * src_cols + (size_t)x0) * CH;          // the box's first byte in a frame

    RectifyPx p[kRectifyPxPerLane];
#pragma unroll
    for (uint32_t k = 0; k < kRectifyPxPerLane; ++k) {
        const uint32_t ca = (uint32_t)(rectify_clamp(ix[k], x0, x1) - x0), cb = (uint32_t)(rectify_clamp(ix[k] + 1, x0, x1) - x0);
        const uint32_t ra = (uint32_t)(rectify_clamp(iy[k], y0, y1) - y0), rw = (uint32_t)(rectify_clamp(iy[k] + 1, y0, y1) - y0);
        p[k].xa = ca * CH; p[k].xb = cb * CH; p[k].w = wts[k];
        if (use_lds) {
            p[k].oa = ra * pitch; p[k].ob = rw * pitch;
            p[k].sh = ((ra * rb) & 15u) | (((rw * rb) & 15u) << 4);
        } else {
            p[k].oa = ra * rb; p[k].ob = rw * rb; p[k].sh = 0;              // behind box0: below src_frame < 2^30
        }
    }
    uint8_t* __restrict__ drow = dst + ((size_t)py * cols + px) * CH;
    uint32_t out[kRectifyPxPerLane][CH];

    if (!use_lds) {
        for (uint32_t j = 0; j < count; ++j) {
            const uint32_t f = first + j * step;
            const uint8_t* __restrict__ g = src + (size_t)f * src_frame + box0;
#pragma unroll
            for (uint32_t k = 0; k < kRectifyPxPerLane; ++k)
                rectify_blend<CH>(p[k], 0u, 0u, [&](uint32_t o) { return (uint32_t)g[o]; }, out[k]);
            if (n_px) rectify_store<CH>(drow + (size_t)f * frame_px * CH, out, n_px);
        }
        return;
    }

    // the quads this lane stages of every frame: quad qi of box row r, up to four of them (kRectifyLdsBytes / 16 / kRectifyThreads)
    constexpr uint32_t kStage = kRectifyLdsBytes / 16 / kRectifyThreads;
    const uint32_t total = empty ? 0u : bh * quads;
    uint32_t row_off[kStage], quad_off[kStage];
#pragma unroll
    for (uint32_t s = 0; s < kStage; ++s) {
        const uint32_t idx = t + s * kRectifyThreads, r = idx / quads;
        row_off[s] = r * rb; quad_off[s] = 16u * (idx - r * quads);
    }
    const uintptr_t lo = (uintptr_t)src, hi = lo + (size_t)batch * src_frame;
    const uint8_t* L = reinterpret_cast<const uint8_t*>(lds);
    // the lane's quads of frame f into q: the loads of the NEXT frame are issued in front of a frame's taps, so that their latency
    // passes behind the arithmetic and not in front of a barrier.  A quad that holds no byte of its row is not loaded (and never read)
    uint4 q[kStage];
    const auto fetch = [&](uint32_t f) {
        const uintptr_t a0 = lo + (size_t)f * src_frame + box0;
#pragma unroll
        for (uint32_t s = 0; s < kStage; ++s) {
            q[s] = make_uint4(0, 0, 0, 0);
            if (t + s * kRectifyThreads < total) {
                const uintptr_t ar = a0 + row_off[s], qa = (ar & ~(uintptr_t)15) + quad_off[s];
                if (qa < ar + (size_t)bw * CH) {                            // the quad holds bytes of the row
                    if (qa >= lo && qa + 16 <= hi) {
                        q[s] = *reinterpret_cast<const uint4*>(qa);
                    } else {                                                // at an end of the source batch: its bytes one by one
                        uint32_t w4[4] = {0, 0, 0, 0};
                        for (uint32_t b = 0; b < 16; ++b)
                            if (qa + b >= lo && qa + b < hi) w4[b >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(qa + b) << (8u * (b & 3u));
                        q[s] = make_uint4(w4[0], w4[1], w4[2], w4[3]);
                    }
                }
            }
        }
    };
    fetch(first);
    for (uint32_t j = 0; j < count; ++j) {
        const uint32_t f = first + j * step;
        const uintptr_t a0 = lo + (size_t)f * src_frame + box0;
        if (j) __syncthreads();                                             // the last frame's taps are done with the box
#pragma unroll
        for (uint32_t s = 0; s < kStage; ++s)
            if (t + s * kRectifyThreads < total) lds[t + s * kRectifyThreads] = q[s];
        __syncthreads();
        if (j + 1 < count) fetch(f + step);
        const uint32_t c0 = (uint32_t)(a0 & 15u);
#pragma unroll
        for (uint32_t k = 0; k < kRectifyPxPerLane; ++k)
            rectify_blend<CH>(p[k], (c0 + (p[k].sh & 15u)) & 15u, (c0 + (p[k].sh >> 4)) & 15u, [&](uint32_t o) { return (uint32_t)L[o]; }, out[k]);
        if (n_px) rectify_store<CH>(drow + (size_t)f * frame_px * CH, out, n_px);
    }
}

}  // namespace dcmt
