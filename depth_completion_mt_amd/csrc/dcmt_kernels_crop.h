// dcmt_kernels_crop.h -- the two pieces of plain data movement at the library's ends, batched on the device:
//     k_crop_frames     one window out of each frame of a RAGGED batch (frames of several sizes and pitches anywhere in one source
//                       buffer, described by a device table of dcmt_crop_src records) into one uniform [batch][out_rows][out_cols]
//                       batch, elements of 1..4 opaque bytes: what every *_dev entry point takes
//     k_depth_to_u16    a dense f32 plane as the KITTI uint16 payload, cv::Mat::convertTo(CV_16U, scale): the way out
//
// k_crop_frames: grid (bands of `band` rows, frames), four waves per workgroup, a wave takes one destination row at a time.  The
// frame's record is loaded once per wave through the scalar cache (the index is blockIdx.y) and tested with crop_record_ok
// (dcmt_crop.h) before any address is formed from it; a frame whose record fails is written as zero bytes.  A row is cut by
// crop_cut_row -- the cut is wave-uniform, it lives in SGPRs -- and lane l takes pieces l, l + 64, ...: consecutive lanes store
// consecutive 16-byte pieces (1 KiB per store instruction) and load consecutive naturally aligned quads, two per piece where the
// source is not 16-byte aligned against the destination (the second is the next lane's first: one pass over the lines).  The loads
// of two pieces are issued before the first store.  The row's at most 30 end bytes go one per lane.  Vector stores only.
//
// k_depth_to_u16: the batch as one flat run of pixels, eight per lane where both pointers are 16-byte aligned (two 16-byte loads,
// one 16-byte store), one pixel per access otherwise and in the run's last partial group: the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dcmt.h"
#include "dcmt_crop.h"

namespace dcmt {

static_assert(sizeof(dcmt_crop_src) == 32 && offsetof(dcmt_crop_src, row_stride) == 8 && offsetof(dcmt_crop_src, rows) == 12 &&
              offsetof(dcmt_crop_src, x0) == 20 && offsetof(dcmt_crop_src, reserved) == 28, "dcmt_crop_src layout");

// device memory as dcmt_crop.h's functions take it: byte addresses in, accesses relative to the kernel's two global pointers out
struct CropMem {
    const uint8_t* __restrict__ src;
    uint8_t* __restrict__ dst;
    __device__ __forceinline__ void load16(uint64_t a, uint32_t* w) const
    {
        const uint4 v = *reinterpret_cast<const uint4*>(src + (a - (uint64_t)src));
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    // volatile: a byte load stays a byte load (sixteen of them side by side would otherwise be merged into one unaligned wide load)
    // (and a volatile access keeps the address space it is written with: global, named here, or it would be a flat load)
    __device__ __forceinline__ uint32_t load8(uint64_t a) const
    {
        typedef const volatile __attribute__((address_space(1))) uint8_t* GlobalByte;
        return *(GlobalByte)(src + (a - (uint64_t)src));
    }
    __device__ __forceinline__ void store16(uint64_t a, const uint32_t* o) const
    {
        *reinterpret_cast<uint4*>(dst + (a - (uint64_t)dst)) = make_uint4(o[0], o[1], o[2], o[3]);
    }
    __device__ __forceinline__ void store8(uint64_t a, uint32_t v) const { dst[a - (uint64_t)dst] = (uint8_t)v; }
};

// grid (ceil(out_rows / band), batch), kCropThreads threads.  src: src_bytes bytes; table: [batch] records; dst: [batch][out_rows]
// [out_cols] elements of elem = 1..4 bytes, out_cols * elem < 2^31.  dst overlaps neither src nor the table.
__global__ __launch_bounds__(kCropThreads)
void k_crop_frames(const uint8_t* __restrict__ src, uint64_t src_bytes, const dcmt_crop_src* __restrict__ table, uint32_t elem,
                   uint8_t* __restrict__ dst, uint32_t out_rows, uint32_t out_cols, uint32_t band)
{
    const uint32_t f = blockIdx.y;
    const uint32_t* __restrict__ rec = reinterpret_cast<const uint32_t*>(table) + 8 * (size_t)f;
    const uint32_t w0 = rec[0], w1 = rec[1], row_stride = rec[2];
    const int32_t rows = (int32_t)rec[3], cols = (int32_t)rec[4], x0 = (int32_t)rec[5], y0 = (int32_t)rec[6];
    const uint64_t offset = (uint64_t)w0 | ((uint64_t)w1 << 32);
    const bool ok = crop_record_ok(offset, row_stride, rows, cols, x0, y0, elem, (int32_t)out_rows, (int32_t)out_cols, src_bytes);

    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t len = out_cols * elem;
    const uint64_t lo = (uint64_t)src, hi = lo + src_bytes;
    const uint32_t r0 = blockIdx.x * band, r1 = out_rows - r0 < band ? out_rows : r0 + band;
    const CropMem m = {src, dst};
    for (uint32_t r = r0 + wave; r < r1; r += kCropWaves) {
        const uint64_t d = crop_row_dst((uint64_t)dst, f, out_rows, len, r);
        if (ok) {
            const uint64_t s = crop_row_src(lo, offset, row_stride, x0, y0, elem, r);
            const RowCut c = crop_cut_row(d, s, len);
            for (uint32_t p = lane; p < c.pieces; p += 128u) {
                uint32_t wa[8], wb[8], o[4];
                const bool two = p + 64u < c.pieces;
                const bool da = crop_fetch_piece(m, c, s, p, lo, hi, wa);
                const bool db = two && crop_fetch_piece(m, c, s, p + 64u, lo, hi, wb);
                crop_assemble(wa, c.sh, da, o);
                m.store16(crop_piece_dst(c, d, p), o);
                if (two) {
                    crop_assemble(wb, c.sh, db, o);
                    m.store16(crop_piece_dst(c, d, p + 64u), o);
                }
            }
            if (lane < c.head + c.tail) crop_copy_edge(m, c, d, s, lane);
        } else {
            const RowCut c = crop_cut_row(d, 0, len);
            const uint32_t z[4] = {0, 0, 0, 0};
#pragma clang loop vectorize(disable) unroll(disable)
            for (uint32_t p = lane; p < c.pieces; p += 64u) m.store16(crop_piece_dst(c, d, p), z);       // (vectorised, it came out as dword stores)
            if (lane < c.head + c.tail) m.store8(d + crop_edge_pos(c, lane), 0);
        }
    }
}

// ---- f32 depth -> uint16 payload ------------------------------------------------------------------------------------------
// t = x * scale rounded once; rint, ties to even (v_rndne_f32); saturated to 0..65535 on t's BIT PATTERN: the library is built
// with -ffinite-math-only and t may be +Inf for a finite x, so no float compare decides anything here.  A set sign bit (negatives,
// -0.0) gives 0; bits >= those of 65535.0f, read as integers (everything from 65535 up, +Inf), give 65535.
__device__ __forceinline__ uint32_t depth_u16(float x, float scale)
{
    const float t = __fmul_rn(x, scale);
    const uint32_t b = __float_as_uint(t);
    const bool low = (b >> 31) != 0, high = b >= 0x477fff00u;
    const uint32_t r = (uint32_t)(int32_t)__builtin_rintf(low || high ? 0.0f : t);      // the conversion only ever sees 0 <= t < 65535
    return low ? 0u : high ? 65535u : r;
}

// grid ceil(total / (kU16Threads * kU16PxPerLane)), kU16Threads threads; total <= kU16SegPx (dcmt_plan_side.h).  kVec: src and out
// are 16-byte aligned.
template <bool kVec>
__global__ __launch_bounds__(kU16Threads)
void k_depth_to_u16(const float* __restrict__ src, uint32_t total, float scale, uint16_t* __restrict__ out)
{
    const uint32_t q = (blockIdx.x * kU16Threads + threadIdx.x) * kU16PxPerLane;
    if (q >= total) return;
    if (kVec && total - q >= kU16PxPerLane) {
        const float4 a = reinterpret_cast<const float4*>(src + q)[0], b = reinterpret_cast<const float4*>(src + q)[1];
        uint4 o;
        o.x = depth_u16(a.x, scale) | (depth_u16(a.y, scale) << 16);
        o.y = depth_u16(a.z, scale) | (depth_u16(a.w, scale) << 16);
        o.z = depth_u16(b.x, scale) | (depth_u16(b.y, scale) << 16);
        o.w = depth_u16(b.z, scale) | (depth_u16(b.w, scale) << 16);
        *reinterpret_cast<uint4*>(out + q) = o;
    } else {
#pragma unroll
        for (uint32_t i = 0; i < kU16PxPerLane; ++i)
            if (q + i < total) out[q + i] = (uint16_t)depth_u16(src[q + i], scale);
    }
}

}  // namespace dcmt
