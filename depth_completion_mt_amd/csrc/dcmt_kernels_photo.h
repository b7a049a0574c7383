// dcmt_kernels_photo.h -- get_initial_error (DC_stereo_lidar/main_sl.cpp:618-712, its data: :636-682 and the count of :696) for a batch
// of dense depth planes and grey stereo pairs: per pixel the square root of the sum of squared differences between a window of the
// left image and the same window of the right image at the disparity the pixel's depth implies, as a byte, and four counts per
// frame.  The definition, to the last bit, is in include/dcmt.h (dcmt_photo_error_dev); this file is its two kernels.
//
// Everything is integer but three f32 operations (the product baseline * focal, the quotient by the depth, the difference from the
// column), and everything that is DECIDED about a float is decided on its bits: the library is built with -ffinite-math-only, so a
// float compare against a NaN or an infinity is one the compiler may remove.
//
//   k_photo_error<W>        the LDS route.  grid (bands, frames), 256 threads.  A workgroup owns `band` output rows of one frame across
//                           the whole width and stages the band + 2 W - 1 rows its windows read, of both images, into LDS (16-byte
//                           loads and stores where `vec`): a row lies kPhotoPadLeft bytes behind the start of its pitch, so that a
//                           window that hangs over either end of the row reads pad bytes, never another row's or nothing's.  Pad
//                           bytes and rows outside the frame are never written and may hold anything: every tap the definition
//                           excludes is ANDed to zero in BOTH operands, so it adds nothing.  A lane does four adjacent pixels of
//                           a row: one 16-byte depth load, three LDS dwords of the left row (columns j0 - 4 .. j0 + 7) serve all
//                           four windows, and each pixel's right window -- 2 W bytes at a data-dependent byte offset -- comes from
//                           the two or three aligned dwords around it and v_alignbyte.  The squared differences are never formed
//                           byte by byte: sum (l - r)^2 = sum l^2 + sum r^2 - 2 sum l r, three packed unsigned 8-bit dot products
//                           (v_dot4_u32_u8) per dword of window and row, the sums running on in the accumulator operand from row
//                           to row, exact in 32-bit integers (a window's sum is at most 64 * 255^2 < 2^23).  W is a template
//                           argument: the byte offsets of the four left windows are constants.
//   k_photo_error_global    the fallback route, for frames so wide that one output row's window rows do not fit the LDS budget.
//                           grid (ceil(rows * cols / 256), frames), a thread per pixel, the taps read from global memory with the
//                           definition's conditions as written.  The same integers.
//
// The square root is the integer square root, bit by bit on the sum clamped to 255^2: eight steps, no floating point whose rounding
// would have to be argued.  The four counts are summed per lane in 32 bits (a workgroup sees at most 2^16 pixels of at most 64
// matches), reduced per wave and per workgroup, and leave as one 64-bit integer atomic add per workgroup and word; the call has
// cleared them in front of the kernel.
//
// G: PhotoK, the call's baseline and focal by value (dcmt_photo_error_dev), or PhotoTable, the device's [batch] 8-byte records
// (dcmt_photo_error_calib_dev), of which the workgroup takes record blockIdx.y: two dwords, loaded as integers and tested as the host
// tests the uniform call's (finite, positive).  A frame whose record fails is written as zeros and counts nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dcmt.h"
#include "dcmt_photo.h"

namespace dcmt {

struct PhotoK { float baseline, focal; };
struct PhotoTable { const dcmt_stereo_calib* __restrict__ records; };

// a finite f32 above zero, on its bits
__device__ __forceinline__ bool photo_positive_finite(uint32_t b) { return (int32_t)b > 0 && b < 0x7f800000u; }

// baseline * focal, one rounded product (:648); false for a record the call refuses
__device__ __forceinline__ bool photo_record(const PhotoK& k, uint32_t, float& bf)
{
    bf = __fmul_rn(k.baseline, k.focal);
    return true;
}
__device__ __forceinline__ bool photo_record(const PhotoTable& t, uint32_t f, float& bf)
{
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(t.records) + 2 * (size_t)f;
    const uint32_t bb = w[0], fb = w[1];
    bf = __fmul_rn(__uint_as_float(bb), __uint_as_float(fb));
    return photo_positive_finite(bb) && photo_positive_finite(fb);
}

// Steps 1 - 4 of the definition for the pixel in column j whose depth has the bits db: true where the pixel is valid, pr its column
// in the right image; pr = 1 otherwise, so that an address formed from it stays inside the staged row.  bf_finite: the product did not
// overflow (where it did, the disparity is infinite or NaN for every depth: no pixel is inside).
__device__ __forceinline__ bool photo_target(uint32_t db, int j, float bf, bool bf_finite, int cols, int& pr)
{
    pr = 1;
    if (!((int32_t)db > 0 && db <= 0x7f800000u) || !bf_finite) return false;          // !(depth > 0): zeros, negatives, NaN
    const float disparity = db == 0x7f800000u ? 0.0f : __fdiv_rn(bf, __uint_as_float(db));
    const float t = __fsub_rn((float)j, disparity);
    const uint32_t tb = __float_as_uint(t);
    if (!(tb >= 0x3f800000u && tb < 0x4f000000u)) return false;                         // 1 <= t < 2^31, which no NaN satisfies
    const int q = (int)t;
    if (q >= cols) return false;
    pr = q;
    return true;
}

// min(255, floor(sqrt(n)))
__device__ __forceinline__ uint32_t photo_isqrt255(uint32_t n)
{
    n = n < 65025u ? n : 65025u;
    uint32_t r = 0;
#pragma unroll
    for (int b = 7; b >= 0; --b) {
        const uint32_t c = r | (1u << b);
        if (c * c <= n) r = c;
    }
    return r;
}

// bytes lo .. hi - 1 of eight set; 0 <= lo <= 8, hi <= 8
__device__ __forceinline__ uint64_t photo_byte_mask(int lo, int hi)
{
    if (hi <= lo) return 0;
    const uint64_t below_hi = hi >= 8 ? ~0ull : (1ull << (8 * hi)) - 1ull;
    return below_hi & ~((1ull << (8 * lo)) - 1ull);
}

// the same of four, for a window of one dword (hi <= 4)
__device__ __forceinline__ uint32_t photo_byte_mask32(int lo, int hi)
{
    if (hi <= lo) return 0;
    const uint32_t below_hi = hi >= 4 ? ~0u : (1u << (8 * hi)) - 1u;
    return below_hi & ~((1u << (8 * lo)) - 1u);
}

// the four counts of a workgroup's lanes into the frame's statistics
__device__ __forceinline__ void photo_add_stats(unsigned long long* __restrict__ stats, uint32_t f, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3)
{
    __shared__ uint32_t s_part[kPhotoThreads / 64][4];
    uint32_t v[4] = {v0, v1, v2, v3};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[k] += (uint32_t)__shfl_xor((int)v[k], d, 64);
    const uint32_t tid = threadIdx.x;
    if ((tid & 63u) == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) s_part[tid >> 6][k] = v[k];
    __syncthreads();
    if (tid < 4) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < kPhotoThreads / 64; ++w) sum += s_part[w][tid];
        if (sum != 0) atomicAdd(stats + 4 * (size_t)f + tid, (unsigned long long)sum);
    }
}

// the dword at byte offset s of three consecutive dwords, s + 4 <= 12
__device__ __forceinline__ uint32_t photo_dword_at(const uint32_t (&L)[3], int s)
{
    const int k = s >> 2, sh = s & 3;
    return sh == 0 ? L[k] : __builtin_amdgcn_alignbyte(L[k + 1 < 3 ? k + 1 : 2], L[k], (uint32_t)sh);
}

template <int W, typename G>
__global__ __launch_bounds__(kPhotoThreads)
void k_photo_error(const uint32_t* __restrict__ depth, const uint8_t* __restrict__ left, const uint8_t* __restrict__ right,
                   uint8_t* __restrict__ err, unsigned long long* __restrict__ stats, int rows, int cols, uint32_t band, uint32_t pitch, int vec, G P)
{
    static_assert(W >= 1 && W <= kPhotoMaxWindow, "window");
    constexpr int NW = (2 * W + 3) / 4;                    // dwords of a window's row
    extern __shared__ __attribute__((aligned(16))) uint8_t s_photo[];
    const uint32_t f = blockIdx.y, tid = threadIdx.x;
    const int i0 = (int)(blockIdx.x * band);
    const uint32_t nb = (uint32_t)(rows - i0) < band ? (uint32_t)(rows - i0) : band;       // the band's rows inside the frame
    const size_t frame = (size_t)f * (size_t)rows * (size_t)cols;
    float bf;
    if (!photo_record(P, f, bf)) {
        if (err) {
            uint8_t* __restrict__ o = err + frame + (size_t)i0 * cols;
            for (size_t k = tid; k < (size_t)nb * cols; k += kPhotoThreads) o[k] = 0;
        }
        return;
    }
    const bool bf_finite = (__float_as_uint(bf) & 0x7f800000u) != 0x7f800000u;

    // stage rows i0 - W .. i0 + band + W - 2 of both images, those inside the frame
    const uint32_t S = photo_staged_rows(band, W);
    uint8_t* const sl = s_photo;
    uint8_t* const sr = s_photo + (size_t)S * pitch;
    const int r0 = i0 - W;
    if (vec) {
        const uint32_t c16 = (uint32_t)cols >> 4;
        for (uint32_t idx = tid; idx < S * c16; idx += kPhotoThreads) {
            const uint32_t s = idx / c16, c = idx - s * c16;
            const int r = r0 + (int)s;
            if (r < 0 || r >= rows) continue;
            const size_t g = frame + (size_t)r * cols + 16 * c;
            const uint4 a = *reinterpret_cast<const uint4*>(left + g);
            const uint4 b = *reinterpret_cast<const uint4*>(right + g);
            *reinterpret_cast<uint4*>(sl + s * pitch + kPhotoPadLeft + 16 * c) = a;
            *reinterpret_cast<uint4*>(sr + s * pitch + kPhotoPadLeft + 16 * c) = b;
        }
    } else {
        for (uint32_t idx = tid; idx < S * (uint32_t)cols; idx += kPhotoThreads) {
            const uint32_t s = idx / (uint32_t)cols, c = idx - s * (uint32_t)cols;
            const int r = r0 + (int)s;
            if (r < 0 || r >= rows) continue;
            const size_t g = frame + (size_t)r * cols + c;
            sl[s * pitch + kPhotoPadLeft + c] = left[g];
            sr[s * pitch + kPhotoPadLeft + c] = right[g];
        }
    }
    __syncthreads();

    const uint32_t nq = ((uint32_t)cols + 3u) >> 2;        // quads of a row
    uint32_t n_valid = 0, n_match = 0, n_nonzero = 0, sum_err = 0;
    for (uint32_t t = tid; t < nb * nq; t += kPhotoThreads) {
        const uint32_t row = t / nq, q = t - row * nq;
        const int i = i0 + (int)row, j0 = (int)(4 * q);
        const size_t g = frame + (size_t)i * cols + j0;
        uint32_t db[4];
        if (vec) {
            const uint4 d = *reinterpret_cast<const uint4*>(depth + g);
            db[0] = d.x; db[1] = d.y; db[2] = d.z; db[3] = d.w;
        } else {
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) db[qq] = j0 + qq < cols ? depth[g + qq] : 0u;
        }
        int pr[4];
        uint32_t m0[4], m1[4], nk[4], sq[4], cr[4], ra[4], rs[4];
        bool ok[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int j = j0 + qq;
            ok[qq] = photo_target(db[qq], j, bf, bf_finite, cols, pr[qq]);
            // tap b = k + W is kept iff 0 < j - W + b < cols and 0 < pr - W + b < cols and b < 2 W
            const int lo_c = j < pr[qq] ? j : pr[qq], hi_c = j < pr[qq] ? pr[qq] : j;
            const int lo = W + 1 - lo_c > 0 ? W + 1 - lo_c : 0;
            const int hi = W + cols - hi_c < 2 * W ? W + cols - hi_c : 2 * W;
            if constexpr (NW == 1) {
                m0[qq] = ok[qq] ? photo_byte_mask32(lo, hi) : 0u; m1[qq] = 0;
            } else {
                const uint64_t m = ok[qq] ? photo_byte_mask(lo, hi) : 0ull;
                m0[qq] = (uint32_t)m; m1[qq] = (uint32_t)(m >> 32);
            }
            // the right window's first byte within a staged row (the pitch is a multiple of 16): its aligned dword and its byte in it
            const uint32_t ob = kPhotoPadLeft + (uint32_t)(pr[qq] - W);
            ra[qq] = ob & ~3u; rs[qq] = ob & 3u;
            nk[qq] = ok[qq] && hi > lo ? (uint32_t)(hi - lo) : 0u;
            sq[qq] = 0; cr[qq] = 0;                         // sum l^2 + sum r^2 (at most 2 * 64 * 255^2), sum l r
        }
        uint32_t n_rows = 0;
#pragma unroll
        for (int p = 0; p < 2 * W; ++p) {
            const int r = i + p - W;
            const bool row_ok = r > 0 && r < rows;
            n_rows += row_ok ? 1u : 0u;
            const uint32_t slot = row + (uint32_t)p;
            const uint32_t* lrow = reinterpret_cast<const uint32_t*>(sl + slot * pitch + kPhotoPadLeft + (uint32_t)j0 - 4u);
            const uint32_t L[3] = {lrow[0], lrow[1], lrow[2]};         // columns j0 - 4 .. j0 + 7
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const uint32_t* rp = reinterpret_cast<const uint32_t*>(sr + slot * pitch + ra[qq]);
                const uint32_t sh = rs[qq];
                const uint32_t R0 = rp[0], R1 = rp[1];
                const uint32_t mk0 = row_ok ? m0[qq] : 0u;
                const uint32_t l0 = photo_dword_at(L, 4 + qq - W) & mk0;
                const uint32_t q0 = __builtin_amdgcn_alignbyte(R1, R0, sh) & mk0;
                uint32_t squares = __builtin_amdgcn_udot4(l0, l0, sq[qq], false);      // the sums run on in the accumulator operand
                squares = __builtin_amdgcn_udot4(q0, q0, squares, false);
                uint32_t cross = __builtin_amdgcn_udot4(l0, q0, cr[qq], false);
                if constexpr (NW == 2) {
                    const uint32_t R2 = rp[2];
                    const uint32_t mk1 = row_ok ? m1[qq] : 0u;
                    const uint32_t l1 = photo_dword_at(L, 8 + qq - W) & mk1;
                    const uint32_t q1 = __builtin_amdgcn_alignbyte(R2, R1, sh) & mk1;
                    squares = __builtin_amdgcn_udot4(l1, l1, squares, false);
                    squares = __builtin_amdgcn_udot4(q1, q1, squares, false);
                    cross = __builtin_amdgcn_udot4(l1, q1, cross, false);
                }
                sq[qq] = squares; cr[qq] = cross;
            }
        }
        uint32_t e[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            e[qq] = photo_isqrt255(sq[qq] - 2u * cr[qq]);  // (a pixel that is not valid has an empty mask: 0)
            n_valid += ok[qq] ? 1u : 0u;
            n_match += nk[qq] * n_rows;
            n_nonzero += e[qq] != 0 ? 1u : 0u;
            sum_err += e[qq];
        }
        if (err) {
            if (vec) *reinterpret_cast<uint32_t*>(err + g) = e[0] | (e[1] << 8) | (e[2] << 16) | (e[3] << 24);
            else {
#pragma unroll
                for (int qq = 0; qq < 4; ++qq)
                    if (j0 + qq < cols) err[g + qq] = (uint8_t)e[qq];
            }
        }
    }
    if (stats) photo_add_stats(stats, f, n_valid, n_match, n_nonzero, sum_err);
}

template <typename G>
__global__ __launch_bounds__(kPhotoThreads)
void k_photo_error_global(const uint32_t* __restrict__ depth, const uint8_t* __restrict__ left, const uint8_t* __restrict__ right,
                          uint8_t* __restrict__ err, unsigned long long* __restrict__ stats, int rows, int cols, int window, G P)
{
    const uint32_t f = blockIdx.y, n = (uint32_t)rows * (uint32_t)cols;
    const uint32_t idx = blockIdx.x * kPhotoGlobalPx + threadIdx.x;
    const size_t frame = (size_t)f * (size_t)n;
    float bf;
    if (!photo_record(P, f, bf)) {
        if (err && idx < n) err[frame + idx] = 0;
        return;
    }
    const bool bf_finite = (__float_as_uint(bf) & 0x7f800000u) != 0x7f800000u;
    uint32_t valid = 0, matches = 0, e = 0;
    if (idx < n) {
        const int i = (int)(idx / (uint32_t)cols), j = (int)(idx - (uint32_t)i * (uint32_t)cols);
        int pr;
        if (photo_target(depth[frame + idx], j, bf, bf_finite, cols, pr)) {
            valid = 1;
            uint32_t ssd = 0;
            for (int p = -window; p < window; ++p) {
                const int r = i + p;
                if (!(r > 0 && r < rows)) continue;
                const uint8_t* __restrict__ lr = left + frame + (size_t)r * cols;
                const uint8_t* __restrict__ rr = right + frame + (size_t)r * cols;
                for (int k = -window; k < window; ++k) {
                    if (!(j + k > 0 && j + k < cols && pr + k > 0 && pr + k < cols)) continue;
                    const int d = (int)lr[j + k] - (int)rr[pr + k];
                    ssd += (uint32_t)(d * d);
                    ++matches;
                }
            }
            e = photo_isqrt255(ssd);
        }
        if (err) err[frame + idx] = (uint8_t)e;
    }
    if (stats) photo_add_stats(stats, f, valid, matches, e != 0 ? 1u : 0u, e);
}

}  // namespace dcmt
