// dcmt_kernels_cloud.h -- what DC_stereo_lidar/main_sl.cpp does with the refined depth after the path (:1251-1270), batched on
// the device:
//     cv::GaussianBlur(optimized_depth, optimized_depth, cv::Size(5, 5), 0);                         (:1253)  k_gauss5
//     reproject_pc_colors(optimized_depth, colour image, ...)  /  reproject_pc(optimized_depth)      (:924-965, :887-922)
//
// Back-projection: every pixel with depth > 0 (an f32 compare) becomes one 16-byte record, frames in batch order, pixels
// row-major -- the reference's push_back order:
//     z = depth;  x_ = (float)(((double)x - cx) * (double)z / fx);  y_ = (float)(((double)y - cy) * (double)z / fy);
// f64 subtraction, product and a true division, one rounding each, then one rounding to f32.  The fourth dword holds
// b | g << 8 | r << 16 | 255 << 24 from the colour plane (PointXYZRGB), or 1.0f without one (PointXYZ's padding, and the
// [x y z w] record dcmt_project_points_dev reads).
//
// An order-preserving stream compaction with integer counts only; no workgroup waits on another, no atomics:
//   k_cloud_count    one workgroup per (chunk, frame), the chunking of dcmt_kernels_eval.h.  A frame is a flat run of groups
//                    of 4 pixels; each of the workgroup's 4 waves owns a contiguous quarter of the chunk's groups and walks it
//                    64 groups (256 pixels) per step, lane l on group l of the step.  One count per wave to the slab:
//                    [frame][chunk][wave] uint32;
//   k_cloud_scan     ONE workgroup: the exclusive scan of the slab in (frame, chunk, wave) order, in place, and d_offsets
//                    (the base of each frame's first entry, and the total).  Integer sums: the result does not depend on how
//                    the slab is cut among the workgroup's waves;
//   k_cloud_scatter  the same runs.  A wave carries a wave-uniform base, advanced by the popcount of each step; inside a step
//                    the rank of pixel i of lane l = sum_k mbcnt(ballot_k) + the lane's own earlier pixels.  (row, col) from one
//                    integer division per group and a carry.  The step's records go through a per-wave LDS stage in rank order
//                    (no workgroup barrier: a wave only reads what it wrote itself), so that lane l of a round computes and
//                    stores record 64 * round + l: consecutive 16-byte stores, and on a sparse plane one round of f64
//                    divisions per step with every lane at work instead of four with a few.  64-bit addressing; a record
//                    whose global index is >= capacity is not stored.
// Depth loads are 16 bytes at any dword alignment and colour loads 12 bytes at any byte alignment (gfx950's global loads run
// in unaligned mode, as k_eval_partial / k_color_minmax rely on); the partial last group of a frame (n % 4 pixels) goes pixel
// by pixel.  A frame's records depend only on its own pixels; only the base depends on what lies in front of it.
// Bytes per pixel: 4 (count) + 4 (re-read) + 3 (colour) + 16 * (share of pixels with depth > 0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dcmt_calib.h"
#include "dcmt_cloud.h"
#include "dcmt_gauss.h"

namespace dcmt {

constexpr int kCloudThreads = 64 * kCloudWaves;
constexpr int kCloudScanThreads = 1024;

// (float)(((double)i - c) * (double)z / f): the x_ (i = column, c = cx, f = fx) or y_ (row, cy, fy) of a pixel of depth z.  f64
// subtraction, product and a true division, one rounding each, then one rounding to f32 (k_cloud_scatter, and the kernels of
// dcmt_kernels_reproject.h)
__device__ __forceinline__ float unproject_axis(uint32_t i, double c, double z, double f)
{
    return (float)__ddiv_rn(__dmul_rn(__dsub_rn((double)i, c), z), f);
}

// the groups [ws, we) of wave w of chunk c (G groups per chunk: eval_chunk_groups(n)): a contiguous quarter of the chunk
__device__ __forceinline__ void cloud_wave_run(uint32_t n, uint32_t G, uint32_t c, uint32_t w, uint32_t& ws, uint32_t& we)
{
    const uint32_t ng = (n + 3) / 4;
    const uint32_t g0 = c * G, g1 = min(g0 + G, ng), W = (G + kCloudWaves - 1) / kCloudWaves;
    ws = min(g0 + w * W, g1);
    we = min(ws + W, g1);
}

// the 4 pixels of group g of a frame (0 where the group is beyond the run or the pixel beyond the frame)
__device__ __forceinline__ void cloud_load4(const float* __restrict__ p, uint32_t g, uint32_t n, bool active, float d[4])
{
    if (active && g < n / 4) {
        float4 t;
        __builtin_memcpy(&t, p + 4 * (size_t)g, sizeof t);
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t q = 4 * g + i;
            d[i] = active && q < n ? p[q] : 0.0f;
        }
    }
}

// The intrinsics as the argument `geo` of k_cloud_count and k_cloud_scatter: CloudK itself, by value (dcmt_depth_to_cloud_dev), or a
// table of per-frame records (dcmt_depth_to_cloud_calib_dev, dcmt_calib.h), of which the workgroup takes record blockIdx.y -- loaded
// once per wave through the scalar cache in front of the pixel loop, into the SGPRs where the by-value argument lies
struct CloudTable { const dcmt_cloud_params* __restrict__ records; };
__device__ __forceinline__ const CloudK& cloud_k(const CloudK& arg, const CloudK&) { return arg; }
__device__ __forceinline__ const CloudK& cloud_k(const CloudTable&, const CloudK& rec) { return rec; }

// grid (eval_chunks(n), frames), 256 threads; G = eval_chunk_groups(n).  slab: [frames][chunks][kCloudWaves] counts.  The count does
// not depend on the intrinsics: the CloudK instance takes them last and reads nothing of them (its text is that of a kernel without
// the argument but for the offset of the hidden gridDim.x behind it: DESIGN.md section 34); the CloudTable instance tests the frame's record, and a frame whose record is bad counts nothing, so the scan's
// offsets stay true and k_cloud_scatter<.., CloudTable>, which skips the frame, leaves no gap
template <typename KSrc = CloudK>
__global__ __launch_bounds__(kCloudThreads)
void k_cloud_count(const float* __restrict__ depth, uint32_t n, uint32_t G, uint32_t* __restrict__ slab, KSrc geo)
{
    if constexpr (std::is_same_v<KSrc, CloudTable>) {
        CloudK rec;
        if (!load_cloud_record(geo.records, blockIdx.y, rec)) {         // wave-uniform: one scalar load per wave
            if ((threadIdx.x & 63) == 0) slab[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kCloudWaves + threadIdx.x / 64] = 0u;
            return;
        }
    }
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), l = threadIdx.x & 63;
    const float* __restrict__ p = depth + (size_t)blockIdx.y * n;
    uint32_t ws, we;
    cloud_wave_run(n, G, blockIdx.x, w, ws, we);
    uint32_t cnt = 0;
    for (uint32_t gb = ws; gb < we; gb += 64) {
        float d[4];
        cloud_load4(p, gb + l, n, gb + l < we, d);
#pragma unroll
        for (int i = 0; i < 4; ++i) cnt += (uint32_t)__popcll(__ballot(d[i] > 0.0f));
    }
    if (l == 0) slab[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kCloudWaves + w] = cnt;
}

// one workgroup of 1024 threads.  slab: entries counts in, exclusive bases out; per = entries per frame (chunks * kCloudWaves, a
// multiple of 4); offsets: [frames + 1].  Each of the 16 waves owns one contiguous sixteenth of the slab and walks it in tiles of
// 256 entries, 16 bytes per lane: first the wave's total, then -- behind the one barrier, with the totals of the waves in front
// as the carry -- the scan of its tiles (4 entries in the lane, a shuffle scan over the lanes, a wave-uniform carry).
__global__ __launch_bounds__(kCloudScanThreads)
void k_cloud_scan(uint32_t* __restrict__ slab, uint32_t entries, uint32_t per, uint32_t frames, int32_t* __restrict__ offsets)
{
    constexpr uint32_t kWaves = kCloudScanThreads / 64;
    __shared__ uint32_t wsum[kWaves];
    const uint32_t l = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
    const uint32_t S = ((entries + kWaves - 1) / kWaves + 255) & ~255u;
    const uint32_t s0 = min(w * S, entries), s1 = min(s0 + S, entries);       // multiples of 4: an access is inside or outside
    uint4* __restrict__ v = reinterpret_cast<uint4*>(slab);
    uint32_t s = 0;
#pragma unroll 4
    for (uint32_t e = s0 + 4 * l; e < s1; e += 256) { const uint4 a = v[e / 4]; s += a.x + a.y + a.z + a.w; }
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (l == 0) wsum[w] = s;
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t j = 0; j < w; ++j) run += wsum[j];
    if (threadIdx.x == kCloudScanThreads - 1) offsets[frames] = (int32_t)(run + s);
    for (uint32_t tb = s0; tb < s1; tb += 256) {
        const uint32_t e = tb + 4 * l;
        uint4 a = {0u, 0u, 0u, 0u};
        if (e < s1) a = v[e / 4];
        const uint32_t t = a.x + a.y + a.z + a.w;
        uint32_t inc = t;
        for (int m = 1; m < 64; m <<= 1) { const uint32_t o = __shfl_up(inc, m, 64); if ((int)l >= m) inc += o; }
        if (e < s1) {
            uint4 b;
            b.x = run + inc - t; b.y = b.x + a.x; b.z = b.y + a.y; b.w = b.z + a.z;
            if (e % per == 0) offsets[e / per] = (int32_t)b.x;                 // per % 4 == 0: a frame starts on an access
            v[e / 4] = b;
        }
        run += __shfl(inc, 63, 64);
    }
}

// grid (eval_chunks(n), frames), 256 threads.  slab: the bases k_cloud_scan left.  bgr: [frames][n][3] bytes or null.  geo: as for
// k_cloud_count; a frame whose record is bad was counted as empty there and is skipped
template <bool kColor, typename KSrc = CloudK>
__global__ __launch_bounds__(kCloudThreads)
void k_cloud_scatter(const float* __restrict__ depth, const uint8_t* __restrict__ bgr, uint32_t n, uint32_t G, uint32_t cols, KSrc geo,
                     const uint32_t* __restrict__ slab, uint4* __restrict__ points, uint32_t capacity)
{
    [[maybe_unused]] CloudK rec;
    if constexpr (std::is_same_v<KSrc, CloudTable>)
        if (!load_cloud_record(geo.records, blockIdx.y, rec)) return;
    const CloudK& k = cloud_k(geo, rec);
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), l = threadIdx.x & 63;
    const float* __restrict__ p = depth + (size_t)blockIdx.y * n;
    const uint8_t* __restrict__ cp = kColor ? bgr + 3 * (size_t)blockIdx.y * n : nullptr;
    uint32_t ws, we;
    cloud_wave_run(n, G, blockIdx.x, w, ws, we);
    __shared__ uint4 stage_all[kCloudWaves][256];          // per wave: the records of one step (up to 256), in rank order
    uint4* stage = stage_all[w];
    uint32_t base = slab[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kCloudWaves + w];     // wave-uniform
    if (base >= capacity) return;                         // the whole run lies beyond the caller's room
    for (uint32_t gb = ws; gb < we; gb += 64) {
        const uint32_t g = gb + l, q = 4 * g;
        const bool active = g < we;
        float d[4];
        cloud_load4(p, g, n, active, d);
        uint32_t c[4] = {0x3f800000u, 0x3f800000u, 0x3f800000u, 0x3f800000u};       // 1.0f
        if (kColor) {
            if (active && g < n / 4) {
                uint3 t;
                __builtin_memcpy(&t, cp + 3 * (size_t)q, sizeof t);
                c[0] = t.x | 0xff000000u;
                c[1] = (t.x >> 24) | (t.y << 8) | 0xff000000u;
                c[2] = (t.y >> 16) | (t.z << 16) | 0xff000000u;
                c[3] = (t.z >> 8) | 0xff000000u;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (active && q + i < n) {
                        const uint8_t* s = cp + 3 * (size_t)(q + i);
                        c[i] = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | 0xff000000u;
                    }
            }
        }
        bool v[4];
        uint32_t lower = 0, step = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = d[i] > 0.0f;
            const unsigned long long b = __ballot(v[i]);
            lower += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            step += (uint32_t)__popcll(b);
        }
        // the step's records in rank order to the wave's LDS stage (pixel, row, column, fourth dword) ...
        uint32_t r = lower;
        uint32_t row = q / cols, col = q - row * cols;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i > 0 && ++col == cols) { col = 0; ++row; }
            if (v[i]) {
                uint4 e;
                e.x = __float_as_uint(d[i]); e.y = col; e.z = row; e.w = c[i];
                stage[r++] = e;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ... and out again 64 at a time: lane l computes and stores record j + l, so a store instruction writes consecutive
        // records and every lane of a round divides (one round per step on a sparse plane, four on a dense one)
        for (uint32_t j = 0; j < step; j += 64) {
            const uint32_t slot = j + l;
            if (slot < step && base + slot < capacity) {
                const uint4 e = stage[slot];
                const double z = (double)__uint_as_float(e.x);
                uint4 o;
                o.x = __float_as_uint(unproject_axis(e.y, k.cx, z, k.fx));
                o.y = __float_as_uint(unproject_axis(e.z, k.cy, z, k.fy));
                o.z = e.x;
                o.w = e.w;
                points[(size_t)(base + slot)] = o;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        base += step;
    }
}

// ---- cv::GaussianBlur(src, dst, Size(5, 5), 0) without the cascade's masked select ------------------------------------------
// [1 4 6 4 1]/16, rows then columns, BORDER_REFLECT_101 (reflect101: 0 for a length of 1, repeated reflection for 2), each pass
// gauss_taps.  A wave streams down a strip of 64 columns (60 outputs, 2 halo columns either side; lane l holds column
// x0 - 2 + l, reflected into the frame) over a band of band_rows output rows (kGaussRows; fewer for a handful of frames, so that
// they still make a few thousand waves): a row is one coalesced load per lane, its
// neighbours come through lane shuffles, the row pass results of the last 5 rows stay in registers for the column pass.  No LDS,
// no barrier; the loads of kGaussBatch rows go out together.  src and dst must not overlap (the entry point sends an in-place
// call through scratch).
constexpr int kGaussBatch = 6;      // (kGaussCols, kGaussRows: dcmt_cloud.h)

// grid (ceil(strips * bands / 4), frames), 256 threads: one wave per (strip, band); strips = ceil(cols / kGaussCols),
// bands = ceil(rows / band_rows)
//
// VALID: the Gaussian that ignores holes (dcmt_gaussian5_valid_dev, and the cascade's "gaussian_valid" finish), dcmt.h's GV: with
// v(x) = x >= thr, num = G5(v ? x : 0) and den = G5(v ? 1 : 0) run side by side through the same shuffles and rings -- den is exact,
// a multiple of 1/256 -- and a valid pixel stores num / den (one IEEE division), an invalid one its own bits.  A wave whose output
// lanes all have den == 1 (every tap valid: the interior of a filled region) skips the division: num / 1.0f is num.
// INVERT: the cascade's final invert (y >= thr ? max_depth - y : y) in the store.  thr and max_depth are read by those instances only.
template <bool VALID = false, bool INVERT = false>
__global__ __launch_bounds__(256)
void k_gauss5(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols, int strips, int bands, int band_rows, float thr,
              float max_depth)
{
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), l = threadIdx.x & 63;
    const int id = blockIdx.x * 4 + w;
    if (id >= strips * bands) return;
    const int band = id / strips, strip = id - band * strips;
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    const float* __restrict__ s = src + fo;
    const int gx = strip * kGaussCols - 2 + l;
    // columns and rows beyond the frame's own reflection zone are clamped to something readable; no output depends on them
    const int cx = reflect101(min(gx, cols + 1), cols);
    const bool out_col = l >= 2 && l < 62 && gx < cols;
    const int y0 = band * band_rows, R = min(band_rows, rows - y0);
    float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f, h3 = 0.0f, h4 = 0.0f;
    [[maybe_unused]] float k0 = 0.0f, k1 = 0.0f, k2 = 0.0f, k3 = 0.0f, k4 = 0.0f;     // VALID: the row pass of the mask
    [[maybe_unused]] float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;                           // VALID: the source rows i - 2, i - 1, i
    for (int i0 = 0; i0 < R + 4; i0 += kGaussBatch) {          // input row i of the band is frame row y0 + i - 2
        float v[kGaussBatch];
#pragma unroll
        for (int j = 0; j < kGaussBatch; ++j) {
            const int sy = reflect101(min(y0 + i0 + j - 2, rows + 1), rows);
            v[j] = s[(size_t)sy * cols + cx];
        }
#pragma unroll
        for (int j = 0; j < kGaussBatch; ++j) {
            const int i = i0 + j;
            if (i < R + 4) {                                   // wave-uniform
                float x = v[j];
                if constexpr (VALID) {
                    const bool ok = x >= thr;                  // (NaN: not valid)
                    const float m = ok ? 1.0f : 0.0f;
                    c0 = c1; c1 = c2; c2 = x;
                    x = ok ? x : 0.0f;                         // a select, not a product: +inf stays +inf
                    const float ml1 = __shfl_up(m, 1, 64), mr1 = __shfl_down(m, 1, 64);
                    const float ml2 = __shfl_up(m, 2, 64), mr2 = __shfl_down(m, 2, 64);
                    k0 = k1; k1 = k2; k2 = k3; k3 = k4;
                    k4 = gauss_taps(m, __fadd_rn(ml1, mr1), __fadd_rn(ml2, mr2));
                }
                const float l1 = __shfl_up(x, 1, 64), r1 = __shfl_down(x, 1, 64);
                const float l2 = __shfl_up(x, 2, 64), r2 = __shfl_down(x, 2, 64);
                h0 = h1; h1 = h2; h2 = h3; h3 = h4;
                h4 = gauss_taps(x, __fadd_rn(l1, r1), __fadd_rn(l2, r2));
                if constexpr (!VALID) {
                    if (i >= 4 && out_col)
                        dst[fo + (size_t)(y0 + i - 4) * cols + gx] = gauss_taps(h2, __fadd_rn(h1, h3), __fadd_rn(h0, h4));
                } else if (i >= 4) {                           // wave-uniform
                    float num = gauss_taps(h2, __fadd_rn(h1, h3), __fadd_rn(h0, h4));
                    const float den = gauss_taps(k2, __fadd_rn(k1, k3), __fadd_rn(k0, k4));
                    if (__builtin_amdgcn_ballot_w64(out_col && den != 1.0f) != 0ull) num = __fdiv_rn(num, den);
                    float y = c0 >= thr ? num : c0;            // c0: the source row of this output row (a valid one has den >= 0.375^2)
                    if constexpr (INVERT) y = y >= thr ? __fsub_rn(max_depth, y) : y;
                    if (out_col) dst[fo + (size_t)(y0 + i - 4) * cols + gx] = y;
                }
            }
        }
    }
}

}  // namespace dcmt
