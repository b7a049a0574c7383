// dcmt_kernels_contour.h -- Slic::display_contours (DC_lidar_camera/slic.cpp:337-384, called at main_lc.cpp:214) and
// Slic::colour_with_cluster_means (slic.cpp:392-433) as include/dcmt.h states them, batched on the device.  Integer arithmetic
// throughout: the result is the same bits whatever the batch, the launch geometry or the run.
//
// Contours.  The reference's scan is column outer, row inner, and a pixel is taken iff at least two of its in-frame neighbours have
// another label and are not taken yet; only the four neighbours the scan has visited, (x-1, y-1), (x-1, y), (x-1, y+1) and (x, y-1),
// can be.  With c = the count over all neighbours but (x, y-1), taken(x, y) is the constant c >= 2 where (x, y-1) is outside the
// frame or has the same label or c != 1, and !taken(x, y-1) otherwise: a column is resolved without a scan, from the nearest
// constant pixel above each pixel and the parity of the distance to it.
//   k_cont_classify  one workgroup per tile of 64 x 64 pixels, labels read row-major with a halo of one into LDS: a code byte per
//                    pixel (dcmt_contour.h), written TRANSPOSED ([cols][rows]) through a second LDS tile, 64 consecutive bytes
//                    per wave store.  Everything that needs labels is in the code byte.
//   k_cont_walk      one wave per frame, lanes = 64 consecutive rows, the columns in order and a column's chunks of 64 rows in order:
//                    one step reads 64 consecutive code bytes (loaded kContAhead steps ahead: the steps are a chain, what binds is
//                    latency), takes the previous column's taken bits from LDS (one 64-bit mask per chunk, the neighbouring
//                    chunks' border bits shifted in), ballots the constant lanes and their constants, and each lane finds the
//                    nearest constant lane at or above its row with a leading-zero count; a run that reaches lane 0 starts from
//                    the last row of the chunk above.  Only that one bit is carried from step to step.  A byte per pixel out
//                    (255 / 0), transposed like the codes, every lane its own byte.
//   k_cont_paint     one workgroup per tile: the taken bytes back to row-major through LDS, d_mask written, the colour stored into
//                    d_bgr where the pixel is taken (no other byte of d_bgr is written).
// Cluster means.
//   k_means_clear    the sums to zero.
//   k_means_sum      one workgroup per tile of 64 x 64 pixels, a thread walks 16 rows of one column and adds up runs of equal labels in
//                    registers; a run goes to the tile's LDS table (labels [the tile's smallest, + kMeansSlots)) or, beyond it,
//                    straight to global memory with integer atomicAdd; the table's used slots are added to global memory at the
//                    end.  u32 sums: 255 * rows * cols < 2^32 is checked by the plan.  Integer adds commute: any order, same bits.
//   k_means_paint    one thread per pixel: sum / count per channel (integer division), labels outside [0, n_labels) left alone.
// Every word another workgroup may write in the same launch is only touched by atomicAdd in that launch (the sums in k_means_sum);
// no workgroup waits for another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcmt_contour.h"

namespace dcmt {

constexpr int kContHaloPitch = kContTile + 3;   // the label tile with its halo: 66 rows of 66 words, 67 apart
constexpr int kContBytePitch = kContTile + 4;   // byte tiles [column][row]: 32 consecutive columns on 32 banks

// grid (tiles_x * chunks, frames), 256 threads: tile column blockIdx.x % tiles_x, rows 64 * (blockIdx.x / tiles_x) ...
__global__ __launch_bounds__(256)
void k_cont_classify(const int32_t* __restrict__ labels, uint32_t rows, uint32_t cols, uint32_t tiles_x, uint8_t* __restrict__ codes)
{
    __shared__ int32_t L[(kContTile + 2) * kContHaloPitch];
    __shared__ uint8_t C[kContTile * kContBytePitch];
    constexpr int HP = kContHaloPitch, HW = kContTile + 2;
    const uint32_t k = blockIdx.x / tiles_x, tx = blockIdx.x - k * tiles_x;
    const uint32_t x0 = tx * kContTile, y0 = k * kContTile;
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(HW * HW); i += 256u) {
        const uint32_t r = i / HW, c = i - r * HW;
        const int64_t gy = (int64_t)y0 + r - 1, gx = (int64_t)x0 + c - 1;
        const bool in = gy >= 0 && gy < (int64_t)rows && gx >= 0 && gx < (int64_t)cols;
        L[r * HP + c] = in ? labels[fo + (size_t)gy * cols + (size_t)gx] : 0;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    {
        const uint32_t x = x0 + lane;
        const bool xm = x > 0, xp = x + 1 < cols;
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            const uint32_t ly = 16 * w + i, y = y0 + ly;
            const int32_t* p = L + (ly + 1) * HP + lane + 1;           // every offset below stays inside the halo tile
            const int32_t own = p[0];
            const bool ym = y > 0, yp = y + 1 < rows;
            auto differs = [&](int off, bool in) { return in && p[off] != own ? 1u : 0u; };
            const uint32_t later = differs(-HP + 1, xp && ym) + differs(1, xp) + differs(HP + 1, xp && yp) + differs(HP, yp);
            C[lane * kContBytePitch + ly] = (uint8_t)(later | differs(-HP - 1, xm && ym) * kCodeWestUp | differs(-1, xm) * kCodeWest |
                                                      differs(HP - 1, xm && yp) * kCodeWestDown | differs(-HP, ym) * kCodeNorth);
        }
    }
    __syncthreads();
    const uint32_t y = y0 + lane;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t cx = 4 * i + w, x = x0 + cx;
        if (x < cols && y < rows) codes[fo + (size_t)x * rows + y] = C[cx * kContBytePitch + lane];
    }
}

// grid (frames), 64 threads, chunks * 8 bytes of dynamic LDS.  codes, taken: [frames][cols][rows]
__global__ __launch_bounds__(64)
void k_cont_walk(const uint8_t* __restrict__ codes, uint8_t* __restrict__ taken, uint32_t rows, uint32_t cols, uint32_t chunks)
{
    extern __shared__ unsigned long long cont_prev[];      // [chunks]: the taken bits of the previous column (this column's, above the step)
    const uint32_t l = threadIdx.x;
    const size_t fo = (size_t)blockIdx.x * rows * cols;
    const uint8_t* __restrict__ code = codes + fo;
    uint8_t* __restrict__ out = taken + fo;
    for (uint32_t k = l; k < chunks; k += 64u) cont_prev[k] = 0ull;
    __syncthreads();

    uint32_t fx = 0, fk = 0;                               // the next step to load: column, chunk
    // its code byte of this lane, 0 below the frame.  The load is unconditional, from an address clamped into the frame (behind the
    // last step: the last column's, never used): loads under a branch make the compiler wait for ALL loads in flight at the first
    // use of one.
    auto fetch = [&]() -> uint32_t {
        const uint32_t y = 64u * fk + l;
        const uint32_t v = code[(size_t)min(fx, cols - 1u) * rows + min(y, rows - 1u)];
        if (++fk == chunks) { fk = 0; ++fx; }
        return y < rows ? v : 0u;
    };

    uint32_t x = 0, k = 0;
    unsigned long long north_west = 0ull;                  // bit 0: taken(x - 1, 64 k - 1)
    uint32_t carry = 0;                                    // taken(x, 64 k - 1)
    auto step = [&](uint32_t cb) {
        const uint32_t y = 64u * k + l;
        const unsigned long long pm = cont_prev[k];
        const unsigned long long pn = k + 1 < chunks ? cont_prev[k + 1] : 0ull;
        const unsigned long long up = (pm << 1) | north_west, down = (pm >> 1) | (pn << 63);
        const uint32_t t_up = (uint32_t)(up >> l) & 1u, t_mid = (uint32_t)(pm >> l) & 1u, t_down = (uint32_t)(down >> l) & 1u;
        const uint32_t c = (cb & kCodeLater) + ((cb >> 3) & ~t_up & 1u) + ((cb >> 4) & ~t_mid & 1u) + ((cb >> 5) & ~t_down & 1u);
        // a lane below the frame has cb = 0: constant, not taken
        const unsigned long long K = __ballot(c != 1u || !(cb & kCodeNorth)), V = __ballot(c >= 2u);
        const unsigned long long low = K & (~0ull >> (63u - l));       // the constant lanes at or above this row
        const uint32_t j = 63u - (uint32_t)__clzll((long long)(low | 1ull));
        const uint32_t t = low != 0ull ? ((uint32_t)(V >> j) ^ (l - j)) & 1u : (carry ^ (l + 1u)) & 1u;
        const unsigned long long T = __ballot(t != 0u);
        if (y < rows) out[(size_t)x * rows + y] = t ? (uint8_t)255 : (uint8_t)0;
        north_west = pm >> 63;
        if (l == 0) cont_prev[k] = T;                      // (every lane's read of it went into T)
        carry = (uint32_t)(T >> 63);
        if (++k == chunks) { k = 0; ++x; north_west = 0ull; carry = 0; }
        // one wave: lane 0's store is ordered in front of the next steps' loads by a wavefront-scope fence, which costs nothing.  (A
        // workgroup barrier here waits for every global load and store in flight, the loads ahead included: 2.11 ms instead of
        // 1.88 ms for 256 frames of 352 x 1216.)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };

    const uint32_t steps = cols * chunks;                  // below 2^31: the plan checks it
    uint32_t cur[kContAhead], nxt[kContAhead];
#pragma unroll
    for (int i = 0; i < kContAhead; ++i) cur[i] = fetch();
    uint32_t s0 = 0;
    for (; s0 + kContAhead <= steps; s0 += kContAhead) {   // ends: s0 grows
#pragma unroll
        for (int i = 0; i < kContAhead; ++i) nxt[i] = fetch();
#pragma unroll
        for (int i = 0; i < kContAhead; ++i) step(cur[i]);
#pragma unroll
        for (int i = 0; i < kContAhead; ++i) cur[i] = nxt[i];
    }
#pragma unroll
    for (int i = 0; i < kContAhead; ++i)
        if (s0 + i < steps) step(cur[i]);
}

// grid (tiles_x * chunks, frames), 256 threads.  mask and bgr: either may be null
__global__ __launch_bounds__(256)
void k_cont_paint(const uint8_t* __restrict__ taken, uint32_t rows, uint32_t cols, uint32_t tiles_x, uint8_t* __restrict__ mask,
                  uint8_t* __restrict__ bgr, uint32_t b, uint32_t g, uint32_t r)
{
    __shared__ uint8_t T[kContTile * kContBytePitch];
    const uint32_t k = blockIdx.x / tiles_x, tx = blockIdx.x - k * tiles_x;
    const uint32_t x0 = tx * kContTile, y0 = k * kContTile;
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t cx = 4 * i + w, x = x0 + cx, y = y0 + lane;
        T[cx * kContBytePitch + lane] = x < cols && y < rows ? taken[fo + (size_t)x * rows + y] : (uint8_t)0;
    }
    __syncthreads();
    const uint32_t x = x0 + lane;
    if (x >= cols) return;
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t ly = 16 * w + i, y = y0 + ly;
        if (y >= rows) break;
        const uint8_t t = T[lane * kContBytePitch + ly];
        const size_t p = fo + (size_t)y * cols + x;
        if (mask) mask[p] = t;
        if (bgr && t) {
            bgr[3 * p] = (uint8_t)b;
            bgr[3 * p + 1] = (uint8_t)g;
            bgr[3 * p + 2] = (uint8_t)r;
        }
    }
}

// grid (at most 4096), 256 threads
__global__ __launch_bounds__(256)
void k_means_clear(uint32_t* __restrict__ sums, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) sums[i] = 0u;
}

// sums[frame][label][4] += (b, g, r, n)
__device__ __forceinline__ void means_add(uint32_t* s, uint32_t b, uint32_t g, uint32_t r, uint32_t n)
{
    atomicAdd(s, b);
    atomicAdd(s + 1, g);
    atomicAdd(s + 2, r);
    atomicAdd(s + 3, n);
}

// grid (tiles_x * tiles_y, frames), 256 threads: lane = column of the tile, wave w its rows 16 w .. 16 w + 15
__global__ __launch_bounds__(256)
void k_means_sum(const int32_t* __restrict__ labels, const uint8_t* __restrict__ bgr, uint32_t rows, uint32_t cols, uint32_t tiles_x,
                 uint32_t n_labels, uint32_t* sums)
{
    __shared__ uint32_t S[kMeansSlots * 4];
    __shared__ uint32_t lowest;
    for (uint32_t i = threadIdx.x; i < (uint32_t)kMeansSlots * 4u; i += 256u) S[i] = 0u;
    if (threadIdx.x == 0) lowest = 0xffffffffu;
    __syncthreads();
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t x = tx * kContTile + (threadIdx.x & 63), y0 = ty * kContTile + kMeansRun * (threadIdx.x >> 6);
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    uint32_t* fs = sums + (size_t)blockIdx.y * n_labels * 4u;
    // a label outside [0, n_labels) reads as 0xffffffff here: never a slot, never counted
    uint32_t lab[kMeansRun], mn = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < kMeansRun; ++i) {
        const uint32_t y = y0 + i;
        const uint32_t v = x < cols && y < rows ? (uint32_t)labels[fo + (size_t)y * cols + x] : 0xffffffffu;
        lab[i] = v < n_labels ? v : 0xffffffffu;
        mn = min(mn, lab[i]);
    }
    for (int m = 32; m >= 1; m >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, m, 64));
    if ((threadIdx.x & 63) == 0) atomicMin(&lowest, mn);
    __syncthreads();
    const uint32_t base = lowest;
    uint32_t cur = 0xffffffffu, b = 0, g = 0, r = 0, n = 0;
    auto flush = [&]() {
        if (n == 0u) return;
        const uint32_t slot = cur - base;
        if (slot < (uint32_t)kMeansSlots) means_add(S + 4u * slot, b, g, r, n);
        else means_add(fs + 4u * (size_t)cur, b, g, r, n);
    };
#pragma unroll
    for (int i = 0; i < kMeansRun; ++i) {
        if (lab[i] != cur) {
            flush();
            cur = lab[i];
            b = g = r = n = 0u;
        }
        if (cur != 0xffffffffu) {
            const uint8_t* p = bgr + 3u * (fo + (size_t)(y0 + i) * cols + x);
            b += p[0];
            g += p[1];
            r += p[2];
            ++n;
        }
    }
    flush();
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < (uint32_t)kMeansSlots; s += 256u)
        if (S[4u * s + 3u] != 0u) means_add(fs + 4u * (size_t)(base + s), S[4u * s], S[4u * s + 1u], S[4u * s + 2u], S[4u * s + 3u]);
}

// grid (ceil(n / 256), frames), 256 threads
__global__ __launch_bounds__(256)
void k_means_paint(const int32_t* __restrict__ labels, uint32_t n, uint32_t n_labels, const uint32_t* __restrict__ sums, uint8_t* __restrict__ bgr)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const size_t i = (size_t)blockIdx.y * n + p;
    const uint32_t lab = (uint32_t)labels[i];
    if (lab >= n_labels) return;
    const uint32_t* __restrict__ s = sums + ((size_t)blockIdx.y * n_labels + lab) * 4u;
    const uint32_t count = s[3];                           // >= 1: this pixel is one of them
    bgr[3 * i] = (uint8_t)(s[0] / count);
    bgr[3 * i + 1] = (uint8_t)(s[1] / count);
    bgr[3 * i + 2] = (uint8_t)(s[2] / count);
}

}  // namespace dcmt
