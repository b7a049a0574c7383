// dcmt_kernels_speckle.h -- the speckle filter of a 16-bit disparity map as include/dcmt.h states it (cv::filterSpeckles for CV_16S),
// batched on the device: the connected components of the live pixels (value != new_val) under the 4-neighbour EDGE relation
// |a - b| <= max_diff, and every pixel of a component of at most max_size pixels set to new_val.  Integer arithmetic throughout: the
// result is the same bits whatever the batch, the launch geometry or the run.
//
// The machinery is that of dcmt_kernels_connect.h (compiled beside it in dcmt_cloud.hip): its keys, conn_find / conn_unite in the
// plane A, the LDS union-find of a 64 x 16 tile, conn_count, and k_conn_flatten itself, which reads no pixel values and is launched
// as it is.  What differs is the relation.  "Equal labels" is transitive, an edge is not: the ramp 0, max_diff, 2 max_diff is one
// component whose ends are no edge.  So every shortcut of the label kernels that concludes "these two are already joined" from
// values alone has to be made from EDGES here:
//   k_spk_local   the left-neighbour union of pixel u is left out only where the three edges u-up, up-upleft and upleft-left all
//                 hold (then u and left are joined through them: u-up and upleft-left by the column chains, up-upleft by its own
//                 union or, by induction up the column, by this same argument).  [[-32, 32], [0, 0]] at max_diff 32 is the case
//                 that comparing each of the three with u's value gets wrong: the bottom pair must be united.
//   k_spk_border  the pair across a tile edge is left out only where the pair one step back along the edge lies in the same two
//                 tiles and pa-pa', pb-pb' and pa'-pb' are all edges (pa-pa', pb-pb' are joined inside their tiles; pa'-pb' by its
//                 own union or, by induction along the edge, by this argument).
// Differences are formed in 32 bits: -32768 against 32767 is 65535.  A pixel equal to new_val (and a pixel outside the frame) is DEAD:
// a singleton that joins nothing and counts nothing; its B word stays 0, so k_conn_flatten passes it by.
//
//   k_spk_local    one workgroup per tile: A[p] = the key of the smallest pixel of p's component within the tile, B[p] = that
//                  component's pixel count at that pixel, 0 elsewhere.
//   k_spk_border   one thread per pixel pair across a tile edge: conn_unite where the pair is an edge.
//   k_conn_flatten tile roots point at the root, tile counts are added into the root's word.
//   k_spk_apply    one thread per pixel (four where the planes' alignment allows): size = B[root]; out = size <= max_size ? new_val :
//                  the source value; depth = +0 where changed; the per-frame changed count summed per wave, one atomicAdd per wave.
//                  The only writer of out and depth; every thread reads its source pixels before it writes them and nobody else reads
//                  them: out may BE the source.
// No workgroup waits for another; every loop is one of dcmt_kernels_connect.h's (a strictly falling key, a cleared mask bit) or
// steps one pixel up a column.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcmt_kernels_connect.h"

namespace dcmt {

constexpr int32_t kSpkDead = 0x40000000;     // a tile's LDS value of a dead pixel: further than 65535 from every int16

// a, b: int16 values or kSpkDead; md in 0..65535.  The difference cannot wrap (|a - b| <= 2^30 + 32768); a dead pixel against a
// live one is further than md apart, so only "both dead" has to be excluded by name.
__device__ __forceinline__ bool spk_edge(int32_t a, int32_t b, int32_t md)
{
    const int32_t d = a - b;
    return a != kSpkDead && (d < 0 ? -d : d) <= md;
}

// grid (tiles_x * tiles_y, frames), 256 threads: lane = column of the tile, wave w its rows 4w .. 4w + 3
__global__ __launch_bounds__(256)
void k_spk_local(const int16_t* __restrict__ src, uint32_t rows, uint32_t cols, uint32_t tiles_x, uint32_t kbits, int32_t new_val, int32_t md,
                 uint32_t* __restrict__ A, uint32_t* __restrict__ B)
{
    __shared__ int32_t L[kConnLds];
    __shared__ uint32_t P[kConnLds];
    __shared__ uint32_t C[kConnLds];
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t x0 = tx * kConnTW, y0 = ty * kConnTH;
    const uint32_t lx = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t gx = x0 + lx;
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    int32_t v[4];
    bool in[4];
    uint32_t r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t ly = 4 * w + i, gy = y0 + ly, u = lx * kConnPad + ly;
        in[i] = gx < cols && gy < rows;
        v[i] = in[i] ? (int32_t)src[fo + (size_t)gy * cols + gx] : kSpkDead;
        if (v[i] == new_val) v[i] = kSpkDead;
        L[u] = v[i];
        C[u] = 0u;
    }
    __syncthreads();
    // a column's runs as chains: a pixel points at the pixel above it where the two are an edge ...
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t ly = 4 * w + i, u = lx * kConnPad + ly;
        P[u] = ly > 0 && spk_edge(v[i], L[u - 1], md) ? u - 1 : u;
    }
    __syncthreads();
    // ... and then at the head of its run: walked while nobody writes, stored behind the barrier
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t u = lx * kConnPad + 4 * w + i;
        for (;;) {                                         // ends: every step goes one pixel up the column
            const uint32_t p = P[u];
            if (p >= u) break;
            u = p;
        }
        r[i] = u;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) P[lx * kConnPad + 4 * w + i] = r[i];
    __syncthreads();
    // the runs of neighbouring columns
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t u = lx * kConnPad + 4 * w + i;
        if (lx == 0 || !spk_edge(v[i], L[u - kConnPad], md)) continue;
        // (not where u-up, up-upleft and upleft-left are edges: the two runs were joined there)
        if (4 * w + i > 0 && spk_edge(v[i], L[u - 1], md) && spk_edge(L[u - 1], L[u - kConnPad - 1], md) &&
            spk_edge(L[u - kConnPad - 1], L[u - kConnPad], md))
            continue;
        conn_lds_unite(P, u, u - kConnPad);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r[i] = conn_lds_find(P, lx * kConnPad + 4 * w + i);
        conn_count(C, r[i], v[i] != kSpkDead);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t ly = 4 * w + i, u = lx * kConnPad + ly;
        if (in[i]) {
            const uint32_t rx = r[i] / kConnPad, ry = r[i] - rx * kConnPad;
            const size_t p = fo + (size_t)(y0 + ly) * cols + gx;
            A[p] = conn_key(x0 + rx, y0 + ry, kbits);
            B[p] = r[i] == u ? C[u] : 0u;                  // (a dead pixel is its own root with a count of 0)
        }
    }
}

// grid (ceil(pairs / 256), frames), 256 threads.  The pairs of k_conn_border: j < pairs_v: edge j / rows between tile columns, row
// j % rows; the others: edge / cols between tile rows, column % cols
__global__ __launch_bounds__(256)
void k_spk_border(const int16_t* __restrict__ src, uint32_t rows, uint32_t cols, uint32_t pairs_v, uint32_t pairs, uint32_t kbits,
                  int32_t new_val, int32_t md, uint32_t* A)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= pairs) return;
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    uint32_t xa, ya, xb, yb;
    size_t back;                                           // the pair one step back along the edge, where it lies in the same two tiles (else 0)
    if (j < pairs_v) {
        const uint32_t e = j / rows;
        ya = yb = j - e * rows;
        xb = (e + 1) * kConnTW;
        xa = xb - 1;
        back = ya % kConnTH != 0 ? cols : 0;
    } else {
        const uint32_t jj = j - pairs_v, e = jj / cols;
        xa = xb = jj - e * cols;
        yb = (e + 1) * kConnTH;
        ya = yb - 1;
        back = xa % kConnTW != 0 ? 1 : 0;
    }
    const size_t pa = fo + (size_t)ya * cols + xa, pb = fo + (size_t)yb * cols + xb;
    const auto value = [&](size_t p) { const int32_t s = src[p]; return s == new_val ? kSpkDead : s; };
    const int32_t a = value(pa), b = value(pb);
    if (!spk_edge(a, b, md)) return;
    if (back != 0) {
        // pa-pa' and pb-pb' are joined inside their tiles, and pa'-pb' joins them across the edge
        const int32_t a1 = value(pa - back), b1 = value(pb - back);
        if (spk_edge(a, a1, md) && spk_edge(b, b1, md) && spk_edge(a1, b1, md)) return;
    }
    conn_unite(A + fo, conn_key(xa, ya, kbits), conn_key(xb, yb, kbits), kbits, cols);
}

// Behind k_conn_flatten.  grid (ceil(n / (256 * kPx)), frames), 256 threads, kPx pixels a thread.  kPx = 4: n a multiple of 4, src and
// out 8-byte aligned (the host decides).  src may be out: no __restrict__ on the two.
template <int kPx>
__global__ __launch_bounds__(256)
void k_spk_apply(const int16_t* src, const uint32_t* __restrict__ A, const uint32_t* __restrict__ B, uint32_t n, uint32_t cols, uint32_t kbits,
                 int32_t new_val, uint32_t max_size, int16_t* out, float* __restrict__ depth, uint32_t* __restrict__ removed)
{
    static_assert(kPx == 1 || kPx == 4, "one pixel, or four in one 8-byte access");
    const uint32_t p = (blockIdx.x * 256u + threadIdx.x) * (uint32_t)kPx;
    const size_t fo = (size_t)blockIdx.y * n;
    uint32_t changed = 0;
    if (p < n) {
        int16_t s[kPx];
        uint32_t t[kPx];
        if constexpr (kPx == 4) {
            const uint2 sv = *reinterpret_cast<const uint2*>(src + fo + p);
            const uint4 tv = *reinterpret_cast<const uint4*>(A + fo + p);
            s[0] = (int16_t)(sv.x & 0xffffu); s[1] = (int16_t)(sv.x >> 16); s[2] = (int16_t)(sv.y & 0xffffu); s[3] = (int16_t)(sv.y >> 16);
            t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
        } else {
            s[0] = src[fo + p];
            t[0] = A[fo + p];
        }
#pragma unroll
        for (int i = 0; i < kPx; ++i) {
            if ((int32_t)s[i] == new_val) continue;
            // A[p] is p's tile root or the root, and A of that is the root (conn_root); the root's B word is the component's size
            const uint32_t root = A[fo + conn_px(t[i], kbits, cols)];
            if (B[fo + conn_px(root, kbits, cols)] > max_size) continue;
            s[i] = (int16_t)new_val;
            if (depth) depth[fo + p + i] = 0.0f;
            ++changed;
        }
        if constexpr (kPx == 4) {
            uint2 o;
            o.x = (uint32_t)(uint16_t)s[0] | ((uint32_t)(uint16_t)s[1] << 16);
            o.y = (uint32_t)(uint16_t)s[2] | ((uint32_t)(uint16_t)s[3] << 16);
            *reinterpret_cast<uint2*>(out + fo + p) = o;
        } else {
            out[fo + p] = s[0];
        }
    }
    if (!removed) return;
    for (int m = 32; m >= 1; m >>= 1) changed += __shfl_xor(changed, m, 64);
    if ((threadIdx.x & 63) == 0 && changed != 0u) atomicAdd(removed + blockIdx.y, changed);
}

}  // namespace dcmt
