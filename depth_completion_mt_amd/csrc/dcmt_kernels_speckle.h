// dcmt_kernels_speckle.h -- the speckle filter of a 16-bit disparity map as include/dcmt.h states it (cv::filterSpeckles for CV_16S),
// batched on the device: the connected components of the live pixels (value != new_val) under the 4-neighbour EDGE relation
// |a - b| <= max_diff, and every pixel of a component of at most max_size pixels set to new_val.  Integer arithmetic throughout: the
// result is the same bits whatever the batch, the launch geometry or the run.
//
// The labelling is that of dcmt_kernels_connect.h (compiled beside it in dcmt_cloud.hip): its tile-local and border stages under
// another relation, SpkRel, and k_conn_flatten itself, which reads no pixel values.  "Equal labels" is transitive, an edge here is
// not: the ramp 0, max_diff, 2 max_diff is one component whose ends are no edge, which is why the shared bodies take their
// shortcuts from edges alone.  Differences are formed in 32 bits: -32768 against 32767 is 65535.  A pixel equal to new_val is DEAD:
// it takes no part, and its word is further than max_diff from every live one's.
//
//   k_spk_local    one workgroup per tile: A[p] = the key of the smallest pixel of p's component within the tile, B[p] = that
//                  component's pixel count at that pixel, 0 elsewhere (a dead pixel: its own key, 0).
//   k_spk_border   one thread per pixel pair across a tile edge: conn_unite where the pair is an edge.
//   k_conn_flatten tile roots point at the root, tile counts are added into the root's word.
//   k_spk_apply    one thread per pixel (four where the planes' alignment allows): size = B[root]; out = size <= max_size ? new_val :
//                  the source value; depth = +0 where changed; the per-frame changed count summed per wave, one atomicAdd per wave.
//                  The only writer of out and depth; every thread reads its source pixels before it writes them and nobody else reads
//                  them: out may BE the source.
// No workgroup waits for another; every loop is one of dcmt_kernels_connect.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcmt_kernels_connect.h"

namespace dcmt {

constexpr int32_t kSpkDead = 0x40000000;     // the word of a dead pixel: further than 65535 from every int16

// a, b: int16 values or kSpkDead; md in 0..65535.  The difference cannot wrap (|a - b| <= 2^30 + 32768); a dead pixel against a
// live one is further than md apart, so only "both dead" has to be excluded by name.
__device__ __forceinline__ bool spk_edge(int32_t a, int32_t b, int32_t md)
{
    const int32_t d = a - b;
    return a != kSpkDead && (d < 0 ? -d : d) <= md;
}

struct SpkRel {                                            // both live and |a - b| <= md (dcmt_kernels_connect.h: a relation)
    using Src = int16_t;
    int32_t new_val, md;
    __device__ __forceinline__ int32_t word(int16_t s) const { return s == new_val ? kSpkDead : (int32_t)s; }
    __device__ __forceinline__ bool live(int32_t v) const { return v != kSpkDead; }
    __device__ __forceinline__ bool edge(int32_t a, int32_t b) const { return spk_edge(a, b, md); }
};

// conn_local_body under SpkRel; grid and threads as k_conn_local
__global__ __launch_bounds__(256)
void k_spk_local(const int16_t* __restrict__ src, uint32_t rows, uint32_t cols, uint32_t tiles_x, uint32_t kbits, int32_t new_val, int32_t md,
                 uint32_t* __restrict__ A, uint32_t* __restrict__ B)
{
    conn_local_body(SpkRel{new_val, md}, src, rows, cols, tiles_x, kbits, A, B);
}

// conn_border_body under SpkRel; grid, threads and pairs as k_conn_border
__global__ __launch_bounds__(256)
void k_spk_border(const int16_t* __restrict__ src, uint32_t rows, uint32_t cols, uint32_t pairs_v, uint32_t pairs, uint32_t kbits,
                  int32_t new_val, int32_t md, uint32_t* A)
{
    conn_border_body(SpkRel{new_val, md}, src, rows, cols, pairs_v, pairs, kbits, A);
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
