// dcmt_dot_rn.h -- the f32 row-times-vector sums of the projection (N2) and the reprojection kernels, shared by both translation
// units: every product and every sum rounded once (__fmul_rn / __fadd_rn: no FMA contraction), sums left to right.  And the 16- / 8- /
// 4-byte accesses of their resolve and fix-up passes (load_words, store_words).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcmt {

// m[0]*x + m[1]*y + m[2]*z + m[3]   (a row of a 3x4 / 4x4 matrix times (x, y, z, 1): the product with 1 is exact)
__device__ __forceinline__ float dot4_rn(const float* m, float x, float y, float z)
{
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z)), m[3]);
}

// m[0]*x + m[1]*y + m[2]*z          (a row of a 3x3 matrix times (x, y, z))
__device__ __forceinline__ float dot3_rn(const float* m, float x, float y, float z)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z));
}

// PW = 4, 2 or 1 neighbouring dwords as one access of 4 * PW bytes, which p must be aligned to (plan::resolve_vec)
template <int PW>
__device__ __forceinline__ void load_words(const uint32_t* __restrict__ p, uint32_t (&w)[PW])
{
    if constexpr (PW == 4) { const uint4 v = *reinterpret_cast<const uint4*>(p); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
    else if constexpr (PW == 2) { const uint2 v = *reinterpret_cast<const uint2*>(p); w[0] = v.x; w[1] = v.y; }
    else w[0] = p[0];
}

template <int PW>
__device__ __forceinline__ void store_words(uint32_t* __restrict__ p, const uint32_t (&w)[PW])
{
    if constexpr (PW == 4) *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    else if constexpr (PW == 2) *reinterpret_cast<uint2*>(p) = make_uint2(w[0], w[1]);
    else p[0] = w[0];
}

}  // namespace dcmt
