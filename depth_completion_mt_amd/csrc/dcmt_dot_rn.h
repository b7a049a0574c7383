// dcmt_dot_rn.h -- the f32 row-times-vector sums of the projection (N2) and the reprojection kernels, shared by both translation
// units: every product and every sum rounded once (__fmul_rn / __fadd_rn: no FMA contraction), sums left to right.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace dcmt
