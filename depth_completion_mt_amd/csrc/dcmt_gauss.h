// dcmt_gauss.h -- the two helpers every 5x5 Gaussian of the library shares (H10 inside k_post_v1 / k_post_s / k_fp_*, and the
// unmasked k_gauss5 of dcmt_kernels_cloud.h, which is compiled in a translation unit of its own).
#pragma once
#include <hip/hip_runtime.h>

namespace dcmt {

// BORDER_REFLECT_101: gfedcb|abcdefgh|gfedcba
__device__ __forceinline__ int reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// One pass of the [1 4 6 4 1]/16 filter in the reference order  c*k0 + s1*k1 + s2*k2  (s1, s2 = the already rounded
// sums of the two neighbour pairs; every product rounded, the sum taken left to right).  k1 = 1/4 and k2 = 1/16 are
// powers of two, so those two products are exact and folding them into fused multiply-adds changes no rounding:
// round(a + exact(s*k)) is what the unfused sequence computes too.  (The one exception is a product that underflows
// into a subnormal and loses bits there, |s| < 2^-122 -- forty orders of magnitude below a depth in metres.)
__device__ __forceinline__ float gauss_taps(float c, float s1, float s2)
{
    return __builtin_fmaf(s2, 0.0625f, __builtin_fmaf(s1, 0.25f, __fmul_rn(c, 0.375f)));
}

}  // namespace dcmt
