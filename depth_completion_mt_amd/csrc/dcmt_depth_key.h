// dcmt_depth_key.h -- the integer key of the nearest-wins calls (dcmt_project_points_nearest*_dev, dcmt_reproject_depth_nearest*_dev,
// dcmt_kernels_nearest.h): a finite f32 as an unsigned integer whose order is the REVERSE of the float's, so that an integer
// atomicMax keeps the smallest float.  On bit patterns only (the library is built with -ffinite-math-only: no float compare here),
// for host and device code alike: tests/key_map_test.cpp walks it on a CPU.
//     ord(b) = b ^ 0x80000000   sign clear    the usual map of f32 bits to unsigned order, -0 below +0:
//              ~b               sign set       ord(-FLT_MAX) = 0x00800000 < ... < ord(-0) = 0x7fffffff < ord(+0) = 0x80000000 < ... < ord(FLT_MAX) = 0xff7fffff
//     key(b) = ~ord(b)                         0x00800000 (FLT_MAX) ... 0xff7fffff (-FLT_MAX): never 0 for a finite value, so 0 is "nothing landed"
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DCMT_KEY_FN __host__ __device__ inline
#else
#define DCMT_KEY_FN inline
#endif

namespace dcmt {

DCMT_KEY_FN uint32_t depth_ord(uint32_t bits) { return (bits >> 31) ? ~bits : bits ^ 0x80000000u; }

// larger key = smaller float
DCMT_KEY_FN uint32_t depth_key(uint32_t bits) { return ~depth_ord(bits); }

// the bits depth_key was given (key != 0: 0 is no key of a finite value)
DCMT_KEY_FN uint32_t depth_unkey(uint32_t key)
{
    const uint32_t ord = ~key;
    return (ord >> 31) ? ord ^ 0x80000000u : ~ord;
}

// what the fix-up pass stores: the winning value's bits, +0.0f where nothing landed
DCMT_KEY_FN uint32_t depth_key_to_bits(uint32_t key) { return key ? depth_unkey(key) : 0u; }

}  // namespace dcmt
