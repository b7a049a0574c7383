// dcmt_chunks.h -- how a frame's flat pixel run is cut into chunks: the metrics, the colourisation's min/max pass and the point
// cloud all walk a frame this way, and the host sizes their slabs and grids with the same two functions.  No HIP: both code
// objects' kernel headers include it, and so do the host code and the CPU test of the plans (tests/plan_test.cpp).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define DCMT_HD __host__ __device__
#else
#define DCMT_HD
#endif

namespace dcmt {

constexpr int kEvalThreads = 256;
constexpr uint32_t kEvalGroupsPerChunk = 2048;       // 8192 pixels per workgroup: 53 chunks for a 352 x 1216 frame
constexpr uint32_t kEvalMaxChunks = 1024;

// a frame of n pixels is ceil(n / 4) groups of 4 consecutive pixels, in eval_chunks(n) chunks of eval_chunk_groups(n) groups
DCMT_HD inline uint32_t eval_chunks(uint32_t n)
{
    const uint32_t ng = (n + 3) / 4;
    const uint32_t c = (ng + kEvalGroupsPerChunk - 1) / kEvalGroupsPerChunk;
    return c < kEvalMaxChunks ? c : kEvalMaxChunks;
}
DCMT_HD inline uint32_t eval_chunk_groups(uint32_t n)
{
    const uint32_t ng = (n + 3) / 4, c = eval_chunks(n);
    return (ng + c - 1) / c;
}

}  // namespace dcmt
