// dcmt_cloud.h -- host-side launchers of the kernels in dcmt_kernels_cloud.h.  Those kernels are compiled in a translation unit
// of their own (dcmt_cloud.hip), so that adding them leaves the code object of the cascade's kernels (dcmt.hip) as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dcmt {

constexpr int kCloudWaves = 4;                  // waves per workgroup of k_cloud_count / k_cloud_scatter = slab entries per (frame, chunk)

struct CloudK { double fx, fy, cx, cy; };

// k_cloud_count -> k_cloud_scan -> k_cloud_scatter on st.  n = rows * cols; chunks = eval_chunks(n), groups = eval_chunk_groups(n)
// (dcmt_kernels_eval.h); slab: [batch][chunks][kCloudWaves] uint32; bgr may be null; capacity in records.
void launch_depth_to_cloud(const float* depth, const uint8_t* bgr, uint32_t n, uint32_t cols, uint32_t chunks, uint32_t groups,
                           uint32_t batch, const CloudK& k, uint32_t* slab, void* points, uint32_t capacity, int32_t* offsets,
                           hipStream_t st);
// k_gauss5 on st; src and dst must not overlap
void launch_gauss5(const float* src, float* dst, int rows, int cols, int batch, hipStream_t st);

// dcmt_reproject_params as the kernels of dcmt_kernels_reproject.h take it: the three rows of M that are used, the two rows of K
struct ReprojK { double fx, fy, cx, cy; float M[12]; float K[6]; };

// k_reproject_scatter -> k_reproject_resolve on st.  winner: the context's winner plane (batch * out_rows * out_cols tags at least);
// gen_tag, idx_bits: this call's generation and the plane's tag layout; depth and out must not overlap.
void launch_reproject(const float* depth, int rows, int cols, int batch, const ReprojK& k, unsigned* winner, unsigned gen_tag, int idx_bits,
                      float* out, int out_rows, int out_cols, hipStream_t st);

}  // namespace dcmt
