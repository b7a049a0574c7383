// dcmt_cloud.hip -- the kernels of dcmt_kernels_cloud.h and dcmt_kernels_reproject.h and their launchers (dcmt_cloud.h); the entry
// points that call them, dcmt_depth_to_cloud*, dcmt_gaussian5* and dcmt_reproject_depth*, are in dcmt.hip with every other entry point.
#include "dcmt_kernels_cloud.h"
#include "dcmt_kernels_reproject.h"

namespace dcmt {

void launch_depth_to_cloud(const float* depth, const uint8_t* bgr, uint32_t n, uint32_t cols, uint32_t chunks, uint32_t groups,
                           uint32_t batch, const CloudK& k, uint32_t* slab, void* points, uint32_t capacity, int32_t* offsets,
                           hipStream_t st)
{
    const dim3 grid(chunks, batch);
    const uint32_t per = chunks * kCloudWaves;
    hipLaunchKernelGGL(k_cloud_count, grid, dim3(kCloudThreads), 0, st, depth, n, groups, slab);
    hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(kCloudScanThreads), 0, st, slab, per * batch, per, batch, offsets);
    if (bgr)
        hipLaunchKernelGGL(k_cloud_scatter<true>, grid, dim3(kCloudThreads), 0, st, depth, bgr, n, groups, cols, k, slab,
                           reinterpret_cast<uint4*>(points), capacity);
    else
        hipLaunchKernelGGL(k_cloud_scatter<false>, grid, dim3(kCloudThreads), 0, st, depth, bgr, n, groups, cols, k, slab,
                           reinterpret_cast<uint4*>(points), capacity);
}

void launch_gauss5(const float* src, float* dst, int rows, int cols, int batch, hipStream_t st)
{
    const int strips = (cols + kGaussCols - 1) / kGaussCols;
    int band_rows = kGaussRows;                      // shorter bands while the call makes fewer than ~2 waves per SIMD
    while (band_rows > 8 && (size_t)strips * ((rows + band_rows - 1) / band_rows) * batch < 2048) band_rows /= 2;
    const int bands = (rows + band_rows - 1) / band_rows;
    hipLaunchKernelGGL(k_gauss5, dim3((unsigned)(((size_t)strips * bands + 3) / 4), batch), dim3(256), 0, st, src, dst, rows, cols, strips, bands,
                       band_rows);
}

void launch_reproject(const float* depth, int rows, int cols, int batch, const ReprojK& k, unsigned* winner, unsigned gen_tag, int idx_bits,
                      float* out, int out_rows, int out_cols, hipStream_t st)
{
    const uint32_t n = (uint32_t)rows * (uint32_t)cols, dst_n = (uint32_t)out_rows * (uint32_t)out_cols;
    const size_t n_px = (size_t)batch * dst_n;
    hipLaunchKernelGGL(k_reproject_scatter, dim3((n + kReprojectPxPerWg - 1) / kReprojectPxPerWg, batch), dim3(256), 0, st, depth, n,
                       (uint32_t)cols, k, winner, (uint32_t)out_rows, (uint32_t)out_cols, gen_tag);
    if (n_px % 4 == 0 && (uintptr_t)out % 16 == 0)
        hipLaunchKernelGGL(k_reproject_resolve<4>, dim3((unsigned)((n_px / 4 + 255) / 256)), dim3(256), 0, st, depth, n, (uint32_t)cols, k, winner,
                           out, dst_n, n_px, gen_tag, idx_bits);
    else if (n_px % 2 == 0 && (uintptr_t)out % 8 == 0)
        hipLaunchKernelGGL(k_reproject_resolve<2>, dim3((unsigned)((n_px / 2 + 255) / 256)), dim3(256), 0, st, depth, n, (uint32_t)cols, k, winner,
                           out, dst_n, n_px, gen_tag, idx_bits);
    else
        hipLaunchKernelGGL(k_reproject_resolve<1>, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, depth, n, (uint32_t)cols, k, winner,
                           out, dst_n, n_px, gen_tag, idx_bits);
}

}  // namespace dcmt
