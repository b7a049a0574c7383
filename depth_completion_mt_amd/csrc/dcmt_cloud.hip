// dcmt_cloud.hip -- the kernels of dcmt_kernels_cloud.h and their launchers (dcmt_cloud.h); the entry points that call them,
// dcmt_depth_to_cloud* and dcmt_gaussian5*, are in dcmt.hip with every other entry point.
#include "dcmt_kernels_cloud.h"

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

}  // namespace dcmt
