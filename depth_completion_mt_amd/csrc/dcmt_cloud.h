// dcmt_cloud.h -- what the kernels of dcmt_kernels_cloud.h / dcmt_kernels_reproject.h (compiled in dcmt_cloud.hip, a code object of
// their own) share with the host code that sizes their scratch and grids (dcmt_plan_side.h) and fills their arguments.  No HIP.
#pragma once

namespace dcmt {

constexpr int kCloudWaves = 4;                  // waves per workgroup of k_cloud_count / k_cloud_scatter = slab entries per (frame, chunk)
constexpr int kGaussCols = 60, kGaussRows = 32; // k_gauss5: output columns of a wave's strip, output rows of its band at most
constexpr int kBilCols = 60, kBilRows = 32;     // k_bilateral5 (dcmt_kernels_bilateral.h): the same, for its strips and bands
constexpr int kReprojectPxPerWg = 1024;         // k_reproject_scatter: 256 threads x 4 source pixels

struct CloudK { double fx, fy, cx, cy; };

// k_bilateral5's constants: gc = -0.5f / sigma_color^2 in f32; the spatial weights (float)exp(-d2 / (2 sigma_space^2)), in double, of
// the squared distances 1, 2 and 4 (bilateral_k)
struct BilK { float gc, ws1, ws2, ws4; };

// dcmt_reproject_params as the kernels of dcmt_kernels_reproject.h take it: the three rows of M that are used, the two rows of K
struct ReprojK { double fx, fy, cx, cy; float M[12]; float K[6]; };

}  // namespace dcmt
