// dcmt_kernels_project.h -- the last-wins kernels of N2, compiled in dcmt.hip (the cascade's code object).  What they share with the
// nearest-wins kernels (dcmt_kernels_nearest.h, dcmt_cloud.hip) is in dcmt_project.h: ProjMats, ProjTable, project_point,
// point_depth, project_wg_frame, the record loaders, project_scatter_run and project_scatter_calib_run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "dcmt_dot_rn.h"
#include "dcmt_project.h"

namespace dcmt {

// ---------------------------------------------------------------------------------
// N2: LiDAR points -> sparse depth image (SL/main_sl.cpp:478-520).  Pass 1: one thread per point; the pixel's winner
// is the LAST point in file order = the largest point index (atomicMax on an int plane, -1 = empty).  Pass 2: one
// thread per pixel recomputes the winning point's depth (the same deterministic arithmetic) or writes 0.
// Every product and sum is rounded separately (__fmul_rn / __fadd_rn: no FMA contraction), sums left to right.
// ---------------------------------------------------------------------------------

// The winner plane holds TAGS: (generation << idx_bits) | global point index.  A call only looks at tags of its own generation, so
// the plane is not cleared between calls (one 0.48 GB memset per 256 sweeps less); the host clears it when the generations run out
// or a call needs more index bits than the plane's layout has.  Within a generation the larger tag is the larger point index =
// the later point in file order (a frame's points are contiguous), the reference's "last writer wins".
// ProjTable: the record of each point's OWN frame, project_scatter_calib_run (dcmt_project.h) storing the tag.  Measured 13 % behind
// the uniform call, all of it here.  A frame with a bad record scatters nothing: its part of the winner plane
// keeps no tag of this generation and the resolve writes zeros there.
template <typename MSrc = ProjMats>
__global__ __launch_bounds__(256)
void k_project_scatter(const float* __restrict__ pts, const int* __restrict__ offsets, int n_points, int batch,
                       MSrc geo, unsigned* __restrict__ winner, int rows, int cols, unsigned gen_tag)
{
    if constexpr (std::is_same_v<MSrc, ProjTable>)
        project_scatter_calib_run(pts, offsets, n_points, batch, geo.records, rows, cols,
                                  [&](size_t px, unsigned i, float) { atomicMax(&winner[px], gen_tag | i); });
    else
        project_scatter_run(pts, offsets, n_points, batch, geo, rows, cols, [&](int lo, int u, int v, int i, float) {
            atomicMax(&winner[((size_t)lo * rows + v) * cols + u], gen_tag | (unsigned)i);
        });
}

// One thread per PW neighbouring pixels of the whole batch (the tags hold global point indices, so a thread's pixels may lie in two
// frames): 8- / 16-byte accesses where the batch size and the buffers allow.  Most pixels have no point of this generation and are a
// zero; the winners' depths are recomputed from their points (the depth alone: the pixel is known, so the two divisions and the bounds
// test of the first pass are not repeated).
// ProjTable: the record of each pixel's OWN frame -- the winning point's frame is the frame of the pixel it won.  A wave's 64 * PW
// consecutive pixels lie in one frame almost always (a frame of 352 x 1216 has 1672 such runs, one of which holds its end): the
// frame of the wave's first pixel and that pixel's place in it are wave-uniform -- one division per wave, on the scalar unit -- and
// where the run ends inside the frame, that frame's record comes through the scalar cache once per wave and no lane divides.
// Otherwise each lane finds the frame of its first pixel (a 32-bit division) and each pixel that holds a winner gathers the 64 bytes
// point_depth reads from its own frame's record.  frame_px = rows * cols; the uniform instance does not read it.
template <int PW, typename MSrc = ProjMats>
__global__ __launch_bounds__(256)
void k_project_resolve(const float* __restrict__ pts, MSrc geo, const unsigned* __restrict__ winner, float* __restrict__ sparse,
                       size_t n_px, unsigned gen_tag, int idx_bits, uint32_t frame_px)
{
    constexpr bool kTable = std::is_same_v<MSrc, ProjTable>;
    const uint32_t l = threadIdx.x & 63;
    const size_t i_wave = (blockIdx.x * (size_t)256 + __builtin_amdgcn_readfirstlane(threadIdx.x & ~63u)) * PW;     // the wave's first pixel
    const size_t i = kTable ? i_wave + (size_t)l * PW : (blockIdx.x * (size_t)256 + threadIdx.x) * PW;
    if (i >= n_px) return;
    uint32_t w[PW], o[PW];
    load_words<PW>(winner + i, w);
    const unsigned mask = (1u << idx_bits) - 1u;
    uint32_t f_wave = 0, r_wave = 0;
    bool one_record = true;                                   // one record serves all of the wave's pixels
    if constexpr (kTable) {
        f_wave = (uint32_t)(i_wave / frame_px);                                   // i_wave < n_px here, so f_wave < batch
        r_wave = (uint32_t)(i_wave - (size_t)f_wave * frame_px);
        one_record = r_wave + 64u * PW <= frame_px;                               // (a frame has < 2^29 pixels: no overflow)
    }
    if (one_record) {
        [[maybe_unused]] ProjMats rec;
        if constexpr (kTable) load_project_depth_record(geo.records, f_wave, rec);
        const ProjMats& M = proj_m(geo, rec);
#pragma unroll
        for (int k = 0; k < PW; ++k) {
            o[k] = 0u;
            if ((w[k] & ~mask) == gen_tag) {
                const float4 p = *reinterpret_cast<const float4*>(pts + 4 * (size_t)(w[k] & mask));
                o[k] = __float_as_uint(point_depth(M, p.x, p.y, p.z));
            }
        }
    } else if constexpr (kTable) {
        uint32_t r = r_wave + l * PW;                                             // < frame_px + 256
        const uint32_t df = r / frame_px;
        uint32_t f = f_wave + df;                                                 // i < n_px, so f < batch, and so is every frame below:
        r -= df * frame_px;                                                       // i + PW <= n_px (the pixel count is a multiple of PW)
#pragma unroll
        for (int k = 0; k < PW; ++k) {
            if (k > 0 && ++r == frame_px) { r = 0; ++f; }
            o[k] = 0u;
            if ((w[k] & ~mask) == gen_tag) {
                ProjMats M;
                load_project_depth_record(geo.records, f, M);
                const float4 p = *reinterpret_cast<const float4*>(pts + 4 * (size_t)(w[k] & mask));
                o[k] = __float_as_uint(point_depth(M, p.x, p.y, p.z));
            }
        }
    }
    store_words<PW>(reinterpret_cast<uint32_t*>(sparse) + i, o);
}

}  // namespace dcmt
