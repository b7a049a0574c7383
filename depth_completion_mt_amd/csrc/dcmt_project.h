// dcmt_project.h -- what the kernels of N2 (LiDAR points -> sparse depth image, SL/main_sl.cpp:478-520) share across the two code
// objects: the last-wins kernels k_project_* (dcmt_kernels_project.h, dcmt.hip) and the nearest-wins ones (dcmt_kernels_nearest.h,
// dcmt_cloud.hip) transform, accept and reject a point with the very same statements (project_scatter_run, project_scatter_calib_run),
// find a point's frame the same way and read a per-frame record (dcmt_project_calib, dcmt_calib.h; ProjTable) through the same
// loaders; only what is stored at the landing pixel differs.
// Every product and sum is rounded separately (__fmul_rn / __fadd_rn: no FMA contraction), sums left to right.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dcmt_calib.h"
#include "dcmt_dot_rn.h"

namespace dcmt {

struct ProjMats { float T[12]; float P[12]; };   // the three rows of T that are used; P

// the host's T (4x4) and P (3x4) as the kernels take them: the bottom row of T is never used (SL :483-485)
inline ProjMats proj_mats(const float* T, const float* P)
{
    ProjMats M;
    __builtin_memcpy(M.T, T, sizeof M.T);
    __builtin_memcpy(M.P, P, sizeof M.P);
    return M;
}

// dot4_rn: dcmt_dot_rn.h

// returns false if the point is dropped; otherwise pixel (u, v) and its depth
__device__ __forceinline__ bool project_point(const ProjMats& M, float x, float y, float z, int rows, int cols, int& u, int& v, float& depth)
{
    const float tx = dot4_rn(M.T, x, y, z), ty = dot4_rn(M.T + 4, x, y, z), tz = dot4_rn(M.T + 8, x, y, z);
    if (!(tz > 0.0f)) return false;                                   // SL :487
    const float px = dot4_rn(M.P, tx, ty, tz), py = dot4_rn(M.P + 4, tx, ty, tz), pz = dot4_rn(M.P + 8, tx, ty, tz);
    if (pz == 0.0f) return false;                                     // x/0 is +-inf or NaN: fails every bound below
    const float uf = __fdiv_rn(px, pz), vf = __fdiv_rn(py, pz);       // SL :502-503
    if (!(uf >= 0.0f && uf < (float)cols && vf >= 0.0f && vf < (float)rows)) return false;   // SL :506-507
    u = (int)uf; v = (int)vf; depth = pz;
    return true;
}

// depth of a point the first pass has already accepted: p.z of project_point, the same operations in the same order
__device__ __forceinline__ float point_depth(const ProjMats& M, float x, float y, float z)
{
    const float tx = dot4_rn(M.T, x, y, z), ty = dot4_rn(M.T + 4, x, y, z), tz = dot4_rn(M.T + 8, x, y, z);
    return dot4_rn(M.P + 8, tx, ty, tz);
}

// frame of the workgroup's first point i0: one search per workgroup (offsets[f] <= i0 < offsets[f+1]); a thread's own frame is that
// one or, where sweeps end inside the workgroup's 256 points, a later one.  0 <= result < batch whatever the offsets hold.  EVERY
// thread of the workgroup must call it (a barrier).
__device__ __forceinline__ int project_wg_frame(const int* __restrict__ offsets, int batch, int i0)
{
    __shared__ int s_lo;
    if (threadIdx.x == 0) {
        int lo = 0, hi = batch;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (offsets[mid] <= i0) lo = mid; else hi = mid; }
        s_lo = lo;
    }
    __syncthreads();
    return s_lo;
}

// The scatter with one pair of matrices for the whole batch, one point per thread of a 256-thread workgroup: the workgroup's frame
// search, the thread's own frame, the point's record, project_point.  store(frame, u, v, i, depth): what is done at the landing pixel
// (u, v) of that frame with the global point index i -- the store decides whether the bound is tested again in the integer domain
// before the address is formed (the nearest-wins rule does; the last-wins rule never did: DESIGN.md section 16).
template <typename Store>
__device__ __forceinline__ void project_scatter_run(const float* __restrict__ pts, const int* __restrict__ offsets, int n_points, int batch,
                                                    const ProjMats& M, int rows, int cols, Store store)
{
    const int i0 = blockIdx.x * 256;
    const int lo_wg = project_wg_frame(offsets, batch, i0);
    const int i = i0 + threadIdx.x;
    if (i >= n_points) return;
    int lo = lo_wg;
    while (lo + 1 < batch && offsets[lo + 1] <= i) ++lo;            // lo_wg <= lo < batch whatever the offsets hold
    const float4 p = *reinterpret_cast<const float4*>(pts + 4 * (size_t)i);       // x, y, z, reflectance (16-byte records)
    int u, v; float d;
    if (!project_point(M, p.x, p.y, p.z, rows, cols, u, v, d)) return;
    store(lo, u, v, i, d);
}

// ---- a table of per-frame matrices (dcmt_project_calib, dcmt_calib.h) ---------------------------------------------------------
// The matrices as the kernels' argument `geo`, the idiom of k_cloud_scatter (dcmt_kernels_cloud.h): ProjMats itself, by value
// (dcmt_project_points*_dev), or the table (dcmt_project_points*_calib_dev)
struct ProjTable { const dcmt_project_calib* __restrict__ records; };
__device__ __forceinline__ const ProjMats& proj_m(const ProjMats& arg, const ProjMats&) { return arg; }
__device__ __forceinline__ const ProjMats& proj_m(const ProjTable&, const ProjMats& rec) { return rec; }


// A record as ProjMats; `ok`: every one of its 24 entries is finite, tested on the bits
__device__ __forceinline__ bool load_project_record(const dcmt_project_calib* __restrict__ table, uint32_t f, ProjMats& M)
{
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(table) + kProjRecWords * (size_t)f;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) { const uint32_t b = w[i]; ok = ok && bits_finite32(b); M.T[i] = __uint_as_float(b); }
#pragma unroll
    for (int i = 0; i < 12; ++i) { const uint32_t b = w[12 + i]; ok = ok && bits_finite32(b); M.P[i] = __uint_as_float(b); }
    return ok;
}

// the same test by 24 lanes of a wave at once, a word each, and one ballot (on the scalar unit it takes some seventy instructions
// per wave, in a kernel that has about as many per wave in all).  EVERY lane of the wave must be active.
__device__ __forceinline__ bool project_record_ok_wave(const dcmt_project_calib* __restrict__ table, uint32_t f)
{
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(table) + kProjRecWords * (size_t)f;
    const uint32_t l = threadIdx.x & 63;
    return __ballot(l < kProjRecWords && !bits_finite32(w[l < kProjRecWords ? l : 0])) == 0;
}

// the whole record, untested
__device__ __forceinline__ void load_project_record_untested(const dcmt_project_calib* __restrict__ table, uint32_t f, ProjMats& M)
{
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(table) + kProjRecWords * (size_t)f;
#pragma unroll
    for (int i = 0; i < 12; ++i) M.T[i] = __uint_as_float(w[i]);
#pragma unroll
    for (int i = 0; i < 12; ++i) M.P[i] = __uint_as_float(w[12 + i]);
}

// what point_depth reads (T rows 0..2, P row 2), untested: a pixel with a tag of the call's generation lies in a frame whose record
// the scatter has accepted
__device__ __forceinline__ void load_project_depth_record(const dcmt_project_calib* __restrict__ table, uint32_t f, ProjMats& M)
{
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(table) + kProjRecWords * (size_t)f;
#pragma unroll
    for (int i = 0; i < 12; ++i) M.T[i] = __uint_as_float(w[i]);
#pragma unroll
    for (int i = 8; i < 12; ++i) M.P[i] = __uint_as_float(w[12 + i]);
}

// The scatter with the record of each point's OWN frame, one point per thread of a 256-thread workgroup.  A workgroup's 256 points
// span a sweep boundary wherever d_offsets says so (empty sweeps included), so the frame is the lane's.  The common case -- a sweep
// has some 120 000 points -- is a wave whose points all lie in the frame of the workgroup's first point: that frame's record is
// requested through the scalar cache as soon as the workgroup's search has found it, while the lanes' own offsets loads are in
// flight (the kernel is a chain of dependent loads), and tested by 24 lanes and one ballot; a second ballot asks whether every
// active lane of the wave stayed in that frame.  If so the wave runs the instruction stream of the uniform kernel on SGPRs.
// Otherwise (a wave behind a sweep boundary) each lane gathers and tests its own frame's 96 bytes.  A frame with a bad record
// scatters nothing.  store(pixel, i, depth): pixel = the landing pixel's index in the [batch][rows][cols] plane, i = the global
// point index; it is called only after the bound has held in the integer domain (below).
template <typename Store>
__device__ __forceinline__ void project_scatter_calib_run(const float* __restrict__ pts, const int* __restrict__ offsets, int n_points, int batch,
                                                          const dcmt_project_calib* __restrict__ table, int rows, int cols, Store store)
{
    const int i0 = blockIdx.x * 256;
    const int lo_wg = __builtin_amdgcn_readfirstlane(project_wg_frame(offsets, batch, i0));     // 0 <= lo_wg < batch whatever the offsets hold
    const bool ok_wg = project_record_ok_wave(table, (uint32_t)lo_wg);            // (every lane is still active here)
    const int i = i0 + threadIdx.x;
    if (i >= n_points) return;
    ProjMats M_wg;
    load_project_record_untested(table, (uint32_t)lo_wg, M_wg);
    int lo = lo_wg;
    while (lo + 1 < batch && offsets[lo + 1] <= i) ++lo;            // lo_wg <= lo < batch
    const float4 p = *reinterpret_cast<const float4*>(pts + 4 * (size_t)i);       // x, y, z, reflectance (16-byte records)
    const auto scatter = [&](const ProjMats& M) {
        int u, v; float d;
        if (!project_point(M, p.x, p.y, p.z, rows, cols, u, v, d)) return;
        // project_point's bounds are float compares, which -ffinite-math-only lets the compiler treat as if uf and vf were finite; a
        // record that is finite but huge makes them NaN.  The address is formed only after the bound has held in the integer domain
        if ((unsigned)u < (unsigned)cols && (unsigned)v < (unsigned)rows)
            store(((size_t)lo * rows + (unsigned)v) * cols + (unsigned)u, (unsigned)i, d);
    };
    if (__ballot(lo != lo_wg) == 0) {                               // (over the active lanes)
        if (ok_wg) scatter(M_wg);
    } else {
        ProjMats M;
        if (load_project_record(table, (uint32_t)lo, M)) scatter(M);
    }
}

}  // namespace dcmt
