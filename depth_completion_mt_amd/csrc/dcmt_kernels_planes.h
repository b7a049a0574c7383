// dcmt_kernels_planes.h -- the kernels of dcmt_superpixel_planes_dev (include/dcmt.h): one least-squares plane of inverse depth per
// superpixel through the returns that fall in it.  Compiled in dcmt_cloud.hip; the constants, the moment record and the fit itself
// are dcmt_planes.h's.
//   k_planes_clear   the moment records to their start: sums 0, minima 2^32 - 1, maxima 0.
//   k_planes_sum     one workgroup per tile of 64 x 64 pixels, a thread walks 16 rows of one column.  Only returns contribute: a
//                    return's nine integer terms and its six extremes go to the tile's LDS table (labels [the lowest label among
//                    the tile's returns, + kPlanesSlots)) or, beyond it, straight to the frame's records in global memory; the
//                    slots that were used are flushed with one set of global atomics each.  <true>: the refit pass, which counts a
//                    return only where its label's first fit is a plane and |w - w^| <= refit_tol * w^.
//   k_planes_solve   one lane per (frame, label): planes_fit on the record.  <true>: the refit, which replaces a plane by the
//                    trimmed plane where there is one.
//   k_planes_paint   VEC pixels per lane (4 with 16-byte loads and stores where the frame and the pointers allow it): the label's
//                    48-byte fit comes from L2, neighbouring pixels share it.
// Every word another workgroup may write in the same launch is only touched by atomics in that launch (the records in k_planes_sum):
// integer adds, minima and maxima commute, so the records do not depend on the order.  In place (out == depth): k_planes_paint is
// the only writer of out, and a lane reads its pixels before it writes them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dcmt.h"
#include "dcmt_planes.h"

namespace dcmt {

static_assert(sizeof(dcmt_plane_fit) == kPlanesFitBytes, "dcmt_plane_fit");

// grid (at most 4096), 256 threads; n 32-bit words
__global__ __launch_bounds__(256)
void k_planes_clear(uint32_t* __restrict__ mom, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) mom[i] = planes_clear_word((uint32_t)(i % (2u * kPlanesMomWords)));
}

// one return (or one LDS slot) into a record
__device__ __forceinline__ void planes_accumulate(unsigned long long* m, const PlaneMoments& q)
{
    atomicAdd(m, (unsigned long long)q.n);
    atomicAdd(m + 1, (unsigned long long)q.su);
    atomicAdd(m + 2, (unsigned long long)q.sv);
    atomicAdd(m + 3, (unsigned long long)q.suu);
    atomicAdd(m + 4, (unsigned long long)q.suv);
    atomicAdd(m + 5, (unsigned long long)q.svv);
    atomicAdd(m + 6, (unsigned long long)q.sw);
    atomicAdd(m + 7, (unsigned long long)q.suw);
    atomicAdd(m + 8, (unsigned long long)q.svw);
    uint32_t* e = reinterpret_cast<uint32_t*>(m + 9);
    atomicMin(e, q.umin);
    atomicMax(e + 1, q.umax);
    atomicMin(e + 2, q.vmin);
    atomicMax(e + 3, q.vmax);
    atomicMin(e + 4, q.wmin);
    atomicMax(e + 5, q.wmax);
}

// a depth's bits are a return's: finite, valid_thresh <= z <= max_depth.  Both bounds are positive finite floats, whose bits order as
// the numbers do; NaN, +-inf, negatives and -0.0 have bits above max_depth's.
__device__ __forceinline__ bool planes_is_return(uint32_t zb, uint32_t lo_bits, uint32_t hi_bits)
{
    return zb >= lo_bits && zb <= hi_bits;
}

// the code of a return: one correctly rounded f32 division, then round to nearest even (at most 2^20: exact)
__device__ __forceinline__ uint32_t planes_code(uint32_t zb)
{
    return __float2uint_rn(__fdiv_rn(kPlanesW, __uint_as_float(zb)));
}

// grid (tiles_x * tiles_y, frames), 256 threads: lane = column of the tile, wave w its rows 16 w .. 16 w + 15
template <bool REFIT>
__global__ __launch_bounds__(256)
void k_planes_sum(const uint32_t* __restrict__ depth, const int32_t* __restrict__ labels, uint32_t rows, uint32_t cols, uint32_t tiles_x,
                  uint32_t n_labels, uint32_t lo_bits, uint32_t hi_bits, const dcmt_plane_fit* __restrict__ fits, double tol,
                  unsigned long long* mom)
{
    __shared__ unsigned long long S[kPlanesSlots * kPlanesMomWords];
    __shared__ uint32_t lowest;
    uint32_t* S32 = reinterpret_cast<uint32_t*>(S);
    for (uint32_t i = threadIdx.x; i < (uint32_t)kPlanesSlots * 2u * kPlanesMomWords; i += 256u) S32[i] = planes_clear_word(i);
    if (threadIdx.x == 0) lowest = 0xffffffffu;
    __syncthreads();
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t x = tx * kPlanesTile + (threadIdx.x & 63), y0 = ty * kPlanesTile + kPlanesRun * (threadIdx.x >> 6);
    const size_t fo = (size_t)blockIdx.y * rows * cols;
    unsigned long long* fm = mom + (size_t)blockIdx.y * n_labels * kPlanesMomWords;
    const dcmt_plane_fit* ff = REFIT ? fits + (size_t)blockIdx.y * n_labels : nullptr;
    // a pixel that is no return reads as label 0xffffffff here: never a slot, never counted
    uint32_t lab[kPlanesRun], zb[kPlanesRun], mn = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < kPlanesRun; ++i) {
        const uint32_t y = y0 + i;
        const bool in = x < cols && y < rows;
        zb[i] = in ? depth[fo + (size_t)y * cols + x] : 0u;
        const bool ret = in && planes_is_return(zb[i], lo_bits, hi_bits);
        const uint32_t v = ret ? (uint32_t)labels[fo + (size_t)y * cols + x] : 0xffffffffu;
        lab[i] = v < n_labels ? v : 0xffffffffu;
        mn = min(mn, lab[i]);
    }
    for (int m = 32; m >= 1; m >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, m, 64));
    if ((threadIdx.x & 63) == 0) atomicMin(&lowest, mn);
    __syncthreads();
    const uint32_t base = lowest;
#pragma unroll
    for (int i = 0; i < kPlanesRun; ++i) {
        if (lab[i] == 0xffffffffu) continue;
        const uint32_t u = x, v = y0 + i, w = planes_code(zb[i]);
        if (REFIT) {
            const dcmt_plane_fit* f = ff + lab[i];
            if (f->kind != (uint32_t)kPlanesPlane) continue;
            const double what = planes_eval(f->a, f->b, f->c, u, v);
            if (!(fabs(planes_sub((double)w, what)) <= planes_mul(tol, what))) continue;
        }
        PlaneMoments q;
        q.n = 1u; q.su = u; q.sv = v;
        q.suu = (uint64_t)u * u; q.suv = (uint64_t)u * v; q.svv = (uint64_t)v * v;
        q.sw = w; q.suw = (uint64_t)u * w; q.svw = (uint64_t)v * w;
        q.umin = q.umax = u; q.vmin = q.vmax = v; q.wmin = q.wmax = w;
        const uint32_t slot = lab[i] - base;
        if (slot < (uint32_t)kPlanesSlots) planes_accumulate(S + (size_t)slot * kPlanesMomWords, q);
        else planes_accumulate(fm + (size_t)lab[i] * kPlanesMomWords, q);
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < (uint32_t)kPlanesSlots; s += 256u)
        if (S[(size_t)s * kPlanesMomWords] != 0u)                       // a used slot: base + s is the label of a return, below n_labels
            planes_accumulate(fm + (size_t)(base + s) * kPlanesMomWords, planes_load(S + (size_t)s * kPlanesMomWords));
}

// grid (ceil(count / 256)), 256 threads: count = frames * n_labels records
template <bool REFIT>
__global__ __launch_bounds__(256)
void k_planes_solve(const unsigned long long* __restrict__ mom, size_t count, uint32_t min_points, uint32_t min_extent, dcmt_plane_fit* fits)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    if (REFIT && fits[i].kind != (uint32_t)kPlanesPlane) return;
    const PlaneFit f = planes_fit(planes_load(mom + i * kPlanesMomWords), min_points, min_extent);
    if (REFIT) {
        if (f.kind != (uint32_t)kPlanesPlane) return;                   // the trimmed set is no plane: the first fit stands
        fits[i].a = f.a; fits[i].b = f.b; fits[i].c = f.c;
        fits[i].used = f.used; fits[i].wmin = f.wmin; fits[i].wmax = f.wmax;
        return;
    }
    dcmt_plane_fit o;
    o.a = f.a; o.b = f.b; o.c = f.c;
    o.seen = f.seen; o.used = f.used; o.wmin = f.wmin; o.wmax = f.wmax; o.kind = f.kind; o.reserved = 0u;
    fits[i] = o;
}

// one pixel's output bits
__device__ __forceinline__ uint32_t planes_pixel(uint32_t zb, int32_t label, uint32_t u, uint32_t v, uint32_t n_labels, uint32_t lo_bits,
                                                 uint32_t hi_bits, bool keep, const dcmt_plane_fit* __restrict__ ff)
{
    if ((uint32_t)label >= n_labels) return 0u;
    const dcmt_plane_fit* f = ff + (uint32_t)label;
    if (f->kind == (uint32_t)kPlanesNone) return 0u;
    if (keep && planes_is_return(zb, lo_bits, hi_bits)) return zb;
    double what = planes_eval(f->a, f->b, f->c, u, v);
    const double lo = (double)f->wmin, hi = (double)f->wmax;
    what = what < lo ? lo : (what > hi ? hi : what);
    return __float_as_uint((float)planes_div((double)kPlanesW, what));
}

// grid (ceil(n / VEC / 256), frames), 256 threads; n pixels a frame, a multiple of VEC
template <int VEC>
__global__ __launch_bounds__(256)
void k_planes_paint(const uint32_t* depth /* may be out */, const int32_t* __restrict__ labels, uint32_t n, uint32_t cols, uint32_t n_labels,
                    uint32_t lo_bits, uint32_t hi_bits, int keep, const dcmt_plane_fit* __restrict__ fits, uint32_t* out)
{
    const uint32_t p = (blockIdx.x * 256u + threadIdx.x) * (uint32_t)VEC;
    if (p >= n) return;
    const size_t i = (size_t)blockIdx.y * n + p;
    const dcmt_plane_fit* ff = fits + (size_t)blockIdx.y * n_labels;
    uint32_t v = p / cols, u = p - v * cols;
    if (VEC == 4) {
        const uint4 z = *reinterpret_cast<const uint4*>(depth + i);
        const int4 l = *reinterpret_cast<const int4*>(labels + i);
        const uint32_t zs[4] = {z.x, z.y, z.z, z.w};
        const int32_t ls[4] = {l.x, l.y, l.z, l.w};
        uint32_t o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = planes_pixel(zs[k], ls[k], u, v, n_labels, lo_bits, hi_bits, keep != 0, ff);
            if (++u == cols) { u = 0u; ++v; }
        }
        *reinterpret_cast<uint4*>(out + i) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        out[i] = planes_pixel(depth[i], labels[i], u, v, n_labels, lo_bits, hi_bits, keep != 0, ff);
    }
}

}  // namespace dcmt
