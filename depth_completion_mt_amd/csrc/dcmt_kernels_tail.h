// dcmt_kernels_tail.h -- k_tail: everything that follows k_fp_s / k_fp_q in a speculative (device entry point) call, as ONE launch
// with one workgroup per frame.
//
// k_fp_s / k_fp_q finish every frame whose holes H7 closes, which is every frame of ordinary data; what is left is rare and
// used to be five launches that read one word per workgroup and returned:
//   * a frame that k_fp_* left with holes (cnt[1] > 0) needs the hole-closure loop: H7 again from X6 into pp[0] (the redo, not
//     counted), applications 1 .. n_apps while the previous one left holes (pp[0] <-> pp[1], counted in cnt[1 + app]), then
//     H9..H11 from the last plane into dst -- k_fill_s (redo), k_fill_s x n_apps, k_post_s;
//   * a 16-bit attempt (k_pre_p<Q16OUT> -> k_fp_q) that raised its flag needs the f32 kernels: k_pre_p (still a launch of its
//     own, gated on the flag, in front of this one) and k_fp_s, which is the first phase here.
// The workgroup of a frame with nothing to do reads the flag and its counter and returns.  Otherwise its four waves walk the
// frame's strips phase by phase and meet at a barrier between phases.  A phase of a frame depends on nothing but that frame's
// earlier phases, so no workgroup ever waits for another one: no spinning on memory, no grid-wide barrier.
//
// The phases hand their planes to each other through global memory.  In front of every barrier stands a __threadfence(): it
// completes the wave's stores to pp[0] / pp[1] / dst and its counter atomics at the L2 and drops the lines this CU's vector
// cache holds, so that what the other waves of the workgroup read behind the barrier -- a plane written in this phase, at
// addresses this CU last read two phases ago -- comes from the L2 and not from a stale line.  Every load of a phase is followed
// by its own wave's fence before the barrier opens, so no line fetched before a plane was rewritten survives into the phase
// that reads it.  The counters are read with atomic loads for the same reason.  On this rare path the fences' cost is nothing.
#pragma once

#include "dcmt_kernels_fused.h"

namespace dcmt {

__device__ __forceinline__ int tail_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void tail_phase_end() { __threadfence(); __syncthreads(); }

// x6: the f32 X6 (table mode: tb, tbands).  x6q / q16_bad: nullptr, or the codes of the 16-bit attempt in front and its flag.
// While the flag is down the redo reads the codes; once it is raised the workgroup first reruns k_fp_s's body on the X6 the gated
// k_pre_p has just written (which also cleared the frame's counters), FILLED as the host chose it for k_fp_*.
// n_apps: loop applications allowed (min(spec_fill_iters, max_fill_iters) >= 1).
template <bool BLUR, bool FILLED>
__global__ __launch_bounds__(256)
void k_tail(const float* x6, const unsigned short* x6q, const int* q16_bad, float* pp0, float* pp1, float* dst, int* counters, int n_apps,
            int rows, int cols, int fstrips, int pstrips, float max_depth, float thr, const int* tb, int tbands)
{
    __shared__ float s_delay[4][16 * (64 + 64 + 32)];               // fp_s_unit's delay lines (the rerun only)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f = blockIdx.x;
    int* cnt = frame_counters(counters, f);
    const size_t fo = (size_t)f * rows * cols;
    // (the flag was settled by k_pre_p<Q16OUT>, two launches ago: every thread reads the same value)
    const bool rerun = q16_bad != nullptr && tail_load(q16_bad) != 0;
    if (rerun) {
        for (int strip = wave; strip < pstrips; strip += 4)
            fp_s_unit<BLUR, FILLED>(s_delay[wave], x6 + fo, dst + fo, cnt, rows, cols, f, strip, 0, lane, max_depth, thr, tb, tbands, 1);
        tail_phase_end();
    }
    if (tail_load(cnt + 1) == 0) return;                            // no holes left behind H7: k_fp_* has finished the frame (uniform: behind a barrier, or untouched since the last launch)
    // ---- H7 again, into pp[0]
    const bool q16 = x6q != nullptr && !rerun;
    for (int strip = wave; strip < fstrips; strip += 4)
        fill_strip(x6 + fo, pp0 + fo, cnt, rows, cols, f, strip, lane, thr, 0, 1, tb, tbands, x6q ? x6q + fo : nullptr, q16);
    tail_phase_end();
    // ---- H8: application a + 1 runs iff application a left holes (cnt[1 + a], complete behind the barrier; this phase adds to cnt[2 + a])
    int a = 0;
    while (a < n_apps && tail_load(cnt + 1 + a) > 0) {
        ++a;
        const float* in = ((a & 1) ? pp0 : pp1) + fo;
        float* out = ((a & 1) ? pp1 : pp0) + fo;
        for (int strip = wave; strip < fstrips; strip += 4)
            fill_strip(in, out, cnt, rows, cols, f, strip, lane, thr, a, 0, nullptr, 1, nullptr, false);
        tail_phase_end();
    }
    // ---- H9..H11 from the plane the last application wrote (a = apps_done(cnt, n_apps))
    const float* last = ((a & 1) ? pp1 : pp0) + fo;
    for (int strip = wave; strip < pstrips; strip += 4)
        post_strip<11, BLUR>(last, dst + fo, rows, cols, strip, lane, max_depth, thr);
}

}  // namespace dcmt
