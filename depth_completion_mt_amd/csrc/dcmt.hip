// dcmt.hip -- implementation of the C ABI in include/dcmt.h on gfx950 (MI355X).
//
// Host side of the hot path: context (device scratch owned per GPU) and launch sequencing of
// the kernels in dcmt_kernels_v1.h / dcmt_kernels_fused.h (and dcmt_kernels_local.h: the cascade without its extrapolation).  No PyTorch, no OpenCV, no CPU fallback: if there is no gfx950
// device every entry point fails with DCMT_E_NO_DEVICE / DCMT_E_HIP.
//
// The rest of the ABI is in two more translation units over dcmt_ctx.h (the context and the checks every entry point starts with):
// dcmt_cloud.hip (point cloud, unmasked Gaussian, reprojection: kernels and *_dev entry points) and dcmt_host.hip (every synchronous
// host entry point: the host<->device copies around a device call).  Host code may move between them; a kernel and the function that launches it stay
// where they are, in their order: both decide what the compiler emits for every other kernel of the code object.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <algorithm>
#include <new>
#include <type_traits>
#include <vector>

#include "dcmt.h"
#include "dcmt_plan.h"
#include "dcmt_plan_side.h"
#include "dcmt_ctx.h"
#include "dcmt_kernels_v1.h"
#include "dcmt_kernels_project.h"
#include "dcmt_kernels_fused.h"
#include "dcmt_kernels_pair.h"
#include "dcmt_kernels_fp_q16.h"
#include "dcmt_kernels_tail.h"
#include "dcmt_kernels_local.h"
#include "dcmt_kernels_slic.h"
#include "dcmt_kernels_eval.h"
#include "dcmt_kernels_color.h"
#include "dcmt_cloud.h"

using namespace dcmt;


namespace {

using plan::TH;
using plan::TW;
using plan::FTH_FEW;

// dcmt_plan.h restates what the kernel headers and dcmt.h own: every copy is checked here
static_assert(plan::kK0AsCompiled == K0_AS_COMPILED && plan::kK0Diamond == K0_DIAMOND, "k0 presets");
static_assert(plan::pre_p_vw(K0_AS_COMPILED, false) == PreP<K0_AS_COMPILED, false>::VW && plan::pre_p_vw(K0_DIAMOND, false) == PreP<K0_DIAMOND, false>::VW &&
              plan::pre_p_vw(K0_AS_COMPILED, true) == PreP<K0_AS_COMPILED, true>::VW && plan::pre_p_vw(K0_DIAMOND, true) == PreP<K0_DIAMOND, true>::VW, "PreP::VW");
static_assert(plan::pre_s_vw(K0_AS_COMPILED, false) == PreS<K0_AS_COMPILED, false>::VW && plan::pre_s_vw(K0_AS_COMPILED, true) == PreS<K0_AS_COMPILED, true>::VW &&
              plan::pre_s_vw(K0_DIAMOND, false) == PreS<K0_DIAMOND, false>::VW && plan::pre_s_vw(K0_DIAMOND, true) == PreS<K0_DIAMOND, true>::VW, "PreS::VW");
static_assert(plan::kFpQVW == FpQ::VW && plan::kPostSVW == PostS::VW && plan::kFillSVW == FillS::VW, "FpQ / PostS / FillS::VW");
static_assert(plan::kMaxBands == kMaxBands && plan::kLabelGroupMax == kLabelGroupMax, "kMaxBands, kLabelGroupMax");
static_assert(plan::kStageNormalize == DCMT_STAGE_NORMALIZE && plan::kStageClose5 == DCMT_STAGE_CLOSE5 && plan::kStageFill7 == DCMT_STAGE_FILL7 &&
              plan::kStageExtend == DCMT_STAGE_EXTEND && plan::kStageMedian5 == DCMT_STAGE_MEDIAN5 && plan::kStageBlur == DCMT_STAGE_BLUR &&
              plan::kStageFinal == DCMT_STAGE_FINAL, "dcmt_stage");
static_assert(plan::kFlagForceStaged == DCMT_FLAG_FORCE_STAGED && plan::kFlagForceFused == DCMT_FLAG_FORCE_FUSED &&
              plan::kFlagNormalize == DCMT_FLAG_NORMALIZE && plan::kFlagNoExtrapolate == DCMT_FLAG_NO_EXTRAPOLATE, "DCMT_FLAG_*");
static_assert(plan::local_vw(K0_AS_COMPILED) == LocalS<K0_AS_COMPILED>::VW && plan::local_vw(K0_DIAMOND) == LocalS<K0_DIAMOND>::VW &&
              plan::kLocalReach == LocalS<K0_AS_COMPILED>::REACH && plan::kLocalReach == LocalS<K0_DIAMOND>::REACH, "LocalS");
static_assert(plan::q16_params_ok(100.0f, 0.1f) && Q16::params_ok(100.0f, 0.1f) && !plan::q16_params_ok(80.0f, 0.1f) && !Q16::params_ok(80.0f, 0.1f) &&
              !plan::q16_params_ok(100.0f, 0.2f) && !Q16::params_ok(100.0f, 0.2f), "Q16::params_ok");
static_assert(sizeof(plan::Plan::path) == sizeof(dcmt_ctx::last_path), "dcmt_last_path");
static_assert(plan::kOk == DCMT_OK && plan::kInvalid == DCMT_E_INVALID, "dcmt_status");

uint32_t k0_bits(const uint8_t k0[25])
{
    uint32_t b = 0;
    for (int i = 0; i < 25; ++i) if (k0[i]) b |= 1u << i;
    return b;
}

// The label stage's bounding boxes, per (frame, label): two tables, grown on demand and together
int ensure_bbox(dcmt_ctx* ctx, size_t need, hipStream_t st)
{
    bool fresh = false;
    DCMT_TRY(ctx->bb_min.reserve(ctx, need, &fresh));
    DCMT_TRY(ctx->bb_max.reserve(ctx, need, &fresh));
    if (!fresh) return DCMT_OK;
    // "no box" everywhere, once: the label stage's waves put every entry they have read back into this state (a fill in front
    // of every call is two dependent operations with a bubble behind the previous call's last kernel each)
    DCMT_HIP(ctx, hipMemsetAsync(ctx->bb_min, 0x7f, sizeof(int) * ctx->bb_min.n, st));
    DCMT_HIP(ctx, hipMemsetAsync(ctx->bb_max, 0xff, sizeof(int) * ctx->bb_max.n, st));
    return DCMT_OK;
}

constexpr unsigned kQ16Flags = 64;

// The stateful part of the 16-bit dispatch, once per streaming call: a frame that is no multiple of 1/256 m costs the attempt AND the
// f32 rerun; once a call has raised the flag (seen here at the start of a later call, without synchronising) the next 63 calls go
// straight to the f32 kernels -- counted whether or not they would otherwise have made the attempt.
bool q16_allowed_now(dcmt_ctx* ctx)
{
    if (!ctx->knobs.fp_q16) return false;
    if (*(volatile int*)ctx->q16_seen) { *(volatile int*)ctx->q16_seen = 0; ctx->q16_skip = 63; }
    if (ctx->q16_skip > 0) { --ctx->q16_skip; return false; }
    return true;
}

dim3 tile_grid(int rows, int cols, int batch) { return dim3((cols + TW - 1) / TW, (rows + TH - 1) / TH, batch); }

int k0_preset(uint32_t kb)
{
    uint8_t k[25];
    dcmt_k0_as_compiled(k);
    if (kb == k0_bits(k)) return K0_AS_COMPILED;
    dcmt_k0_diamond(k);
    if (kb == k0_bits(k)) return K0_DIAMOND;
    return -1;
}

// with_value (dcmt_ctx.h): f(kind) with the k0 preset (a k0_preset result >= 0) as a compile-time constant, f(flag) with a bool,
// f(tile height) with the staged kernels' FTH_FEW or TH
template <typename F> void with_k0(int k0kind, F f) { with_value<(int)K0_AS_COMPILED, (int)K0_DIAMOND>(k0kind, f); }
template <typename F> void with_bool(bool b, F f) { with_value<true, false>(b, f); }
template <typename F> void with_tile_h(bool few, F f) { with_value<FTH_FEW, TH>(few ? FTH_FEW : TH, f); }

// The hole counters of the first `batch` frames, as they are once `st` has run dry, in ctx->h_counters
int read_counters(dcmt_ctx* ctx, hipStream_t st, int batch)
{
    DCMT_HIP(ctx, hipMemcpyAsync(ctx->h_counters, ctx->counters, sizeof(int) * (size_t)batch * kCntStride, hipMemcpyDeviceToHost, st));
    DCMT_HIP(ctx, hipStreamSynchronize(st));
    return DCMT_OK;
}

// The hole-closure loop shared by both paths.  `launch_app(i)` enqueues application i
// (reads pp[(i-1)&1], writes pp[i&1], skips frames without holes).  Returns the number of
// applications enqueued through *apps.
template <typename LaunchApp>
int fill_loop(dcmt_ctx* ctx, int batch, const dcmt_params* p, hipStream_t st, bool sync_loop, LaunchApp launch_app, int* apps_out)
{
    int rc = DCMT_OK, apps = 0;
    if (sync_loop) {
        // Iteration i of the reference's loop (LO :146-166) counts the holes left by application
        // i-1, fills them (application i: a no-op when there are none) and stops when it saw
        // none; the cap bounds i.
        for (int i = 1;; ++i) {
            DCMT_TRY(read_counters(ctx, st, batch));
            bool any = false;
            for (int f = 0; f < batch; ++f) {
                const int n_i = ctx->h_counters[(size_t)f * kCntStride + i];   // [1 + (i-1)]
                any |= n_i > 0;
                if (p->verbose) std::printf("%d\n", n_i);                       // LO :161
            }
            if (!any) break;
            launch_app(i);
            DCMT_HIP(ctx, hipGetLastError());
            apps = i;
            if (i >= p->max_fill_iters) { rc = DCMT_E_NOT_CONVERGED; break; }
        }
    } else {
        int n = p->spec_fill_iters;
        if (n > p->max_fill_iters) n = p->max_fill_iters;
        for (int i = 1; i <= n; ++i) launch_app(i);
        apps = n;
        DCMT_HIP(ctx, hipGetLastError());
    }
    *apps_out = apps;
    return rc;
}

// Every completion call starts here, once its scratch is there: the state dcmt_last_* report on, and dcmt_last_path
void begin_call(dcmt_ctx* ctx, hipStream_t st, int batch, const char* path)
{
    ctx->last_stream = st;
    ctx->last_batch = batch;
    ctx->last_apps_launched = 0;
    ctx->last_has_loop = 0;
    ctx->last_no_extrapolate = 0;
    std::memcpy(ctx->last_path, path, sizeof ctx->last_path);
}

// The streaming route of a plan.  Whole chain: k_pre_s -> k_fp_s -> k_tail, one workgroup per frame that returns at once for every
// frame k_fp_s finished and runs the hole-closure loop for the others (the host entry points, which read the counters back between
// applications, launch k_fill_s redo, k_fill_s loop applications, k_post_s only_if_holes instead).  stop_after probes:
// k_pre_s -> k_fill_s (-> loop) -> k_post_s / copy.  fr.labels: X4 is already in pp[0] (LC fast path): k_pre only runs H5 + H6 on it.
// fr.src16: uint16 ingest fused into k_pre.  pl.norm: N1's (a, b) per frame, applied while k_pre loads.  p: the call's parameters
// with the effective blur.
int launch_streaming(dcmt_ctx* ctx, const plan::Plan& pl, const Frames& fr, const dcmt_params* p, hipStream_t st, bool sync_loop)
{
    const int stop = p->stop_after, rows = fr.rows, cols = fr.cols, batch = fr.batch, xm = pl.xcd_map, bands = pl.bands;
    const bool q16 = pl.q16, filled = pl.filled, bl = p->blur == DCMT_BLUR_GAUSSIAN;
    float* dst = fr.dst;
    // (the hole counters are cleared by the first kernel of the chain: clear_frame_counters)
    auto stamp = [&](int i) { if (ctx->timing && ctx->tev[i]) (void)hipEventRecord(ctx->tev[i], st); };
    stamp(1);
    const size_t fe = (size_t)rows * cols;
    const dim3 b256(256);
    const float* d_x4 = fr.labels ? ctx->pp[0] : nullptr;
    const uint16_t* src16 = fr.src16;
    const float* cf = pl.norm && !d_x4 ? ctx->norm_coef : nullptr;     // (nullptr with d_x4 and with src16)
    float* x6 = ctx->x5;
    float* pp0 = ctx->pp[0];
    float* pp1 = ctx->pp[1];
    int* cnt = ctx->counters;
    int* tc = pl.table ? ctx->tb : nullptr;
    const void* in = src16 ? (const void*)src16 : d_x4 ? (const void*)d_x4 : (const void*)fr.src;
    float* o6 = stop == DCMT_STAGE_EXTEND && pl.out == plan::Out::DST ? dst : x6;

    const float scale = src16 ? fr.in_scale : 1.0f;
    // k_pre_s (one column per lane) into o6
    auto pre_s = [&](auto kind, auto wide_) {
        constexpr int KIND = decltype(kind)::value;
        constexpr bool WIDE = decltype(wide_)::value;
        auto* k = d_x4 ? k_pre_s<KIND, WIDE, true, false> : src16 ? k_pre_s<KIND, false, false, true> :
                  cf ? k_pre_s<KIND, WIDE, false, false, true> : k_pre_s<KIND, WIDE, false, false>;
        hipLaunchKernelGGL(k, dim3(pl.pre_grid), b256, 0, st, in, o6, rows, cols, pl.pre_strips, batch, xm, p->max_depth, p->valid_thresh,
                           scale, cf, tc, cnt);
    };
    // k_pre_p (two columns per lane) into o: X6 in f32, or as 16-bit codes (QOUT) that raise *qbad where a value has none and clear
    // *qclr; gate != nullptr: the launch returns at once unless *gate is raised.  (The 16-bit attempt never has cf.)
    auto pre_p = [&](auto kind, auto qout, float* o, int* qbad, const int* gate, int* qclr) {
        constexpr int KIND = decltype(kind)::value;
        constexpr bool QOUT = decltype(qout)::value;
        auto* k = d_x4 ? k_pre_p<KIND, true, false, false, QOUT> : src16 ? k_pre_p<KIND, false, true, false, QOUT> :
                  cf ? k_pre_p<KIND, false, false, true> : k_pre_p<KIND, false, false, false, QOUT>;
        hipLaunchKernelGGL(k, dim3(pl.pre_grid), b256, 0, st, in, o, rows, cols, pl.pre_strips, bands, batch, xm, p->max_depth,
                           p->valid_thresh, scale, cf, tc, cnt, qbad, gate, ctx->q16_seen_dev, qclr);
    };
    int* qbad = ctx->q16_bad;               // the flag of this call's 16-bit attempt
    if (q16 && pl.q16_own_flag) {
        // a captured call: every replay clears the captured calls' flag itself and leaves the ring, which only the host can move round, alone
        qbad = ctx->q16_bad + kQ16Flags;
        DCMT_HIP(ctx, hipMemsetAsync(qbad, 0, sizeof(int), st));
        with_k0(pl.k0kind, [&](auto kind) { pre_p(kind, std::true_type{}, reinterpret_cast<float*>(ctx->x6q.p), qbad, nullptr, nullptr); });
    } else if (q16) {
        // this attempt's flag (cleared by the previous attempt's kernel, or by dcmt_create) and the next one's, which this attempt's kernel clears
        qbad = ctx->q16_bad + ctx->q16_attempts % kQ16Flags;
        int* qnext = ctx->q16_bad + (ctx->q16_attempts + 1) % kQ16Flags;
        ++ctx->q16_attempts;
        with_k0(pl.k0kind, [&](auto kind) { pre_p(kind, std::true_type{}, reinterpret_cast<float*>(ctx->x6q.p), qbad, nullptr, qnext); });
    } else if (pl.pair) {
        with_k0(pl.k0kind, [&](auto kind) { pre_p(kind, std::false_type{}, o6, nullptr, nullptr, nullptr); });
    } else {
        with_k0(pl.k0kind, [&](auto kind) { if (pl.wide) pre_s(kind, std::true_type{}); else pre_s(kind, std::false_type{}); });
    }
    DCMT_HIP(ctx, hipGetLastError());
    stamp(2);
    if (stop == DCMT_STAGE_EXTEND) {
        if (o6 != dst) DCMT_HIP(ctx, hipMemcpyAsync(dst, o6, sizeof(float) * (size_t)batch * fe, hipMemcpyDeviceToDevice, st));
        return DCMT_OK;
    }

    const int fstrips = pl.fill_strips, pstrips = pl.post_strips;
    const dim3 fgrid(pl.fill_grid);
    // the hole-closure loop's applications 1, 2, ... (pp[0] <-> pp[1])
    auto fill_apps = [&](int* apps) {
        return fill_loop(ctx, batch, p, st, sync_loop, [&](int i) {
            hipLaunchKernelGGL(k_fill_s, fgrid, b256, 0, st, (i & 1) ? pp0 : pp1, (i & 1) ? pp1 : pp0, cnt, rows, cols,
                               fstrips, batch, xm, p->valid_thresh, i, 0, (const int*)nullptr, 1, (const unsigned short*)nullptr, (const int*)nullptr);
        }, apps);
    };
    if (pl.fuse_fp) {
        // one kernel for H7..H11 (k_fp_s deals (frame, strip, band) units to waves in one flat sequence, per XCD with the XCD map: no
        // half-empty workgroups); frames it leaves with holes are redone by the unfused kernels below
        const int n_redo = pl.n_redo;
        if (q16) {
            auto* fpq = filled ? k_fp_q<true, true> : bl ? k_fp_q<true, false> : k_fp_q<false, false>;
            hipLaunchKernelGGL(fpq, dim3(pl.fp_q_grid), b256, 0, st, (const void*)ctx->x6q, dst, cnt, rows, cols, pl.q_strips, batch, xm,
                               p->max_depth, p->valid_thresh, (const int*)tc, bands);
            // frames that are no multiples of 1/256 m: both f32 kernels again, gated on the flag the attempt raised (k_pre_p returns at once
            // otherwise; k_fp_s is k_tail's first phase, or a gated launch where no k_tail follows)
            // (the uint16 entry point too: a payload beyond 30719 = 119.996 m has no code)
            with_k0(pl.k0kind, [&](auto kind) { pre_p(kind, std::false_type{}, x6, nullptr, qbad, nullptr); });
        }
        if (pl.fp_s_launch) {
            auto* fps = filled ? k_fp_s<true, true> : bl ? k_fp_s<true> : k_fp_s<false>;
            hipLaunchKernelGGL(fps, dim3(pl.fp_s_grid), b256, 0, st, x6, dst, cnt, rows, cols, pstrips, batch, xm, p->max_depth,
                               p->valid_thresh, (const int*)tc, bands, q16 ? (const int*)qbad : (const int*)nullptr, pl.fb_s);
        }
        DCMT_HIP(ctx, hipGetLastError());
        stamp(3);
        ctx->last_has_loop = 1;
        int rc = DCMT_OK, apps = 0;
        if (pl.tail) {
            auto* kt = filled ? k_tail<true, true> : bl ? k_tail<true, false> : k_tail<false, false>;
            hipLaunchKernelGGL(kt, dim3(batch), b256, 0, st, (const float*)x6, q16 ? (const unsigned short*)ctx->x6q : (const unsigned short*)nullptr,
                               q16 ? (const int*)qbad : (const int*)nullptr, pp0, pp1, dst, cnt, n_redo, rows, cols, fstrips, pstrips, p->max_depth,
                               p->valid_thresh, (const int*)tc, bands);
            DCMT_HIP(ctx, hipGetLastError());
            apps = n_redo;
        } else if (n_redo > 0) {
            {                     // host entry points: look before launching anything else
                DCMT_TRY(read_counters(ctx, st, batch));
                bool any = false;
                for (int f = 0; f < batch; ++f) any |= ctx->h_counters[(size_t)f * kCntStride + 1] > 0;
                if (!any) { if (p->verbose) for (int f = 0; f < batch; ++f) std::printf("0\n"); return DCMT_OK; }
            }
            hipLaunchKernelGGL(k_fill_s, fgrid, b256, 0, st, x6, pp0, cnt, rows, cols, fstrips, batch, xm, p->valid_thresh, 0, 1, (const int*)tc, bands,
                               q16 ? (const unsigned short*)ctx->x6q : (const unsigned short*)nullptr, (const int*)qbad);
            rc = fill_apps(&apps);
            if (rc != DCMT_OK && rc != DCMT_E_NOT_CONVERGED) return rc;
            hipLaunchKernelGGL((bl ? k_post_s<11, true> : k_post_s<11, false>), dim3(pl.post_grid), b256, 0, st, pp0, pp1, dst, cnt, apps,
                               rows, cols, pstrips, batch, xm, p->max_depth, p->valid_thresh, 1);
            DCMT_HIP(ctx, hipGetLastError());
        }
        stamp(4);
        ctx->tev_valid = ctx->timing;
        ctx->last_apps_launched = apps;
        return rc;
    }
    hipLaunchKernelGGL(k_fill_s, fgrid, b256, 0, st, x6, stop == DCMT_STAGE_FILL31 ? dst : pp0, cnt, rows, cols,
                       fstrips, batch, xm, p->valid_thresh, 0, 0, (const int*)nullptr, 1, (const unsigned short*)nullptr, (const int*)nullptr);
    DCMT_HIP(ctx, hipGetLastError());
    if (stop == DCMT_STAGE_FILL31) return DCMT_OK;

    ctx->last_has_loop = 1;
    int apps = 0;
    const int rc = fill_apps(&apps);
    if (rc != DCMT_OK && rc != DCMT_E_NOT_CONVERGED) return rc;
    if (stop <= DCMT_STAGE_FILLLOOP) {
        hipLaunchKernelGGL((k_post_v1<TH, TW>), tile_grid(rows, cols, batch), dim3(kThreads), 0, st, pp0, pp1, dst, cnt, apps,
                           rows, cols, p->max_depth, p->valid_thresh, p->blur, 8);
    } else {
        auto* post = stop == DCMT_STAGE_MEDIAN5 ? k_post_s<9, false> : stop == DCMT_STAGE_BLUR ? (bl ? k_post_s<10, true> : k_post_s<10, false>) :
                     (bl ? k_post_s<11, true> : k_post_s<11, false>);
        hipLaunchKernelGGL(post, dim3(pl.post_grid), b256, 0, st, pp0, pp1, dst, cnt, apps, rows, cols, pstrips, batch, xm,
                           p->max_depth, p->valid_thresh, 0);
    }
    DCMT_HIP(ctx, hipGetLastError());
    ctx->last_apps_launched = apps;
    return rc;
}

// the scratch plane (or dst) a plan points the output of the kernel that reads the frames at
float* out_plane(const dcmt_ctx* ctx, plan::Out o, float* dst) { return o == plan::Out::DST ? dst : o == plan::Out::X5 ? ctx->x5 : ctx->pp[0]; }

int run_plan(dcmt_ctx* ctx, const plan::Plan& pl, const Frames& fr, const dcmt_params* p, int blur, hipStream_t st, bool sync_loop);
int launch_local(dcmt_ctx* ctx, const plan::Plan& pl, const Frames& fr, const dcmt_params* p, int blur, hipStream_t st);

// the cascade's literals of the bilateral finish (img_completion.cpp:174); fixed: dcmt_params has no room for them
constexpr float kBilateralSigmaColor = 1.5f, kBilateralSigmaSpace = 2.0f;

// Plans the call (dcmt_plan.h), allocates what the plan names, then enqueues the cascade on `st`.  sync_loop: run the hole-closure
// loop exactly as the reference would, reading the hole counters back between applications (host entry points); otherwise enqueue
// p->spec_fill_iters applications speculatively.
int run_chain(dcmt_ctx* ctx, const Frames& fr, const dcmt_params* p, bool force_gaussian, hipStream_t st, bool sync_loop)
{
    const int rows = fr.rows, cols = fr.cols, batch = fr.batch, stop = p->stop_after;
    const uint32_t kb = k0_bits(p->k0);
    // (the labeled entry points force the reference's Gaussian, except for this project's own opt-in)
    const int blur = force_gaussian && p->blur != DCMT_BLUR_GAUSSIAN_VALID ? (int)DCMT_BLUR_GAUSSIAN : p->blur;
    // A call whose stream is being captured into a graph (dcmt.h, "Graph capture") runs later, on every replay: events recorded or
    // lines printed once, now, would mean nothing then -- refused before anything is enqueued
    const bool capturing = !sync_loop && stream_capturing(st);
    if (capturing && (ctx->timing || p->verbose)) return DCMT_E_INVALID;
    ctx->tev_valid = 0;
    if ((p->flags & DCMT_FLAG_NORMALIZE) && fr.src16) return DCMT_E_UNSUPPORTED;
    plan::Call c;
    c.rows = rows; c.cols = cols; c.batch = batch;
    c.input = fr.labels ? plan::Input::LABELED : fr.src16 ? plan::Input::U16 : plan::Input::F32;
    c.n_labels = fr.n_labels;
    c.src = fr.src16 ? (uintptr_t)fr.src16 : (uintptr_t)fr.src; c.dst = (uintptr_t)fr.dst; c.labels = (uintptr_t)fr.labels;
    c.in_scale = fr.in_scale;
    c.max_depth = p->max_depth; c.valid_thresh = p->valid_thresh;
    c.k0kind = k0_preset(kb);
    c.gaussian = blur == DCMT_BLUR_GAUSSIAN;
    c.bilateral = blur == DCMT_BLUR_BILATERAL_CLONE;
    c.valid = blur == DCMT_BLUR_GAUSSIAN_VALID;
    c.max_fill_iters = p->max_fill_iters; c.spec_fill_iters = p->spec_fill_iters; c.stop_after = stop; c.flags = p->flags;
    c.sync_loop = sync_loop;
    // The context's skip state is the eager calls': a captured call neither reads nor advances it (what it decided now would hold for
    // every replay).  It makes the attempt wherever the plan allows one, on the flag the captured calls have to themselves
    c.capturing = capturing;
    c.q16_allowed = plan::route_of(ctx->knobs, c) == plan::Route::STREAMING && (capturing ? ctx->knobs.fp_q16 != 0 : q16_allowed_now(ctx));
    const plan::Plan pl = plan::plan_call(ctx->knobs, c);
    if (!pl.bilateral && !pl.gauss_valid) return run_plan(ctx, pl, fr, p, blur, st, sync_loop);

    // The bilateral finish: the plan's chain up to the median into the context's median plane (allocated by the first such call,
    // before anything is enqueued), then k_bilateral5 from there into dst.  A loop that hit max_fill_iters is filtered like any other.
    // The Gaussian that ignores holes with the extrapolation: the same, with k_gauss5<VALID> -- where the loop hit max_fill_iters
    // it is what keeps the holes that are left out of their neighbours.
    DCMT_TRY(ctx->median.reserve(ctx, ctx->frame_elems * (size_t)ctx->max_batch));
    Frames fm = fr;
    fm.dst = ctx->median;
    dcmt_params q = *p;
    q.stop_after = DCMT_STAGE_MEDIAN5;
    const int rc = run_plan(ctx, pl, fm, &q, DCMT_BLUR_NONE, st, sync_loop);
    if (rc != DCMT_OK && rc != DCMT_E_NOT_CONVERGED) return rc;
    if (pl.gauss_valid)
        DCMT_TRY(gauss5_valid_enqueue(ctx, ctx->median, fr.dst, rows, cols, batch, p->valid_thresh, pl.gauss_valid_invert, p->max_depth, st));
    else
    DCMT_TRY(bilateral5_enqueue(ctx, ctx->median, fr.dst, rows, cols, batch, kBilateralSigmaColor, kBilateralSigmaSpace, pl.bilateral_invert,
                                p->max_depth, p->valid_thresh, st));
    return rc;
}

// The rest of run_chain: allocates what the plan names, then enqueues its kernels.  blur: the effective one.
int run_plan(dcmt_ctx* ctx, const plan::Plan& pl, const Frames& fr, const dcmt_params* p, int blur, hipStream_t st, bool sync_loop)
{
    const int rows = fr.rows, cols = fr.cols, batch = fr.batch, stop = p->stop_after;
    const uint32_t kb = k0_bits(p->k0);

    // Scratch only one of the paths uses is allocated by the first call whose plan names it (never again afterwards) -- before anything
    // of the call is enqueued: an allocation synchronises, and one that fails must not leave half a call in the stream.  The 16-bit
    // plane of k_pre_p<Q16OUT> -> k_fp_q (and 16 bytes of slack), the column statistics of the staged tile kernels, the label stage's
    // bounding boxes.
    if (pl.needs_x6q) DCMT_TRY(ctx->x6q.reserve(ctx, ctx->frame_elems * (size_t)ctx->max_batch + 16 / sizeof(unsigned short)));
    if (pl.needs_colstat) DCMT_TRY(ctx->colstat.reserve(ctx, 2 * (size_t)ctx->max_cols * ((ctx->max_rows + FTH_FEW - 1) / FTH_FEW) * ctx->max_batch));
    if (pl.needs_bbox) DCMT_TRY(ensure_bbox(ctx, (size_t)batch * fr.n_labels * 2, st));
    begin_call(ctx, st, batch, pl.path);
    ctx->last_no_extrapolate = pl.no_extrapolate;
    if (ctx->timing && ctx->tev[0]) (void)hipEventRecord(ctx->tev[0], st);

    const size_t n_px = (size_t)batch * rows * cols;
    const float* d_src = fr.src;
    float* d_dst = fr.dst;
    float* out = out_plane(ctx, pl.out, d_dst);     // an overlapping call's probe: scratch, then one copy (the plan says why that plane is free)
    const float* coef = nullptr;
    if (pl.norm) {
        // N1: one read-only pass for the per-frame extrema, then (a, b) per frame; the first kernel of whichever
        // path runs below applies them while it loads
        const size_t fe = (size_t)rows * cols;
        // (norm_stats is all zero here: dcmt_create cleared it, k_norm_coef clears what it has read)
        hipLaunchKernelGGL(k_minmax, dim3(kMinmaxUnits * batch), dim3(256), 0, st, d_src, ctx->norm_stats, fe, batch, pl.xcd_map);
        hipLaunchKernelGGL(k_norm_coef, dim3((batch + 63) / 64), dim3(64), 0, st, ctx->norm_stats, ctx->norm_coef, batch, p->norm_lo, p->norm_hi);
        DCMT_HIP(ctx, hipGetLastError());
        coef = ctx->norm_coef;
        if (pl.route == plan::Route::NORMALIZE_ONLY) {
            hipLaunchKernelGGL(k_norm_write, dim3(2048), dim3(256), 0, st, d_src, out, coef, fe, batch);
            DCMT_HIP(ctx, hipGetLastError());
            if (out != d_dst) DCMT_HIP(ctx, hipMemcpyAsync(d_dst, out, sizeof(float) * n_px, hipMemcpyDeviceToDevice, st));
            return DCMT_OK;
        }
    }
    if (pl.needs_bbox) {
        // LC fast path: bounding boxes -> the label stage -> X4 (in pp[0]; the CLOSE5 probe: the plan's plane)
        const int32_t* d_labels = fr.labels;
        const int n_labels = fr.n_labels;
        float* x4 = pl.route == plan::Route::LABEL_PROBE ? out : ctx->pp[0];
        const dim3 bg((cols + 63) / 64, (rows + kBboxRows - 1) / kBboxRows, batch);
        with_bool(pl.bbox_lds, [&](auto lds) {
            hipLaunchKernelGGL(k_label_bbox<decltype(lds)::value>, bg, dim3(256), lds ? sizeof(int) * 4 * (size_t)n_labels : 0, st, d_src, d_labels, n_labels,
                               ctx->bb_min, ctx->bb_max, x4, rows, cols, p->max_depth, p->valid_thresh, coef);
        });
        const dim3 lg(pl.label_grid_x, batch);
        if (pl.lpair)
            with_k0(pl.k0kind, [&](auto kind) { with_bool(coef != nullptr, [&](auto norm) {
                hipLaunchKernelGGL((k_label_stage_p<decltype(kind)::value, decltype(norm)::value>), lg, dim3(256), 0, st, d_src, d_labels, n_labels,
                                   pl.label_group, ctx->bb_min, ctx->bb_max, x4, rows, cols, p->max_depth, p->valid_thresh, coef);
            }); });
        else
            with_k0(pl.k0kind, [&](auto kind) { with_bool(coef != nullptr, [&](auto norm) { with_bool(pl.label_pairs, [&](auto pairs) {
                hipLaunchKernelGGL((k_label_stage_s<decltype(kind)::value, decltype(norm)::value, decltype(pairs)::value>), lg, dim3(256), 0, st, d_src,
                                   d_labels, n_labels, ctx->bb_min, ctx->bb_max, x4, rows, cols, p->max_depth, p->valid_thresh, coef);
            }); }); });
        DCMT_HIP(ctx, hipGetLastError());
        if (pl.route == plan::Route::LABEL_PROBE) {
            if (x4 != d_dst) DCMT_HIP(ctx, hipMemcpyAsync(d_dst, x4, sizeof(float) * n_px, hipMemcpyDeviceToDevice, st));
            return DCMT_OK;
        }
    }
    if (pl.route == plan::Route::STREAMING) {
        dcmt_params q = *p;
        q.blur = blur;
        return launch_streaming(ctx, pl, fr, &q, st, sync_loop);
    }
    if (pl.route == plan::Route::LOCAL) return launch_local(ctx, pl, fr, p, blur, st);
    if (pl.u16_convert) {   // the staged kernels take f32: convert into scratch that nothing writes before they have read it
        hipLaunchKernelGGL(k_u16_to_f32, dim3(1024), dim3(256), 0, st, fr.src16, ctx->pp[0], n_px, fr.in_scale);
        d_src = ctx->pp[0];
    }

    // staged tile kernels.  Up to FILL7 the kernel that reads the frames writes the probe itself: stages 2..4 as its dump, FILL7 as
    // its X5 output
    const dim3 grid(pl.tiles_x, pl.tiles_y, batch), block(kThreads);
    const int stat_rows = pl.tiles_y;              // tile rows of the kernel that writes the column statistics
    float* x5_out = stop == DCMT_STAGE_FILL7 ? out : ctx->x5;
    float* dump_out = pl.dump ? out : d_dst;       // (not written without a dump stage)
    if (fr.labels)
        with_tile_h(pl.few, [&](auto th) {
            hipLaunchKernelGGL((k_pre_labeled_v1<decltype(th)::value, TW>), grid, block, 0, st, d_src, fr.labels, fr.n_labels, x5_out, ctx->colstat,
                               ctx->counters, dump_out, rows, cols, p->max_depth, p->valid_thresh, kb, pl.dump, coef);
        });
    else
        with_tile_h(pl.few, [&](auto th) {
            hipLaunchKernelGGL((k_pre_v1<decltype(th)::value, TW>), grid, block, 0, st, d_src, x5_out, ctx->colstat, ctx->counters, dump_out, rows, cols,
                               p->max_depth, p->valid_thresh, kb, pl.dump, coef);
        });
    DCMT_HIP(ctx, hipGetLastError());
    if (stop <= DCMT_STAGE_FILL7) {
        if (out != d_dst) DCMT_HIP(ctx, hipMemcpyAsync(d_dst, out, sizeof(float) * n_px, hipMemcpyDeviceToDevice, st));
        return DCMT_OK;
    }
    if (pl.no_extrapolate) {
        // H9..H11 on X5 itself: with no application launched k_post_v1 reads its first plane and never looks at the counters
        with_tile_h(pl.few, [&](auto th) { with_bool(pl.valid_kind, [&](auto valid) {
            hipLaunchKernelGGL((k_post_v1<decltype(th)::value, TW, decltype(valid)::value>), grid, block, 0, st, ctx->x5, ctx->x5, d_dst, ctx->counters, 0,
                               rows, cols, p->max_depth, p->valid_thresh, blur, stop);
        }); });
        DCMT_HIP(ctx, hipGetLastError());
        return DCMT_OK;
    }

    // H6 + H7 (extend_only: the EXTEND probe), and the loop's applications
    auto fill31 = [&](const float* in, float* o, int app, int extend_only) {
        with_tile_h(pl.few, [&](auto th) {
            hipLaunchKernelGGL((k_fill31_v1<decltype(th)::value, TW>), grid, block, 0, st, in, o, ctx->colstat, ctx->counters, rows, cols, p->valid_thresh,
                               app, extend_only, stat_rows);
        });
    };
    if (stop == DCMT_STAGE_EXTEND) {
        fill31(ctx->x5, d_dst, 0, 1);
        DCMT_HIP(ctx, hipGetLastError());
        return DCMT_OK;
    }
    fill31(ctx->x5, stop == DCMT_STAGE_FILL31 ? d_dst : ctx->pp[0], 0, 0);
    DCMT_HIP(ctx, hipGetLastError());
    if (stop == DCMT_STAGE_FILL31) return DCMT_OK;

    // H8
    ctx->last_has_loop = 1;
    int apps = 0;
    const int rc = fill_loop(ctx, batch, p, st, sync_loop, [&](int i) { fill31(ctx->pp[(i - 1) & 1], ctx->pp[i & 1], i, 0); }, &apps);
    if (rc != DCMT_OK && rc != DCMT_E_NOT_CONVERGED) return rc;
    ctx->last_apps_launched = apps;

    const int mode = stop <= DCMT_STAGE_FILLLOOP ? 8 : stop;
    with_tile_h(pl.few, [&](auto th) {
        hipLaunchKernelGGL((k_post_v1<decltype(th)::value, TW>), grid, block, 0, st, ctx->pp[0], ctx->pp[1], d_dst, ctx->counters, apps,
                           rows, cols, p->max_depth, p->valid_thresh, blur, mode);
    });
    DCMT_HIP(ctx, hipGetLastError());
    return rc;
}

// dcmt_evaluate_dev / dcmt_evaluate_u16_dev: checks, the slab on first use, then the two kernels (dcmt_kernels_eval.h)
template <typename TG>
int evaluate_dev(dcmt_ctx* ctx, const TG* d_gt, float gt_scale, const float* d_pred, int rows, int cols, int batch, float thresh,
                 int mode, dcmt_eval_frame* d_out, hipStream_t st)
{
    if (!ctx || !d_gt || !d_pred || !d_out) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    if (!finite_bits(thresh) || thresh < 0.0f || !finite_bits(gt_scale)) return DCMT_E_INVALID;
    if (mode != DCMT_EVAL_GT && mode != DCMT_EVAL_BOTH) return DCMT_E_INVALID;
    if ((uintptr_t)d_out % 8 != 0) return DCMT_E_INVALID;
    // first use: sized for the largest call the ctx admits (eval_chunks grows with the frame size), before any launch
    DCMT_TRY(ctx->eval_slab.reserve(ctx, (size_t)kEvalSlabStride * eval_chunks((uint32_t)ctx->frame_elems) * ctx->max_batch));
    const uint32_t n = (uint32_t)rows * (uint32_t)cols, chunks = eval_chunks(n);
    hipLaunchKernelGGL(k_eval_partial<TG>, dim3(chunks, batch), dim3(kEvalThreads), 0, st, d_gt, gt_scale, d_pred, n, thresh,
                       mode == DCMT_EVAL_BOTH ? 1 : 0, ctx->eval_slab);
    hipLaunchKernelGGL(k_eval_combine, dim3(batch), dim3(64), 0, st, ctx->eval_slab, chunks, reinterpret_cast<double*>(d_out));
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

// dcmt_colorize_dev: per segment of frames (plan_colorize: one segment unless the batch has 2^31 pixels or more) a min/max pass over
// its frames, then one map pass over its flat pixel run (dcmt_kernels_color.h)
int colorize_dev(dcmt_ctx* ctx, const float* d_src, int rows, int cols, int batch, uint8_t* d_bgr, hipStream_t st)
{
    if (!ctx || !d_src || !d_bgr) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    if ((uintptr_t)d_src % 4 != 0) return DCMT_E_INVALID;
    const plan::ColorPlan pl = plan::plan_colorize((uint32_t)rows * (uint32_t)cols, batch, (uintptr_t)d_src, (uintptr_t)d_bgr);
    for (uint32_t i = 0; i < pl.count; ++i) {
        const plan::ColorSegment sg = pl.segment(i);
        const float* s = d_src + (size_t)sg.first * pl.n;
        uint8_t* o = d_bgr + (size_t)3 * sg.first * pl.n;
        hipLaunchKernelGGL(k_color_minmax, dim3(sg.minmax_x, sg.minmax_y), dim3(kColorThreads), 0, st, s, pl.n, ctx->color_slab);
        with_bool(sg.aligned, [&](auto aligned) {
            hipLaunchKernelGGL(k_color_map<decltype(aligned)::value>, dim3(sg.map_grid), dim3(kColorThreads), sg.lds, st, s, pl.n, sg.total, ctx->color_slab,
                               pl.chunks, o);
        });
        DCMT_HIP(ctx, hipGetLastError());
    }
    return DCMT_OK;
}

// Route::LOCAL of a plan (DCMT_FLAG_NO_EXTRAPOLATE): k_local from the frames -- or from X4 in pp[0], which the label stage has left
// there -- to the plan's output plane, and the copy of an overlapping call.  blur: the effective one.
int launch_local(dcmt_ctx* ctx, const plan::Plan& pl, const Frames& fr, const dcmt_params* p, int blur, hipStream_t st)
{
    const int rows = fr.rows, cols = fr.cols, batch = fr.batch;
    const bool labeled = fr.labels != nullptr;
    const float* cf = pl.norm && !labeled ? ctx->norm_coef : nullptr;
    const void* in = labeled ? (const void*)ctx->pp[0] : fr.src16 ? (const void*)fr.src16 : (const void*)fr.src;
    const int input = labeled ? LOCAL_START4 : fr.src16 ? LOCAL_U16 : cf ? LOCAL_NORM : LOCAL_F32;
    const float scale = fr.src16 ? fr.in_scale : 1.0f;
    float* out = out_plane(ctx, pl.out, fr.dst);
    // bit 0: the Gaussian runs, bit 2: the Gaussian that ignores holes runs, bit 1: the final invert runs (stop_after = MEDIAN5 is
    // PostPipe<10, POST_BLUR_NONE>: dcmt_kernels_local.h)
    const int variant = (blur == DCMT_BLUR_GAUSSIAN && p->stop_after >= DCMT_STAGE_BLUR ? 1 : 0) | (pl.valid_kind ? 4 : 0) |
                        (p->stop_after == DCMT_STAGE_FINAL ? 2 : 0);
    with_k0(pl.k0kind, [&](auto kind) { with_value<0, 1, 2, 3>(input, [&](auto in_) { with_value<0, 1, 2, 3, 4, 6>(variant, [&](auto v) {
        constexpr int V = decltype(v)::value;
        constexpr int BLUR = (V & 4) ? POST_BLUR_VALID : (V & 1) ? POST_BLUR_GAUSSIAN : POST_BLUR_NONE;
        hipLaunchKernelGGL((k_local<decltype(kind)::value, decltype(in_)::value, (V & 2) ? 11 : 10, BLUR>), dim3(pl.local_grid), dim3(256), 0, st,
                           in, out, rows, cols, pl.local_strips, pl.local_bands, batch, pl.xcd_map, p->max_depth, p->valid_thresh, scale, cf);
    }); }); });
    DCMT_HIP(ctx, hipGetLastError());
    if (out != fr.dst) DCMT_HIP(ctx, hipMemcpyAsync(fr.dst, out, sizeof(float) * (size_t)batch * rows * cols, hipMemcpyDeviceToDevice, st));
    return DCMT_OK;
}

}  // namespace

namespace dcmt {

// (dcmt_ctx.h)
int check_params(const dcmt_ctx* ctx, const void* a, const void* b, int rows, int cols, int batch, const dcmt_params* p)
{
    if (!ctx || !a || !b || !p) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    // max_depth and valid_thresh on their bits, read from the struct's memory (the library is built with -ffinite-math-only: a float
    // compare against NaN or Inf may be folded): both finite, valid_thresh > 0 -- sign clear (-0.0 has it set) and not zero.  At
    // valid_thresh <= 0 the "0 = empty" convention of every producer and of the label stage would mean nothing.
    uint32_t mb, tb;
    std::memcpy(&mb, &p->max_depth, sizeof mb);
    std::memcpy(&tb, &p->valid_thresh, sizeof tb);
    if ((mb & 0x7f800000u) == 0x7f800000u || (tb & 0x7f800000u) == 0x7f800000u) return DCMT_E_INVALID;
    if ((tb >> 31) != 0 || (tb << 1) == 0) return DCMT_E_INVALID;
    if (p->blur == DCMT_BLUR_BILATERAL) return DCMT_E_UNSUPPORTED;
    if (p->blur != DCMT_BLUR_NONE && p->blur != DCMT_BLUR_GAUSSIAN && p->blur != DCMT_BLUR_BILATERAL_CLONE && p->blur != DCMT_BLUR_GAUSSIAN_VALID)
        return DCMT_E_INVALID;
    if (p->max_fill_iters < 1 || p->max_fill_iters > kMaxIters) return DCMT_E_INVALID;
    if (p->spec_fill_iters < 0 || p->spec_fill_iters > kMaxIters) return DCMT_E_INVALID;
    const bool norm = (p->flags & DCMT_FLAG_NORMALIZE) != 0;
    if (p->stop_after < (norm ? DCMT_STAGE_NORMALIZE : DCMT_STAGE_INVERT) || p->stop_after > DCMT_STAGE_FINAL) return DCMT_E_INVALID;
    // stages 6..8 do not exist without the extrapolation (up to FILL7 the flag is ignored)
    if ((p->flags & DCMT_FLAG_NO_EXTRAPOLATE) && p->stop_after >= DCMT_STAGE_EXTEND && p->stop_after <= DCMT_STAGE_FILLLOOP) return DCMT_E_UNSUPPORTED;
    if (norm && !(finite_bits(p->norm_lo) && finite_bits(p->norm_hi))) return DCMT_E_INVALID;
    if (k0_bits(p->k0) == 0) return DCMT_E_INVALID;
    return DCMT_OK;
}

int complete_sync(dcmt_ctx* ctx, const Frames& fr, const dcmt_params* p, bool force_gaussian, hipStream_t st)
{
    return run_chain(ctx, fr, p, force_gaussian, st, true);
}

int winner_generation(dcmt_ctx* ctx, size_t n_px, size_t n_index, hipStream_t st, unsigned* gen_tag)
{
    const bool fresh = n_px > ctx->winner.n;                // what reserve is about to replace
    // (a call that is being captured clears on every replay and leaves the context at generation 0: plan::winner_next)
    const plan::Winner w = plan::winner_next(ctx->winner_bits, ctx->winner_gen, fresh, n_index, stream_capturing(st));
    if (w.status != DCMT_OK) return w.status;
    DCMT_TRY(ctx->winner.reserve(ctx, n_px));
    if (w.clear) {
        ctx->winner_gen = 0;                                // (a clear that fails is tried again by the next call)
        DCMT_HIP(ctx, hipMemsetAsync(ctx->winner, 0, sizeof(unsigned) * ctx->winner.n, st));
    }
    ctx->winner_bits = w.bits;
    ctx->winner_gen = w.keep;
    *gen_tag = w.tag;
    return DCMT_OK;
}

}  // namespace dcmt

extern "C" {

int dcmt_version(void) { return DCMT_VERSION; }

int dcmt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* dcmt_strerror(int s)
{
    switch (s) {
        case DCMT_OK: return "ok";
        case DCMT_E_INVALID: return "invalid argument";
        case DCMT_E_UNSUPPORTED: return "unsupported (bilateral blur: the reference's in-place cv::bilateralFilter call throws; or stop_after 6..8 without the extrapolation)";
        case DCMT_E_NOMEM: return "out of memory";
        case DCMT_E_HIP: return "HIP runtime error";
        case DCMT_E_NOT_CONVERGED: return "hole-closure loop hit max_fill_iters with holes left";
        case DCMT_E_NO_DEVICE: return "no gfx950 device";
        default: return "unknown status";
    }
}

void dcmt_k0_as_compiled(uint8_t k0[25])
{
    // reference img_completion.cpp:71-77: the first 25 bytes of `int d[5][5]` = {0,0,1,0,0, 0,1,...}
    // on a little-endian host: only byte 8 (row 1, col 3) and byte 24 (row 4, col 4) are non-zero
    std::memset(k0, 0, 25);
    k0[1 * 5 + 3] = 1;
    k0[4 * 5 + 4] = 1;
}

void dcmt_k0_diamond(uint8_t k0[25])
{
    static const uint8_t d[25] = {0, 0, 1, 0, 0, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0};
    std::memcpy(k0, d, 25);
}

void dcmt_default_params(dcmt_params* p)
{
    std::memset(p, 0, sizeof(*p));
    p->max_depth = 100.0f;
    p->valid_thresh = 0.1f;
    dcmt_k0_as_compiled(p->k0);
    p->blur = DCMT_BLUR_GAUSSIAN;
    p->max_fill_iters = kMaxIters;
    p->spec_fill_iters = 1;
    p->stop_after = DCMT_STAGE_FINAL;
    p->verbose = 0;
    p->norm_lo = 0.0f;
    p->norm_hi = 100.0f;      // SL/main_sl.cpp:370 (the labeled call at :523 uses 80)
}

int dcmt_create(int device, int max_rows, int max_cols, int max_batch, dcmt_ctx** out)
{
    if (!out || max_rows < 1 || max_cols < 1 || max_batch < 1 || max_batch > 65535) return DCMT_E_INVALID;
    // a frame is one raw buffer resource addressed with 32-bit byte offsets, and kDropOffset (dcmt_kernels_fused.h) must lie
    // beyond its last byte for the "store that writes nothing" idiom: frame bytes <= 0x7fffffc0
    if ((size_t)max_rows * (size_t)max_cols > (size_t)0x1ffffff0) return DCMT_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return DCMT_E_NO_DEVICE;
    if (device < 0 || device >= n) return DCMT_E_INVALID;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return DCMT_E_HIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return DCMT_E_NO_DEVICE;   // kernels are built for gfx950 only
    dcmt_ctx* ctx = new (std::nothrow) dcmt_ctx();
    if (!ctx) return DCMT_E_NOMEM;
    ctx->device = device;
    ctx->max_rows = max_rows; ctx->max_cols = max_cols; ctx->max_batch = max_batch;
    ctx->frame_elems = (size_t)max_rows * max_cols;
    ctx->knobs = plan::knobs_from_env();
    DeviceGuard dev_guard_(ctx);                    // allocate on the context's device, leave the caller's current device as it was
    auto fail = [&](int rc) { dcmt_destroy(ctx); return rc; };
    if (dev_guard_.rc != DCMT_OK) return fail(dev_guard_.rc);
    const size_t plane = ctx->frame_elems * (size_t)max_batch;      // elements
    // two planes: X6 (x5) is dead once the first fill application of the hole-closure loop has read it, and that application writes pp[0], so
    // x5 shares pp[1] (the second application's output); X4 of the label-masked stage and the staged kernels' uint16 conversion live in
    // pp[0], which nothing writes before they have been read
    auto mem = [&](auto& buf, size_t count) { return buf.reserve(ctx, count) == DCMT_OK; };     // (whatever HIP calls the failure: DCMT_E_NOMEM)
    const size_t mb = (size_t)max_batch, chunks = eval_chunks((uint32_t)ctx->frame_elems);
    if (!mem(ctx->pp[0], plane) || !mem(ctx->pp[1], plane)) return fail(DCMT_E_NOMEM);
    ctx->x5 = ctx->pp[1];
    if (!mem(ctx->counters, kCntStride * mb) || !mem(ctx->q16_bad, kQ16Flags + 1)) return fail(DCMT_E_NOMEM);      // the ring, and the captured calls' flag
    if (hipMemset(ctx->q16_bad, 0, sizeof(int) * (kQ16Flags + 1)) != hipSuccess) return fail(DCMT_E_HIP);
    if (!mem(ctx->q16_seen, 64 / sizeof(int))) return fail(DCMT_E_NOMEM);
    *ctx->q16_seen = 0;
    if (hipHostGetDevicePointer((void**)&ctx->q16_seen_dev, ctx->q16_seen, 0) != hipSuccess) return fail(DCMT_E_HIP);
    // (first, last) table: one slot per frame and row band.  Bands are only chosen while frames x strips x bands stays near one
    // round of waves (plan_call), so frames x bands <= max_batch + kPreBandWaves; an explicit DCMT_BANDS may go up to kMaxBands each.
    const size_t tb_slots = ctx->knobs.bands > 0 ? mb * kMaxBands : std::min<size_t>(mb * kMaxBands, mb + plan::kPreBandWaves);
    if (!mem(ctx->tb, 2 * (size_t)max_cols * tb_slots) || !mem(ctx->norm_stats, 2 * mb)) return fail(DCMT_E_NOMEM);
    if (hipMemset(ctx->norm_stats, 0, sizeof(uint32_t) * 2 * mb) != hipSuccess) return fail(DCMT_E_HIP);
    if (!mem(ctx->norm_coef, 2 * mb) || !mem(ctx->color_slab, kColorSlabStride * chunks * mb) || !mem(ctx->cloud_slab, kCloudWaves * chunks * mb) ||
        !mem(ctx->h_counters, kCntStride * mb) || !mem(ctx->rectify_route, 2))
        return fail(DCMT_E_NOMEM);
    if (hipMemset(ctx->rectify_route, 0, sizeof(uint32_t) * 2) != hipSuccess) return fail(DCMT_E_HIP);
    *out = ctx;
    return DCMT_OK;
}

void dcmt_destroy(dcmt_ctx* ctx)
{
    if (!ctx) return;
    DeviceGuard dev_guard_(ctx);
    if (ctx->own_stream) { (void)hipStreamSynchronize(ctx->own_stream); (void)hipStreamDestroy(ctx->own_stream); }
    for (auto e : ctx->tev) if (e) (void)hipEventDestroy(e);
    delete ctx;                                     // every buffer frees itself, on the context's device: the guard outlives them
}

int dcmt_complete_f32_dev(dcmt_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int batch,
                          const dcmt_params* params, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    int rc = check_params(ctx, d_src, d_dst, rows, cols, batch, params);
    if (rc != DCMT_OK) return rc;
    return run_chain(ctx, Frames{d_src, nullptr, 1.0f, nullptr, 0, d_dst, rows, cols, batch}, params, false, (hipStream_t)stream, false);
}

int dcmt_complete_u16_dev(dcmt_ctx* ctx, const uint16_t* d_src, float scale, float* d_dst, int rows, int cols, int batch,
                          const dcmt_params* params, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    int rc = check_params(ctx, d_src, d_dst, rows, cols, batch, params);
    if (rc != DCMT_OK) return rc;
    return run_chain(ctx, Frames{nullptr, d_src, scale, nullptr, 0, d_dst, rows, cols, batch}, params, false, (hipStream_t)stream, false);
}

int dcmt_complete_labeled_f32_dev(dcmt_ctx* ctx, const float* d_src, const int32_t* d_labels, int n_labels, float* d_dst,
                                  int rows, int cols, int batch, const dcmt_params* params, int use_superpixel, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    int rc = check_params(ctx, d_src, d_dst, rows, cols, batch, params);
    if (rc != DCMT_OK) return rc;
    if (!d_labels) return DCMT_E_INVALID;
    return run_chain(ctx, Frames{d_src, nullptr, 1.0f, use_superpixel ? d_labels : nullptr, n_labels, d_dst, rows, cols, batch}, params, true,
                     (hipStream_t)stream, false);
}

}  // extern "C"

// T, P: the host's one pair of matrices (dcmt_project_points_dev), or null with d_table, the device's [batch] records
// (dcmt_project_points_calib_dev)
static int project_points(dcmt_ctx* ctx, const float* d_points, const int32_t* d_offsets, int n_points, int batch,
                          const float* T, const float* P, const dcmt_project_calib* d_table, float* d_sparse, int rows, int cols, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !d_offsets || (!d_table && (!T || !P)) || !d_sparse || n_points < 0 || (n_points > 0 && !d_points)) return DCMT_E_INVALID;
    if ((uintptr_t)d_points % 16 != 0) return DCMT_E_INVALID;           // the 16-byte point records are read whole
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t n_px = (size_t)batch * rows * cols;
    if (d_table && (!plan::calib_table_aligned((uintptr_t)d_table, 16) || !plan::calib_table_clear_of((uintptr_t)d_table, sizeof *d_table, batch, (uintptr_t)d_sparse, sizeof(float) * n_px))) return DCMT_E_INVALID;
    unsigned gen_tag = 0;
    const int rc = winner_generation(ctx, n_px, (size_t)n_points, st, &gen_tag);      // (2^30 points per call: 16 GiB of records)
    if (rc != DCMT_OK) return rc;
    unsigned* winner = ctx->winner;
    const auto launch = [&](auto src) {                // ProjMats or ProjTable
        using Src = decltype(src);
        if (n_points > 0)
            hipLaunchKernelGGL(k_project_scatter<Src>, dim3((n_points + 255) / 256), dim3(256), 0, st, d_points, d_offsets, n_points, batch, src,
                               winner, rows, cols, gen_tag);
        with_value<4, 2, 1>(plan::resolve_vec(n_px, (uintptr_t)d_sparse), [&](auto v) {
            hipLaunchKernelGGL((k_project_resolve<decltype(v)::value, Src>), dim3((unsigned)((n_px / v + 255) / 256)), dim3(256), 0, st, d_points, src, winner,
                               d_sparse, n_px, gen_tag, ctx->winner_bits, (uint32_t)rows * (uint32_t)cols);
        });
    };
    if (d_table) launch(ProjTable{d_table});
    else launch(proj_mats(T, P));
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

// d_table: null (dcmt_stereo_refine_dev: baseline and focal from params) or the device's [batch] records (dcmt_stereo_refine_calib_dev)
static int stereo_refine(dcmt_ctx* ctx, const float* d_depth, const uint8_t* d_left, const uint8_t* d_right, float* d_refined,
                         int rows, int cols, int batch, const dcmt_stereo_params* params, const dcmt_stereo_calib* d_table, bool table, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !d_depth || !d_left || !d_right || !d_refined || !params) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    if (params->iterations > 1000) return DCMT_E_INVALID;
    if (table && (!plan::calib_table_aligned((uintptr_t)d_table, 8) || !plan::calib_table_clear_of((uintptr_t)d_table, sizeof *d_table, batch, (uintptr_t)d_refined, sizeof(float) * (size_t)batch * rows * cols)))
        return DCMT_E_INVALID;
    StereoP P{params->baseline, params->focal, params->damp, params->max_depth, params->iterations < 0 ? 4 : params->iterations};
    const plan::StereoPlan pl = plan::plan_stereo(rows, cols, batch);
    if (pl.status != DCMT_OK) return pl.status;
    const dim3 sg(pl.gx, pl.gy, pl.gz);
    const auto launch = [&](auto src) {                // StereoP or StereoTable
        with_bool(pl.lds_row, [&](auto lds_row) {
            hipLaunchKernelGGL((k_stereo_refine<decltype(lds_row)::value, decltype(src)>), sg, dim3(256), lds_row ? pl.lds : 0, (hipStream_t)stream, d_depth,
                               d_left, d_right, d_refined, rows, cols, batch, src);
        });
    };
    if (table) launch(StereoTable{d_table, P.damp, P.max_depth, P.iterations});
    else launch(P);
    DCMT_HIP(ctx, hipGetLastError());
    return DCMT_OK;
}

extern "C" {

int dcmt_project_points_dev(dcmt_ctx* ctx, const float* d_points, const int32_t* d_offsets, int n_points, int batch,
                            const float T[16], const float P[12], float* d_sparse, int rows, int cols, void* stream)
{
    if (!T || !P) return DCMT_E_INVALID;
    return project_points(ctx, d_points, d_offsets, n_points, batch, T, P, nullptr, d_sparse, rows, cols, stream);
}

int dcmt_project_points_calib_dev(dcmt_ctx* ctx, const float* d_points, const int32_t* d_offsets, int n_points, int batch,
                                  const dcmt_project_calib* d_calib, float* d_sparse, int rows, int cols, void* stream)
{
    if (!d_calib) return DCMT_E_INVALID;
    return project_points(ctx, d_points, d_offsets, n_points, batch, nullptr, nullptr, d_calib, d_sparse, rows, cols, stream);
}

void dcmt_default_stereo_params(dcmt_stereo_params* p)
{
    p->baseline = 0.54f;          // SL/main_sl.cpp:847
    p->focal = 9.597910e+02f;     // :848
    p->damp = 500.0f;             // :808
    p->max_depth = 100.0f;        // :876
    p->iterations = 4;            // :805
}

int dcmt_stereo_refine_dev(dcmt_ctx* ctx, const float* d_depth, const uint8_t* d_left, const uint8_t* d_right, float* d_refined,
                           int rows, int cols, int batch, const dcmt_stereo_params* params, void* stream)
{
    return stereo_refine(ctx, d_depth, d_left, d_right, d_refined, rows, cols, batch, params, nullptr, false, stream);
}

int dcmt_stereo_refine_calib_dev(dcmt_ctx* ctx, const float* d_depth, const uint8_t* d_left, const uint8_t* d_right, float* d_refined,
                                 int rows, int cols, int batch, const dcmt_stereo_params* params, const dcmt_stereo_calib* d_calib, void* stream)
{
    return stereo_refine(ctx, d_depth, d_left, d_right, d_refined, rows, cols, batch, params, d_calib, true, stream);
}

int dcmt_evaluate_dev(dcmt_ctx* ctx, const float* d_gt, const float* d_pred, int rows, int cols, int batch, float thresh, int mode,
                      dcmt_eval_frame* d_out, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    return evaluate_dev(ctx, d_gt, 1.0f, d_pred, rows, cols, batch, thresh, mode, d_out, (hipStream_t)stream);
}

int dcmt_evaluate_u16_dev(dcmt_ctx* ctx, const uint16_t* d_gt, float gt_scale, const float* d_pred, int rows, int cols, int batch,
                          float thresh, int mode, dcmt_eval_frame* d_out, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    return evaluate_dev(ctx, d_gt, gt_scale, d_pred, rows, cols, batch, thresh, mode, d_out, (hipStream_t)stream);
}

int dcmt_colorize_dev(dcmt_ctx* ctx, const float* d_src, int rows, int cols, int batch, uint8_t* d_bgr, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    return colorize_dev(ctx, d_src, rows, cols, batch, d_bgr, (hipStream_t)stream);
}

void dcmt_colormap_jet(uint8_t bgr[768])
{
    if (!bgr) return;
    static const uint32_t jet[256] = {DCMT_JET_BGR_PACKED};
    for (int i = 0; i < 256; ++i) {
        bgr[3 * i] = (uint8_t)jet[i];
        bgr[3 * i + 1] = (uint8_t)(jet[i] >> 8);
        bgr[3 * i + 2] = (uint8_t)(jet[i] >> 16);
    }
}

int dcmt_slic_num_centers(int rows, int cols, int step) { return plan::slic_num_centers(rows, cols, step); }

int dcmt_slic_labels_dev(dcmt_ctx* ctx, const uint8_t* d_lab, int rows, int cols, int batch, int step, int nc,
                         int32_t* d_labels, double* d_centers, void* stream)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !d_lab || !d_labels) return DCMT_E_INVALID;
    if (!dims_ok(ctx, rows, cols, batch)) return DCMT_E_INVALID;
    if (step < 6 || nc < 1) return DCMT_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const char* e_scale = std::getenv("DCMT_SLIC_CELL_SCALE");
    const char* e_th = std::getenv("DCMT_SLIC_TH");
    const plan::SlicPlan pl = plan::plan_slic(rows, cols, batch, ctx->max_batch, step, e_scale ? std::atoi(e_scale) : 0, e_th ? std::atoi(e_th) : 0);
    const int n = pl.n, cell_px = pl.cell_px, gx = pl.gx, gy = pl.gy;
    if (n == 0) { DCMT_HIP(ctx, hipMemsetAsync(d_labels, 0xFF, sizeof(int32_t) * pl.clear_labels, st)); return DCMT_OK; }
    DCMT_TRY(ctx->slic_cells.reserve(ctx, pl.reserve_cells));
    DCMT_TRY(ctx->slic_centers[0].reserve(ctx, pl.reserve_centers));
    DCMT_TRY(ctx->slic_centers[1].reserve(ctx, pl.reserve_centers));
    DCMT_TRY(ctx->slic_sums.reserve(ctx, pl.reserve_sums));
    int* const cells = ctx->slic_cells;
    int* set_cnt[2] = {cells + pl.cnt[0], cells + pl.cnt[1]};
    int* set_ovf[2] = {cells + pl.ovf[0], cells + pl.ovf[1]};
    int* set_list[2] = {cells + pl.list[0], cells + pl.list[1]};
    DCMT_HIP(ctx, hipMemsetAsync(d_labels, 0xFF, sizeof(int32_t) * pl.clear_labels, st));                  // clusters = -1 (slic.cpp:24)
    DCMT_HIP(ctx, hipMemsetAsync(set_cnt[0], 0, sizeof(int) * pl.clear_cnt, st));                          // both cell sets' counts and flags
    DCMT_HIP(ctx, hipMemsetAsync(ctx->slic_sums, 0, sizeof(unsigned long long) * pl.clear_sums, st));      // every iteration leaves them zeroed
    hipLaunchKernelGGL(k_slic_init, dim3(pl.init_x, batch), dim3(64), 0, st, d_lab, ctx->slic_centers[0], rows, cols, step, n,
                       set_cnt[0], set_list[0], set_ovf[0], cell_px, gx, gy);
    for (int it = 0; it < 10; ++it) {                                                           // NR_ITERATIONS (slic.h:20)
        double* cur = ctx->slic_centers[it & 1];
        double* nxt = ctx->slic_centers[(it + 1) & 1];
        const int a = it & 1, b = a ^ 1;
        with_value<64, 32, 16>(pl.th, [&](auto h) {
            hipLaunchKernelGGL(k_slic_assign<decltype(h)::value>, dim3(pl.tiles_x, pl.tiles_y, batch), dim3(256), 0, st, d_lab, cur,
                               set_cnt[a], set_list[a], set_ovf[a], d_labels, ctx->slic_sums, rows, cols, step, nc, n, gx, gy, cell_px);
        });
        hipLaunchKernelGGL(k_slic_norm_bin, dim3(pl.bin_x), dim3(256), 0, st, ctx->slic_sums, nxt, n, batch,
                           set_cnt[b], set_list[b], set_ovf[b], set_cnt[a], (int)pl.n_cnt, cell_px, gx, gy);
        DCMT_HIP(ctx, hipGetLastError());
    }
    if (d_centers)       // ten iterations: the final centres are back in buffer 0
        DCMT_HIP(ctx, hipMemcpyAsync(d_centers, ctx->slic_centers[0], sizeof(double) * 5 * (size_t)n * batch, hipMemcpyDeviceToDevice, st));
    return DCMT_OK;
}

int dcmt_last_fill_iters(dcmt_ctx* ctx, int* out, int n)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !out || n < 0 || n > ctx->last_batch) return DCMT_E_INVALID;
    if (stream_capturing(ctx->last_stream)) return DCMT_E_INVALID;                     // nothing of the call has run, and its stream cannot be waited for
    if (ctx->last_no_extrapolate) { std::fill(out, out + n, 0); return DCMT_OK; }      // no loop ran
    if (!ctx->last_has_loop) return DCMT_E_INVALID;
    int rc = read_counters(ctx, ctx->last_stream, ctx->last_batch);
    if (rc != DCMT_OK) return rc;
    for (int f = 0; f < n; ++f) {
        const int* c = ctx->h_counters + (size_t)f * kCntStride;
        int a = 0;
        while (a < ctx->last_apps_launched && c[1 + a] > 0) ++a;
        if (c[1 + a] > 0) { out[f] = -1; rc = DCMT_E_NOT_CONVERGED; }
        else out[f] = a + 1;
    }
    return rc;
}

int dcmt_last_holes_after_extend(dcmt_ctx* ctx, int* out, int n)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !out || n < 0 || n > ctx->last_batch) return DCMT_E_INVALID;
    if (stream_capturing(ctx->last_stream)) return DCMT_E_INVALID;
    if (ctx->last_no_extrapolate) { std::fill(out, out + n, 0); return DCMT_OK; }      // no extension ran
    int rc = read_counters(ctx, ctx->last_stream, ctx->last_batch);
    if (rc != DCMT_OK) return rc;
    for (int f = 0; f < n; ++f) out[f] = ctx->h_counters[(size_t)f * kCntStride];
    return DCMT_OK;
}

int dcmt_last_hip_error(const dcmt_ctx* ctx) { return ctx ? ctx->last_hip_error : 0; }

// a dcmt_rectify_dev call leaves "k_rectify" here (dcmt_rectify.hip): which routes its tiles took is the kernel's to say, in the two
// words of rectify_route
const char* dcmt_last_path(const dcmt_ctx* ctx)
{
    if (!ctx) return "";
    if (std::strcmp(ctx->last_path, "k_rectify") != 0) return ctx->last_path;
    uint32_t w[2] = {0, 0};
    if (hipMemcpy(w, ctx->rectify_route.p, sizeof w, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return ctx->last_path;
    }
    const bool lds = w[0] == ctx->rectify_call, gather = w[1] == ctx->rectify_call;
    return lds && gather ? "k_rectify<lds+gather>" : lds ? "k_rectify<lds>" : gather ? "k_rectify<gather>" : ctx->last_path;
}

int dcmt_set_kernel_timing(dcmt_ctx* ctx, int on)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx) return DCMT_E_INVALID;
    if (on)
        for (auto& e : ctx->tev)
            if (!e) DCMT_HIP(ctx, hipEventCreate(&e));
    ctx->timing = on != 0;
    ctx->tev_valid = 0;
    return DCMT_OK;
}

int dcmt_last_kernel_times(dcmt_ctx* ctx, float ms[DCMT_N_KERNEL_TIMES])
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !ms || !ctx->tev_valid) return DCMT_E_INVALID;
    DCMT_HIP(ctx, hipEventSynchronize(ctx->tev[4]));
    for (int i = 0; i < DCMT_N_KERNEL_TIMES; ++i) DCMT_HIP(ctx, hipEventElapsedTime(&ms[i], ctx->tev[i], ctx->tev[i + 1]));
    return DCMT_OK;
}

}  // extern "C"
