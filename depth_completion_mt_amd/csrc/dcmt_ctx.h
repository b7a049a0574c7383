// dcmt_ctx.h -- what the translation units of the library share and nobody else sees (not installed): the context behind
// dcmt.h's opaque dcmt_ctx and the helpers every entry point starts with.  No kernel here, and no kernel header: dcmt.hip and
// dcmt_cloud.hip each compile their own kernels, dcmt_host.hip compiles none.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "dcmt.h"
#include "dcmt_plan.h"

struct dcmt_ctx {
    int device = 0;
    int max_rows = 0, max_cols = 0, max_batch = 0;
    size_t frame_elems = 0;           // max_rows * max_cols
    // device scratch
    float* x5 = nullptr;              // [max_batch][rows][cols] : cascade after the small fill (= pp[1], see dcmt_create)
    float* pp[2] = {nullptr, nullptr};// ping-pong of the large-fill applications
    int* colstat = nullptr;           // [max_batch][tile rows][2][cols]  (staged path)
    int* counters = nullptr;          // [max_batch][kCntStride]
    int* tb = nullptr;                // [max_batch][2][max_cols]: first / last valid row of every X6 column (k_pre table mode -> k_fp_s)
    uint32_t* norm_stats = nullptr;   // [max_batch][2]  N1: order-preserving keys of each frame's max and (inverted) min
    float* norm_coef = nullptr;       // [max_batch][2]  N1: dst = src * a + b
    // host-entry staging (allocated on first use)
    float* d_in = nullptr;
    float* d_out = nullptr;
    int32_t* d_lab = nullptr;
    int* h_counters = nullptr;        // pinned
    hipStream_t own_stream = nullptr;
    // state of the last call
    hipStream_t last_stream = nullptr;
    int last_batch = 0;
    int last_apps_launched = 0;       // loop applications (app >= 1) enqueued
    int last_has_loop = 0;            // the call went at least through H8
    int last_hip_error = 0;
    char last_path[160] = "";         // dcmt_last_path: the kernels the last call dispatched
    int timing = 0;                   // dcmt_set_kernel_timing: events around the kernel groups of the streaming path
    hipEvent_t tev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int tev_valid = 0;                // the last call recorded all five
    dcmt::plan::Knobs knobs;                // the environment knobs (dcmt_plan.h), read by dcmt_create
    unsigned short* x6q = nullptr;    // [max_batch][rows][cols] X6 as 16-bit codes (k_pre_p<Q16OUT> -> k_fp_q)
    int* q16_bad = nullptr;           // a ring of kQ16Flags flags; attempt n uses flag n % kQ16Flags: raised by k_pre_p<Q16OUT> when a value it stored was
                                      // not a code, and cleared one attempt ahead by that kernel too (no memset in the stream)
    unsigned q16_attempts = 0;
    int* q16_seen = nullptr;          // pinned host word (and its device address) the same kernel sets: the NEXT calls skip the 16-bit attempt
    int* q16_seen_dev = nullptr;
    int q16_skip = 0;                 // calls left without an attempt (after a raised flag: 63, then one more try)
    unsigned* winner = nullptr;       // the winner plane of dcmt_project_points_dev and dcmt_reproject_depth_dev (tags: generation | index; winner_generation),
                                      // allocated by the first call of either
    size_t winner_elems = 0;
    int winner_bits = 0;              // index bits of the plane's tag layout
    unsigned winner_gen = 0;          // generation of the last call (0: the plane is all zeros and nothing has been written)
    int* bb_min = nullptr;            // LC fast path: per (frame, label) bounding boxes, grown on demand
    int* bb_max = nullptr;
    size_t bb_ints = 0;
    // N3 (SLIC) scratch, allocated by the first dcmt_slic_labels_dev call
    int* slic_cells = nullptr;                  // two cell sets: counts [batch][cells] + overflow flags [batch] each, then the index lists [batch][cells][kSlicCellCap] each
    size_t slic_cell_cap = 0;                   // cells per frame that buffer holds
    double* slic_centers[2] = {nullptr, nullptr};
    unsigned long long* slic_sums = nullptr;
    size_t slic_center_cap = 0;                 // centres per frame the two buffers above hold
    double* eval_slab = nullptr;      // dcmt_evaluate*_dev: per (frame, chunk) partial sums, sized for max_batch frames of max_rows x max_cols,
                                      // allocated by the first evaluate call
    float* color_slab = nullptr;      // dcmt_colorize_dev: per (frame, chunk) min and max, sized for max_batch frames of max_rows x max_cols
                                      // (allocated by dcmt_create)
    uint32_t* cloud_slab = nullptr;   // dcmt_depth_to_cloud_dev: per (frame, chunk, wave) record counts, then their exclusive bases; sized like
                                      // color_slab, kCloudWaves entries per chunk (allocated by dcmt_create)
};

namespace dcmt {

#define DCMT_HIP(ctx, call)                                        \
    do {                                                           \
        hipError_t e_ = (call);                                    \
        if (e_ != hipSuccess) {                                    \
            if (ctx) (ctx)->last_hip_error = (int)e_;              \
            return e_ == hipErrorOutOfMemory ? DCMT_E_NOMEM : DCMT_E_HIP; \
        }                                                          \
    } while (0)

// Every entry point that takes a context runs with that context's device current and puts the caller's current device back
// before it returns: one process may drive several GPUs, one host thread + one dcmt_ctx + one stream per GPU (HIP's current
// device is per thread), and a library that is shared with a framework (torch) must not move that framework's device.
struct DeviceGuard {
    int prev = -1, rc = DCMT_OK;
    explicit DeviceGuard(dcmt_ctx* ctx)
    {
        if (!ctx) return;                                   // the entry point reports DCMT_E_INVALID itself
        if (hipGetDevice(&prev) != hipSuccess) { prev = -1; rc = DCMT_E_HIP; return; }
        if (prev != ctx->device) {
            const hipError_t e = hipSetDevice(ctx->device);
            if (e != hipSuccess) { ctx->last_hip_error = (int)e; rc = DCMT_E_HIP; prev = -1; }
        } else prev = -1;                                   // nothing to restore
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define DCMT_ON_DEVICE(ctx) DeviceGuard dev_guard_(ctx); if (dev_guard_.rc != DCMT_OK) return dev_guard_.rc

// the library is built with -ffinite-math-only: test the exponent bits, not the value -- and read them through memory, or the
// compiler, which may assume every float argument finite, folds the test to true
inline bool finite_bits(float v)
{
    volatile float m = v;
    const float c = m;
    uint32_t b;
    std::memcpy(&b, &c, sizeof b);
    return (b & 0x7f800000u) != 0x7f800000u;
}

// rows x cols x batch is a size the context was created for
inline bool dims_ok(const dcmt_ctx* ctx, int rows, int cols, int batch)
{
    return rows >= 1 && cols >= 1 && batch >= 1 && batch <= ctx->max_batch && rows <= ctx->max_rows && cols <= ctx->max_cols;
}

// as finite_bits, for the f64 intrinsics of dcmt_cloud_params
inline bool finite_bits64(double v)
{
    volatile double m = v;
    uint64_t b;
    double t = m;
    std::memcpy(&b, &t, sizeof b);
    return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// The winner plane of dcmt_project_points_dev and dcmt_reproject_depth_dev: tags of generation g = (g << idx_bits) | index, g >= 1
// (0 = the cleared plane); the index is N2's global point index or the reprojection's frame-local source pixel index.  A call only
// looks at tags of its own generation, so the plane is not cleared between calls, whichever of the two they are.  It is cleared when
// it is (re)allocated, when a call needs more index bits than its layout has, and when the generations run out.  n_px: entries
// this call needs; n_index: it stores indices below n_index (N2 keeps its bound of <= n_index).  Any allocation happens here, before
// the call has enqueued anything.  Returns the call's generation, shifted into place.  Defined in dcmt.hip.
int winner_generation(dcmt_ctx* ctx, size_t n_px, size_t n_index, hipStream_t st, unsigned* gen_tag);

// eval_chunks(n) and eval_chunk_groups(n) of dcmt_kernels_eval.h, for a translation unit that must not compile that header's
// kernels (dcmt_cloud.hip, whose kernels walk a frame in the same chunks).  Defined in dcmt.hip.
void frame_chunks(uint32_t n, uint32_t* chunks, uint32_t* groups);

}  // namespace dcmt
