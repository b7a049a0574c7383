// dcmt_ctx.h -- what the translation units of the library share and nobody else sees (not installed): the context behind
// dcmt.h's opaque dcmt_ctx and the helpers every entry point starts with.  No kernel here, and no kernel header: dcmt.hip and
// dcmt_cloud.hip each compile their own kernels, dcmt_host.hip compiles none.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "dcmt.h"
#include "dcmt_plan.h"

struct dcmt_ctx;

namespace dcmt {

// One allocation of the context and its element count: device memory, or host memory that is pinned (h_counters) or pinned and
// mapped (q16_seen).  Frees itself with the context; reads as a plain T* wherever one is expected (launch arguments, arithmetic).
// DCMT_LOCAL keeps an internal name out of libdcmt_hip.so's dynamic symbol table
#define DCMT_LOCAL __attribute__((visibility("hidden")))
enum class Mem { DEVICE, PINNED, MAPPED };
template <typename T, Mem M = Mem::DEVICE>
struct DCMT_LOCAL Buf {
    T* p = nullptr;
    size_t n = 0;                     // elements allocated
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    operator T*() const { return p; }
    void release()
    {
        if (p) (void)(M == Mem::DEVICE ? hipFree(p) : hipHostFree(p));
        p = nullptr; n = 0;
    }
    // Room for `count` elements: nothing when they fit, otherwise free and allocate (the contents are lost; *reallocated is set, and
    // left alone otherwise, so one flag can watch several buffers).  A failure leaves the buffer empty and is reported as DCMT_HIP
    // reports it.  An allocation synchronises the device: callers reserve before they enqueue anything of a call.
    int reserve(dcmt_ctx* ctx, size_t count, bool* reallocated = nullptr);
};

}  // namespace dcmt

// Who allocates what: dcmt_create unless the comment names a first user; what a first user allocates is sized for the context's
// maxima and never again, what is "grown on demand" is reallocated by a call that needs more than any before it.
struct dcmt_ctx {
    template <typename T> using Dev = dcmt::Buf<T>;
    DCMT_LOCAL ~dcmt_ctx() = default;
    int device = 0;
    int max_rows = 0, max_cols = 0, max_batch = 0;
    size_t frame_elems = 0;           // max_rows * max_cols
    // device scratch
    Dev<float> pp[2];                 // [max_batch][rows][cols] each: ping-pong of the large-fill applications
    float* x5 = nullptr;              // cascade after the small fill: an alias of pp[1], owns nothing (see dcmt_create)
    Dev<int> colstat;                 // [max_batch][tile rows][2][cols]  (staged path; the first call whose plan names it)
    Dev<int> counters;                // [max_batch][kCntStride]
    Dev<int> tb;                      // [max_batch][2][max_cols]: first / last valid row of every X6 column (k_pre table mode -> k_fp_s)
    Dev<uint32_t> norm_stats;         // [max_batch][2]  N1: order-preserving keys of each frame's max and (inverted) min
    Dev<float> norm_coef;             // [max_batch][2]  N1: dst = src * a + b
    // staging of dcmt_complete_f32 / dcmt_complete_labeled_f32 (dcmt_host.hip), [max_batch][rows][cols] each: allocated by the first
    // such call (d_lab: the first labeled one) and kept, because these are called once per frame in a loop
    Dev<float> d_in;
    Dev<float> d_out;
    Dev<int32_t> d_lab;
    dcmt::Buf<int, dcmt::Mem::PINNED> h_counters;   // [max_batch][kCntStride]: where read_counters puts the hole counters
    hipStream_t own_stream = nullptr; // the host entry points' stream, created by the first of them
    // state of the last call
    hipStream_t last_stream = nullptr;
    int last_batch = 0;
    int last_apps_launched = 0;       // loop applications (app >= 1) enqueued
    int last_has_loop = 0;            // the call went at least through H8
    int last_no_extrapolate = 0;      // the call ran without H6..H8 (DCMT_FLAG_NO_EXTRAPOLATE): dcmt_last_fill_iters and dcmt_last_holes_after_extend report zeros
    int last_hip_error = 0;
    char last_path[160] = "";         // dcmt_last_path: the kernels the last call dispatched
    int timing = 0;                   // dcmt_set_kernel_timing: events around the kernel groups of the streaming path
    hipEvent_t tev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int tev_valid = 0;                // the last call recorded all five
    dcmt::plan::Knobs knobs;                // the environment knobs (dcmt_plan.h), read by dcmt_create
    Dev<unsigned short> x6q;          // [max_batch][rows][cols] X6 as 16-bit codes (k_pre_p<Q16OUT> -> k_fp_q) and 16 bytes of slack; the first
                                      // call whose plan names it
    Dev<int> q16_bad;                 // a ring of kQ16Flags flags; attempt n uses flag n % kQ16Flags: raised by k_pre_p<Q16OUT> when a value it stored was
                                      // not a code, and cleared one attempt ahead by that kernel too (no memset in the stream).  One more flag
                                      // behind the ring is the captured calls': a replay cannot move round a ring, so a call made while its
                                      // stream is capturing uses this one and clears it itself, with a node in front of its kernels
    unsigned q16_attempts = 0;
    dcmt::Buf<int, dcmt::Mem::MAPPED> q16_seen;     // pinned host word (and its device address) the same kernel sets: the NEXT calls skip the 16-bit attempt
    int* q16_seen_dev = nullptr;      // (an alias, owns nothing)
    int q16_skip = 0;                 // calls left without an attempt (after a raised flag: 63, then one more try)
    Dev<unsigned> winner;             // the winner plane of dcmt_project_points_dev and dcmt_reproject_depth_dev (tags: generation | index; winner_generation),
                                      // allocated by the first call of either, grown on demand
    int winner_bits = 0;              // index bits of the plane's tag layout
    unsigned winner_gen = 0;          // generation of the last call (0: the plane is all zeros and nothing has been written)
    Dev<int> bb_min;                  // LC fast path: per (frame, label) bounding boxes, grown on demand (ensure_bbox), both together
    Dev<int> bb_max;
    // N3 (SLIC) scratch, allocated by the first dcmt_slic_labels_dev call and grown on demand.  All four hold max_batch frames, so
    // their counts grow with the cells / centres per frame and no per-frame capacity is kept beside them.
    Dev<int> slic_cells;              // two cell sets: counts [batch][cells] + overflow flags [batch] each, then the index lists [batch][cells][kSlicCellCap] each
    Dev<double> slic_centers[2];      // the three centre buffers grow together
    Dev<unsigned long long> slic_sums;
    Dev<double> eval_slab;            // dcmt_evaluate*_dev: per (frame, chunk) partial sums, sized for max_batch frames of max_rows x max_cols,
                                      // allocated by the first evaluate call
    Dev<float> color_slab;            // dcmt_colorize_dev: per (frame, chunk) min and max, sized for max_batch frames of max_rows x max_cols
    Dev<float> median;                // [max_batch][rows][cols] the cascade's bilateral finish: the median plane k_bilateral5 reads (pp[0] and pp[1] both
                                      // hold frames' loop results then); the first call with DCMT_BLUR_BILATERAL_CLONE
    Dev<uint32_t> cloud_slab;         // dcmt_depth_to_cloud_dev: per (frame, chunk, wave) record counts, then their exclusive bases; sized like
                                      // color_slab, kCloudWaves entries per chunk
    Dev<uint32_t> conn_slab;          // dcmt_slic_connectivity_dev: per (frame, strip of 64 columns) counts of non-small seeds, then their exclusive
                                      // bases; max_batch x ceil(max_cols / 64) words, allocated by the first such call
    Dev<uint32_t> rectify_route;      // dcmt_rectify_dev's probe: two words (kRectifyRouteLds, kRectifyRouteGather, dcmt_rectify.h), each the id of
                                      // the last call of which a tile took that route; written by k_rectify, read by dcmt_last_path.  Nothing
                                      // else of a rectify call stays behind
    uint32_t rectify_call = 0;        // id of the last dcmt_rectify_dev call (0: none yet; last_path then starts with "k_rectify")
};

namespace dcmt {

// A HIP error becomes the call's status and dcmt_last_hip_error, and stops being the thread's last HIP error: left there, it would be
// what this library's next launch check reports, or that of a framework sharing the runtime (a refused allocation, say)
#define DCMT_HIP(ctx, call)                                        \
    do {                                                           \
        hipError_t e_ = (call);                                    \
        if (e_ != hipSuccess) {                                    \
            (void)hipGetLastError();                               \
            if (ctx) (ctx)->last_hip_error = (int)e_;              \
            return e_ == hipErrorOutOfMemory ? DCMT_E_NOMEM : DCMT_E_HIP; \
        }                                                          \
    } while (0)

// the same for a call that returns a dcmt_status
#define DCMT_TRY(call)                                             \
    do {                                                           \
        const int rc_ = (call);                                    \
        if (rc_ != DCMT_OK) return rc_;                            \
    } while (0)

template <typename T, Mem M>
int Buf<T, M>::reserve(dcmt_ctx* ctx, size_t count, bool* reallocated)
{
    if (count <= n) return DCMT_OK;
    release();
    if (reallocated) *reallocated = true;
    void* q = nullptr;
    DCMT_HIP(ctx, M == Mem::DEVICE ? hipMalloc(&q, sizeof(T) * count) : hipHostMalloc(&q, sizeof(T) * count, M == Mem::MAPPED ? hipHostMallocMapped : hipHostMallocDefault));
    p = static_cast<T*>(q); n = count;
    return DCMT_OK;
}

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

// f(std::integral_constant<_, V>{}) with the first of the listed values that equals v, the last one where none does: a runtime
// value as a template argument, out of that list
template <auto V, auto... Rest, typename T, typename F>
void with_value(T v, F f)
{
    if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<decltype(V), V>{});
    else if (v == V) f(std::integral_constant<decltype(V), V>{});
    else with_value<Rest...>(v, f);
}

// `st` is being captured into a graph (dcmt.h, "Graph capture"): what the call enqueues runs later, any number of times, with the
// arguments it is given now.  A stream that cannot be asked (the null stream while another one captures) is not capturing; the
// error does not stay behind.
inline bool stream_capturing(hipStream_t st)
{
    hipStreamCaptureStatus s = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &s) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return s != hipStreamCaptureStatusNone;
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

// pinhole intrinsics the point cloud and the reprojection can divide by
DCMT_LOCAL inline bool intrinsics_ok(double fx, double fy, double cx, double cy)
{
    return finite_bits64(fx) && finite_bits64(fy) && finite_bits64(cx) && finite_bits64(cy) && fx != 0.0 && fy != 0.0;
}

// The winner plane of dcmt_project_points_dev and dcmt_reproject_depth_dev: tags of generation g = (g << idx_bits) | index, g >= 1
// (0 = the cleared plane); the index is N2's global point index or the reprojection's frame-local source pixel index.  A call only
// looks at tags of its own generation, so the plane is not cleared between calls, whichever of the two they are.  It is cleared when
// it is (re)allocated, when a call needs more index bits than its layout has, and when the generations run out.  n_px: entries
// this call needs; n_index: it stores indices below n_index (N2 keeps its bound of <= n_index).  Any allocation happens here, before
// the call has enqueued anything.  Returns the call's generation, shifted into place.  The state's step is plan::winner_next
// (dcmt_plan_side.h); this function, defined in dcmt.hip, reserves and clears as it says.
int winner_generation(dcmt_ctx* ctx, size_t n_px, size_t n_index, hipStream_t st, unsigned* gen_tag);

// What a completion call is given: device pointers (src or src16; labels only where they are used) and the batch's shape
struct Frames {
    const float* src;
    const uint16_t* src16;
    float in_scale;
    const int32_t* labels;
    int n_labels;
    float* dst;
    int rows, cols, batch;
};

// What dcmt_complete_f32 and dcmt_complete_labeled_f32 (dcmt_host.hip) need of the cascade, which the *_dev ABI does not offer.
// check_params: the checks every dcmt_complete_* entry point starts with (a, b: its source and destination).  complete_sync: the
// cascade on the device planes of `fr`, enqueued on `st`, with the hole-closure loop run exactly as the reference runs it -- the hole
// counters are read back between applications, so the call synchronises with `st` -- and DCMT_E_NOT_CONVERGED where the loop hit
// p->max_fill_iters (dst is written all the same).  Both defined in dcmt.hip.
DCMT_LOCAL int check_params(const dcmt_ctx* ctx, const void* a, const void* b, int rows, int cols, int batch, const dcmt_params* p);
DCMT_LOCAL int complete_sync(dcmt_ctx* ctx, const Frames& fr, const dcmt_params* p, bool force_gaussian, hipStream_t st);

// k_bilateral5 (dcmt_kernels_bilateral.h) enqueued on `st`, for dcmt_bilateral5_dev and the cascade's bilateral finish: d_src and
// d_dst must not overlap; invert: the cascade's final invert with (max_depth, thr) in the store.  DCMT_E_INVALID for a sigma that is
// not finite and positive.  Defined in dcmt_cloud.hip, where the kernel is compiled.
DCMT_LOCAL int bilateral5_enqueue(dcmt_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int batch, float sigma_color,
                                  float sigma_space, bool invert, float max_depth, float thr, hipStream_t st);

// k_gauss5<VALID> (dcmt_kernels_cloud.h) enqueued on `st`, for dcmt_gaussian5_valid_dev and the extrapolating cascade's
// DCMT_BLUR_GAUSSIAN_VALID finish: d_src and d_dst must not overlap; invert: the cascade's final invert with (max_depth, thr) in the
// store.  Defined in dcmt_cloud.hip, where the kernel is compiled.
DCMT_LOCAL int gauss5_valid_enqueue(dcmt_ctx* ctx, const float* d_src, float* d_dst, int rows, int cols, int batch, float thr, bool invert,
                                    float max_depth, hipStream_t st);

}  // namespace dcmt
