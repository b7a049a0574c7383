// dcmt_plan.h -- which kernels a completion call runs, as a value: plan_call() turns the environment knobs and one call's
// arguments into a Plan, dcmt.hip allocates what the plan names and then launches it.  Plain C++17, no HIP: the decisions are
// tested on a CPU (tests/test_plan.py).  Values a kernel header owns are copied here; dcmt.hip static_asserts every copy.
#ifndef DCMT_PLAN_H
#define DCMT_PLAN_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace dcmt {
namespace plan {

// ---- environment knobs (read by dcmt_create; every combination produces identical bits) ---------------------------------
struct Knobs {
    int poison = 0;                   // DCMT_POISON=1: fill the staging output with NaN before every host call
    int xcd_map = 1;                  // XCD-aware workgroup->frame mapping; DCMT_XCD_MAP=0 disables
    int wide = 1;                     // LDS-DMA row loads where alignment allows; DCMT_WIDE=0 disables
    int fuse_fp = 1;                  // H7..H11 in one kernel (k_fp_s); DCMT_FUSE_FP=0 keeps k_fill_s + k_post_s
    int top_table = 1;                // k_pre leaves the extension zones of X6 unwritten, k_fp_s clamps its rows and starts below the top one; DCMT_TOP_TABLE=0 disables
    int pair = 1;                     // two columns per lane in H2..H6 (k_pre_p) where the width is even; DCMT_PAIR=0 keeps k_pre_s
    int bands = 0;                    // row bands per strip in k_pre_p (0 = by batch size); DCMT_BANDS
    int fbands = 0;                   // row bands per strip in k_fp_s (0 = by batch size); DCMT_FBANDS
    int fp_q16 = 1;                   // X6 as 16-bit codes + k_fp_q wherever the frames allow it (multiples of 1/256 m: checked on the device, the f32
                                      // kernels rerun behind a raised flag); DCMT_FP_Q16=0 disables
    int assume_filled = 1;            // k_fp_s / k_fp_q without the median >= thr select where the redo chain follows; DCMT_ASSUME_FILLED=0 keeps it
    int q16_min_waves = 2600;         // ... and the batch is large enough: k_fp_q has half as many, longer waves than k_fp_s (3 per SIMD instead of 4), so it
                                      // only pays from about one round of them on (measured, 352x1216, frames per call, whole step against the f32 kernels:
                                      // 128 -12 %, 256 +3 %, 512 +4 %, 1024 +5 %; threshold = 236 frames); DCMT_Q16_MIN_WAVES
    int bbox_global = 0;              // LC fast path: the bounding-box pass without its per-workgroup LDS table; DCMT_BBOX_GLOBAL (set to anything)
    int label_group = 0;              // LC fast path, two columns per lane: labels side by side per wave (0 = by label size); DCMT_LABEL_GROUP
    int label_pairs = -1;             // LC fast path: one wave per label pair (1), per label (0), by label size (-1); DCMT_LABEL_PAIRS
    int min_fused_batch = 3;          // smaller batches use the staged kernels (measured crossover with both streaming kernels in row bands,
                                      // tools/batch_sweep.py: 1 frame 20.6 k staged / 17.1 k streaming, 2 frames 34.7 k / 34.0 k, 3 frames 39.5 k / 50.4 k,
                                      // 4 frames 42.6 k / 65.7 k, 8 frames 52 k / 124 k frames/s); DCMT_MIN_FUSED_BATCH
    int local_bands = 0;              // row bands per strip in k_local (0 = by batch size); DCMT_LOCAL_BANDS
};

// how a variable's text becomes the member: 'i' its integer value, '1' whether it starts with '1', 'p' whether it is set at all
struct KnobEnv { const char* name; int Knobs::* member; char parse; };
constexpr KnobEnv kKnobEnv[] = {
    {"DCMT_POISON", &Knobs::poison, '1'},
    {"DCMT_XCD_MAP", &Knobs::xcd_map, 'i'},
    {"DCMT_WIDE", &Knobs::wide, 'i'},
    {"DCMT_FUSE_FP", &Knobs::fuse_fp, 'i'},
    {"DCMT_TOP_TABLE", &Knobs::top_table, 'i'},
    {"DCMT_PAIR", &Knobs::pair, 'i'},
    {"DCMT_BANDS", &Knobs::bands, 'i'},
    {"DCMT_FBANDS", &Knobs::fbands, 'i'},
    {"DCMT_FP_Q16", &Knobs::fp_q16, 'i'},
    {"DCMT_ASSUME_FILLED", &Knobs::assume_filled, 'i'},
    {"DCMT_Q16_MIN_WAVES", &Knobs::q16_min_waves, 'i'},
    {"DCMT_BBOX_GLOBAL", &Knobs::bbox_global, 'p'},
    {"DCMT_LABEL_GROUP", &Knobs::label_group, 'i'},
    {"DCMT_LABEL_PAIRS", &Knobs::label_pairs, 'i'},
    {"DCMT_MIN_FUSED_BATCH", &Knobs::min_fused_batch, 'i'},
    {"DCMT_LOCAL_BANDS", &Knobs::local_bands, 'i'},
};

inline Knobs knobs_from_env()
{
    Knobs k;
    for (const KnobEnv& e : kKnobEnv) {
        const char* v = std::getenv(e.name);
        if (v) k.*e.member = e.parse == 'i' ? std::atoi(v) : e.parse == '1' ? v[0] == '1' : 1;
    }
    return k;
}

// ---- constants of the decision ------------------------------------------------------------------------------------------
constexpr int TH = 32, TW = 64;
constexpr int FTH_FEW = 16;          // tile height of the staged kernels for a handful of frames: twice the workgroups, a shorter
                                     // critical path (a single frame's 209 tiles of 32 rows leave a fifth of the CUs idle)
constexpr int kFewFrames = 12;       // ... below this many frames; measured up to 8 frames (tools/batch_sweep.py): +15 % at 3 and 6, +7 % at 8
// output columns per wave of the streaming kernels (owners: PreP, PreS, FpQ, PostS, FillS in the kernel headers)
constexpr int kK0AsCompiled = 0, kK0Diamond = 1;
constexpr int pre_p_vw(int k0kind, bool start4) { return start4 ? 120 : k0kind == kK0AsCompiled ? 108 : 104; }
constexpr int pre_s_vw(int k0kind, bool wide) { return k0kind == kK0AsCompiled ? (wide ? 44 : 48) : (wide ? 40 : 46); }
constexpr int kFpQVW = 120, kPostSVW = 56, kFillSVW = 34;
constexpr int local_vw(int k0kind) { return k0kind == kK0AsCompiled ? 40 : 38; }   // LocalS::VW (k_local, dcmt_kernels_local.h)
constexpr int kLocalReach = 13;      // LocalS::REACH: input rows an output row of k_local needs above and below it
// k_local runs in row bands up to about kLocalBandWaves waves, in bands of at least kLocalMinBandRows rows (a band streams up to
// 20 + 14 rows beside its own) and at most kLocalMaxBands of them (measured, tools/time_no_extrapolate.py --bands, 352x1216: one
// frame 1 / 4 / 11 / 22 / 32 / 44 bands 146 / 47 / 26 / 20 / 19 / 20 us, eight frames 1 / 4 / 9 / 11 / 32 bands 148 / 48 / 46 / 40 / 60 us)
constexpr int kLocalBandWaves = 2560, kLocalMinBandRows = 16, kLocalMaxBands = 32;
constexpr int kMaxBands = 8;         // row bands per strip of k_pre_p (table slots per frame)
constexpr int kLabelGroupMax = 4;    // labels one wave of k_label_stage_p may be given
constexpr int kPreBandWaves = 2560;  // k_pre_p runs in row bands up to about this many waves (also sizes the band table in dcmt_create)
constexpr int kFpSOneBandWaves = 2048, kFpSBandWaves = 3072;   // k_fp_s: one band from the first on, else bands up to about the second
// Q16::params_ok: the 16-bit codes are built on the reference's constants
constexpr bool q16_params_ok(float max_depth, float thr) { return max_depth == 100.0f && thr == 0.1f; }
// dcmt.h: dcmt_stage and the DCMT_FLAG_* bits
constexpr int kStageNormalize = 1, kStageClose5 = 4, kStageFill7 = 5, kStageExtend = 6, kStageMedian5 = 9, kStageBlur = 10, kStageFinal = 11;
constexpr int kFlagForceStaged = 1, kFlagForceFused = 2, kFlagNormalize = 4, kFlagNoExtrapolate = 8;
// dcmt_last_path of a call whose result went to scratch first and was then copied to its overlapping dst
constexpr const char* kPathCopy = " + copy to dst";

// ---- one call -----------------------------------------------------------------------------------------------------------
enum class Input { F32, U16, LABELED };      // LABELED: f32 frames with a label plane that is used (use_superpixel)

struct Call {
    int rows = 0, cols = 0, batch = 0;
    Input input = Input::F32;
    int n_labels = 0;
    uintptr_t src = 0, dst = 0, labels = 0;  // device addresses (src: the f32 or uint16 frames)
    float in_scale = 1.0f;                   // metres per uint16 unit
    // dcmt_params; k0 as its preset (k0_preset: -1 = none), blur as the effective one (the labeled entry points force the Gaussian)
    float max_depth = 100.0f, valid_thresh = 0.1f;
    int k0kind = kK0AsCompiled;
    bool gaussian = true;
    bool bilateral = false;                  // DCMT_BLUR_BILATERAL_CLONE (never with gaussian)
    bool valid = false;                      // DCMT_BLUR_GAUSSIAN_VALID (never with gaussian or bilateral; the labeled entry points keep it)
    int max_fill_iters = 64, spec_fill_iters = 1, stop_after = kStageFinal, flags = 0;
    bool sync_loop = false;                  // host entry points: the hole counters are read back between applications
    bool q16_allowed = false;                // a 16-bit attempt is allowed now (the context's skip state, dcmt.hip: q16_allowed_now)
    bool capturing = false;                  // the call's stream is being captured into a graph: its kernels run later, on every replay
};

enum class Route { NORMALIZE_ONLY, STAGED, LABEL_PROBE, STREAMING, LOCAL };     // LOCAL: k_local (DCMT_FLAG_NO_EXTRAPOLATE)
enum class Out { DST, X5, PP0 };             // where the kernel that reads the frames writes what is (so far) the call's result

struct Plan {
    Route route = Route::STAGED;
    int k0kind = kK0AsCompiled;      // the preset the streaming and label kernels are instantiated for (-1: none, staged)
    bool norm = false;               // N1 in front: k_minmax + k_norm_coef, applied by the first kernel that loads the frames
    int xcd_map = 0;                 // the XCD map, for this batch
    Out out = Out::DST;              // != DST: an overlapping call's probe goes to scratch and one copy moves it to dst
    bool needs_x6q = false, needs_colstat = false, needs_bbox = false;   // scratch to have before anything is enqueued
    // staged tile kernels
    bool few = false;
    int tile_h = TH, tiles_x = 0, tiles_y = 0;   // grid of the staged kernels (and the column statistics' tile rows)
    bool u16_convert = false;        // uint16 frames converted into pp[0] first
    int dump = 0;                    // the stage k_pre*_v1 dumps (stop_after <= CLOSE5)
    // label stage (LC fast path)
    bool bbox_lds = false, lpair = false, label_pairs = false;
    int label_group = 1, label_grid_x = 0;
    // streaming kernels
    bool table = false;              // X6 through the per-column (first, last) table
    bool wide = false, pair = false, q16 = false;
    bool q16_own_flag = false;       // the 16-bit attempt of a captured call: its flag is the context's one flag behind the ring, cleared by a
                                     // node in front of the call's kernels on every replay, and it clears no flag for a next attempt
    int bands = 1, fb_s = 1;         // row bands of k_pre_p (= table slots per frame) / of k_fp_s
    int pre_strips = 0, fill_strips = 0, post_strips = 0, q_strips = 0;
    unsigned pre_grid = 0, fill_grid = 0, post_grid = 0, fp_s_grid = 0, fp_q_grid = 0;
    bool fuse_fp = false;            // H7..H11 in k_fp_* (the whole chain only)
    bool filled = false, tail = false, fp_s_launch = false;
    int n_redo = 0;
    // the bilateral finish: everything above is the plan of the same call with stop_after = MEDIAN5 and the context's median plane as
    // its dst; k_bilateral5 then reads that plane and writes dst, with the final invert for stop_after = FINAL
    bool bilateral = false, bilateral_invert = false;
    // the Gaussian that ignores holes.  With the extrapolation it is planned like the bilateral finish: the chain to MEDIAN5 into the
    // median plane, then k_gauss5<VALID> from there into dst (gauss_valid, and its invert for stop_after = FINAL).  Without it
    // (no_extrapolate below) it is a kind of the kernel that finishes the call: valid_kind, k_local<.., VALID> / k_post_v1<.., VALID>
    bool gauss_valid = false, gauss_valid_invert = false;
    bool valid_kind = false;
    // DCMT_FLAG_NO_EXTRAPOLATE from stop_after = MEDIAN5 on: H6..H8 do not run.  Route::LOCAL: k_local, every strip in local_bands row
    // bands; Route::STAGED: k_pre*_v1 into X5, k_post_v1 from there
    bool no_extrapolate = false;
    int local_bands = 1, local_strips = 0;
    unsigned local_grid = 0;
    char path[160] = "";             // dcmt_last_path
};

// [a, a + a_bytes) and [b, b + b_bytes) share a byte: a completion call's input frames and its dst (in place, or overlapping)
inline bool ranges_overlap(uintptr_t a, size_t a_bytes, uintptr_t b, size_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

// grid of the kernels that deal (frame, strip) pairs to waves in one flat sequence (wave_strip in dcmt_kernels_fused.h)
inline unsigned wave_grid(int strips, int batch, int xcd_map)
{
    return xcd_map ? 8 * (((batch / 8) * strips + 3) / 4) : (batch * strips + 3) / 4;
}

inline void path_append(char (&path)[160], const char* s)
{
    size_t n = 0;
    while (path[n]) ++n;
    while (*s && n + 1 < sizeof path) path[n++] = *s++;
    path[n] = 0;
}

// Which kernels run.  The streaming kernels give one wave a whole column strip: a handful of frames cannot fill the GPU
// with them, there the staged tile kernels (hundreds of small workgroups per frame) win
// DCMT_FLAG_NO_EXTRAPOLATE takes effect from stop_after = MEDIAN5 on (up to FILL7 the call is the same with and without it; the
// stages between do not exist with it and are refused before a call is planned)
inline bool no_extrapolate(const Call& c) { return (c.flags & kFlagNoExtrapolate) && c.stop_after >= kStageMedian5; }

inline Route route_of(const Knobs& k, const Call& c)
{
    if ((c.flags & kFlagNormalize) && c.stop_after == kStageNormalize) return Route::NORMALIZE_ONLY;
    if (no_extrapolate(c)) {
        // k_local wherever the streaming kernels' other conditions hold, at every batch size: its row bands need no table, so a
        // single frame fills the GPU with them
        const bool local = !(c.flags & kFlagForceStaged) && c.k0kind >= 0 && c.rows >= 8 && c.cols >= 8 &&
                           (c.input != Input::LABELED || c.n_labels > 0);
        return local ? Route::LOCAL : Route::STAGED;
    }
    const bool big_enough = c.batch >= k.min_fused_batch || (c.flags & kFlagForceFused);
    const bool streaming = !(c.flags & kFlagForceStaged) && big_enough && c.k0kind >= 0 && c.rows >= 8 && c.cols >= 8;
    if (!streaming) return Route::STAGED;
    if (c.input == Input::LABELED) {
        if (c.n_labels > 0 && c.stop_after == kStageFinal) return Route::STREAMING;
        return c.n_labels > 0 && c.stop_after == kStageClose5 ? Route::LABEL_PROBE : Route::STAGED;
    }
    return c.stop_after >= kStageExtend ? Route::STREAMING : Route::STAGED;
}

// Context scratch (X5 / X6, pp[0], pp[1]) is 256-byte aligned; address 0 below stands for it.
inline Plan plan_call(const Knobs& k, const Call& c)
{
    if (c.bilateral && c.stop_after >= kStageBlur) {
        // The chain as for stop_after = MEDIAN5 on whatever route that takes, into the context's median plane (neither pp[0] nor
        // pp[1] is free: a frame's loop result lies in either, by the number of applications it needed), then one more kernel, the
        // call's only writer of dst -- behind every kernel that reads the frames, so an overlapping dst needs no copy.
        Call m = c;
        m.bilateral = false; m.gaussian = false;
        m.stop_after = kStageMedian5;
        m.dst = 0;
        Plan p = plan_call(k, m);
        p.bilateral = true;
        p.bilateral_invert = c.stop_after == kStageFinal;
        path_append(p.path, " + bilateral5");
        return p;
    }
    if (c.valid && c.stop_after >= kStageBlur && !no_extrapolate(c)) {
        // as above, with k_gauss5<VALID> as the last kernel.  (Without the extrapolation the finish is part of the kernel that reads X5: below.)
        Call m = c;
        m.valid = false; m.gaussian = false;
        m.stop_after = kStageMedian5;
        m.dst = 0;
        Plan p = plan_call(k, m);
        p.gauss_valid = true;
        p.gauss_valid_invert = c.stop_after == kStageFinal;
        path_append(p.path, " + gauss5_valid");
        return p;
    }
    Plan p;
    const int stop = c.stop_after, rows = c.rows, cols = c.cols, batch = c.batch;
    const size_t n_px = (size_t)batch * rows * cols;
    const bool u16 = c.input == Input::U16, labeled = c.input == Input::LABELED;
    p.route = route_of(k, c);
    p.k0kind = c.k0kind;
    p.norm = (c.flags & kFlagNormalize) != 0;
    p.xcd_map = (k.xcd_map && batch % 8 == 0) ? 1 : 0;
    // In place (or overlapping) calls: every kernel that writes dst must run behind the last one that reads the input frames.  Where
    // the kernel that reads them would also write dst (the probes), an overlapping call points its output at scratch the path does
    // not use at that point and copies it to dst (kPathCopy in dcmt_last_path).
    bool overlap = ranges_overlap(c.src, n_px * (u16 ? 2 : 4), c.dst, n_px * 4);

    if (p.route == Route::NORMALIZE_ONLY) {
        // k_norm_write is a grid-stride pass: with a shifted overlap it would overwrite frames other threads have yet to read.
        // Overlapping: into pp[0] (no other kernel of this call) and copied.
        p.out = overlap ? Out::PP0 : Out::DST;
        path_append(p.path, "k_minmax + k_norm_coef + k_norm_write");
        if (p.out != Out::DST) path_append(p.path, kPathCopy);
        return p;
    }

    if (labeled && p.route != Route::STAGED) {
        // LC fast path: bounding boxes -> one wave per label (masked H2..H4) -> X4 -> the img_completion kernels
        // (dead before the redo chain writes pp[0]; x5 shares pp[1]).  The CLOSE5 probe is X4 itself, written straight to dst --
        // unless dst overlaps src: the label stage's waves read src around their label's box (wide boxes in column chunks, a
        // later chunk reading what an earlier one wrote) while others write X4, so X4 stays in pp[0] and is copied
        p.needs_bbox = true;
        const bool to_dst = p.route == Route::LABEL_PROBE && !overlap;
        const uintptr_t x4 = to_dst ? c.dst : 0;
        p.bbox_lds = sizeof(int) * 4 * (size_t)c.n_labels <= 48 * 1024 && !k.bbox_global;
        // two columns per lane (k_label_stage_p) where a lane's 8-byte accesses are aligned; G labels side by side per wave, from the
        // mean label area (a grown box of w + 10 columns takes (w + 10) / 2 + 1 lanes; SLIC-like labels are a few columns wider
        // than the square root of their area)
        p.lpair = k.pair && cols % 2 == 0 && cols >= 8 && c.src % 8 == 0 && c.labels % 8 == 0 && x4 % 8 == 0;
        const double w = std::sqrt((double)rows * cols / c.n_labels) + 4.0;
        const int lanes = (int)((w + 10.0) / 2.0) + 1;
        int G = (64 + lanes / 4) / (lanes > 0 ? lanes : 1);        // as many as fit side by side, rounded up when they nearly do (the rest gets a pass of its own)
        if (G < 1) G = 1;
        if (G > kLabelGroupMax) G = kLabelGroupMax;
        if (k.label_group >= 1 && k.label_group <= kLabelGroupMax) G = k.label_group;
        p.label_group = G;
        // labels of about 22 columns or less (the mean box of an even partition, with SLIC-like slack) can share a
        // wave: one wave per label PAIR; few large labels: one wave per label (see k_label_stage_s)
        p.label_pairs = k.label_pairs >= 0 ? k.label_pairs != 0 : (double)rows * cols / c.n_labels <= 22.0 * 22.0;
        p.label_grid_x = p.lpair ? ((c.n_labels + G - 1) / G + 3) / 4 : p.label_pairs ? (c.n_labels + 7) / 8 : (c.n_labels + 3) / 4;
        if (p.route == Route::LABEL_PROBE) {
            p.out = to_dst ? Out::DST : Out::PP0;
            path_append(p.path, "k_label_bbox + k_label_stage");
            if (p.out != Out::DST) path_append(p.path, kPathCopy);
            return p;
        }
        overlap = false;         // the streaming kernels read X4 in pp[0]
    }

    if (p.route == Route::LOCAL) {
        // One kernel from the frames (uint16 ingest and N1 applied while it loads; labeled: from X4 in pp[0]) to dst.  It writes
        // dst while other waves still read their halo rows and columns from the frames: an overlapping call writes pp[0] -- free,
        // because no fill runs -- and one copy follows (labeled: the kernel reads X4, not the frames, and needs none)
        p.no_extrapolate = true;
        p.out = overlap ? Out::PP0 : Out::DST;
        const int vw = local_vw(c.k0kind);
        p.local_strips = (cols + vw - 1) / vw;
        // row bands, from the batch size: a band recomputes kLocalReach rows of halo above and below its own
        const long long w1 = (long long)batch * p.local_strips;
        int bands = k.local_bands > 0 ? k.local_bands : (w1 >= kLocalBandWaves ? 1 : (int)((kLocalBandWaves + w1 - 1) / w1));
        if (k.local_bands <= 0) {
            if (bands > rows / kLocalMinBandRows) bands = rows / kLocalMinBandRows;
            if (bands > kLocalMaxBands) bands = kLocalMaxBands;
        }
        if (bands > rows) bands = rows;
        if (bands < 1) bands = 1;
        p.local_bands = bands;
        p.local_grid = wave_grid(p.local_strips * bands, batch, p.xcd_map);
        p.valid_kind = c.valid && stop >= kStageBlur;
        if (labeled) path_append(p.path, "k_label_bbox + k_label_stage + ");
        if (p.valid_kind) path_append(p.path, labeled ? "k_local<START4,VALID>" : u16 ? "k_local<U16,VALID>" : p.norm ? "k_local<NORM,VALID>" : "k_local<VALID>");
        else
        path_append(p.path, labeled ? "k_local<START4>" : u16 ? "k_local<U16>" : p.norm ? "k_local<NORM>" : "k_local");
        if (bands > 1) path_append(p.path, " (row bands)");
        if (p.out != Out::DST) path_append(p.path, kPathCopy);
        return p;
    }

    if (p.route == Route::STREAMING) {
        // Whole chain: k_pre -> k_fp_* -> k_tail (host entry points: k_fill_s redo, k_fill_s applications, k_post_s instead of
        // k_tail); stop_after probes: k_pre -> k_fill_s (-> loop) -> k_post_s.
        const bool cf = p.norm && !labeled;          // N1's (a, b) applied while k_pre loads (the label stage has applied them already)
        const uintptr_t src = labeled ? 0 : c.src;
        // table mode: only the k_fp_* path reads X6 through the per-column table (the probes and the unfused kernels get a fully written X6)
        p.fuse_fp = stop == kStageFinal && k.fuse_fp;
        p.table = p.fuse_fp && k.top_table;
        // Frames that overlap dst: the f32 kernels read them only in k_pre, into scratch, and write dst last.  Two things would break
        // that: the stop_after = EXTEND probe, where k_pre writes dst while other waves still read their strips and halo columns from
        // the frames -- it goes to X6 (this call's k_pre output anyway) and one copy moves it to dst; and the 16-bit attempt, whose
        // k_fp_q writes dst BEFORE the gated f32 rerun reads the frames again -- not taken.
        p.out = stop == kStageExtend && overlap ? Out::X5 : Out::DST;
        const uintptr_t o6 = stop == kStageExtend && !overlap ? c.dst : 0;
        // LDS-DMA rows need 16-byte aligned sources: cols % 4 == 0 and a 16-byte aligned base
        p.wide = k.wide && cols % 4 == 0 && src % 16 == 0 && !u16;
        // two columns per lane (k_pre_p) wherever a lane's 8-byte accesses are aligned: even width, 8-byte aligned frames
        p.pair = k.pair && cols % 2 == 0 && cols >= 8 && src % (u16 ? 4 : 8) == 0 && o6 % 8 == 0;
        // row bands: full-height strips of a small batch leave most wave slots empty; bands need the (ti, bi) table (one slot per
        // band).  (Counted with the as-compiled strip width whatever the element and whatever the input.)
        if (p.pair && p.table) {
            const long long w1 = (long long)batch * ((cols + pre_p_vw(kK0AsCompiled, false) - 1) / pre_p_vw(kK0AsCompiled, false));
            p.bands = k.bands > 0 ? k.bands : (w1 >= kPreBandWaves ? 1 : (int)((kPreBandWaves + w1 - 1) / w1));
            if (p.bands > rows / 32) p.bands = rows / 32 > 0 ? rows / 32 : 1;
            if (p.bands > kMaxBands) p.bands = kMaxBands;
        }
        // 16-bit X6 (k_pre_p<Q16OUT> -> k_fp_q): the whole chain in table mode, two columns per lane, the reference's constants, a
        // batch that is large enough, no normalisation in front (normalised depths are no multiples of 1/256), no overlap of the
        // frames with dst (above).  (The uint16 entry point's depths are multiples of 1/256 m by construction, but a payload beyond
        // 30719 -- 119.996 m -- has no code either: the attempt is checked on the device there too.)
        p.q_strips = (cols + kFpQVW - 1) / kFpQVW;
        p.q16 = k.fp_q16 && c.q16_allowed && (long long)batch * p.q_strips >= k.q16_min_waves && p.pair && p.table && !cf &&
                q16_params_ok(c.max_depth, c.valid_thresh) && c.dst % 8 == 0 && (!u16 || c.in_scale == 0.00390625f) && !overlap;
        p.needs_x6q = p.q16;
        p.q16_own_flag = p.q16 && c.capturing;
        const int vw = p.pair ? pre_p_vw(c.k0kind, labeled) : pre_s_vw(c.k0kind, p.wide);
        p.pre_strips = (cols + vw - 1) / vw;
        p.pre_grid = wave_grid(p.pre_strips * p.bands, batch, p.xcd_map);
        if (labeled) path_append(p.path, "k_label_bbox + k_label_stage + ");
        path_append(p.path, p.q16 ? (u16 ? "k_pre_p<U16,Q16OUT>" : "k_pre_p<Q16OUT>") :
                            p.pair ? (labeled ? "k_pre_p<START4>" : u16 ? "k_pre_p<U16>" : cf ? "k_pre_p<NORM>" : "k_pre_p") : "k_pre_s");
        if (p.bands > 1) path_append(p.path, " (row bands)");
        if (stop == kStageExtend) {
            if (p.out != Out::DST) path_append(p.path, kPathCopy);
            return p;
        }
        p.fill_strips = (cols + kFillSVW - 1) / kFillSVW;
        p.fill_grid = (unsigned)((p.fill_strips + 3) / 4) * batch;
        p.post_strips = (cols + kPostSVW - 1) / kPostSVW;
        p.post_grid = (unsigned)((p.post_strips + 3) / 4) * batch;
        if (!p.fuse_fp) return p;
        // one kernel for H7..H11; frames it leaves with holes are redone by the unfused kernels.
        // row bands for k_fp_s: a batch whose strips are fewer than two waves per SIMD runs every strip as fb_s bands, about one
        // round of three waves per SIMD in all (a band pays 19 + 19 rows of halo and 19 steps of pipeline: only worth it while the
        // GPU is not full -- from ~100 frames of 1216 columns on there is one band)
        if (p.table) {
            const long long w1 = (long long)batch * p.post_strips;
            p.fb_s = k.fbands > 0 ? k.fbands : (w1 >= kFpSOneBandWaves ? 1 : (int)((kFpSBandWaves + w1 / 2) / w1));
            if (p.fb_s > rows / 32) p.fb_s = rows / 32 > 0 ? rows / 32 : 1;
            if (p.fb_s < 1) p.fb_s = 1;
        }
        // frames this kernel leaves with holes are recomputed by the redo chain whenever that chain is enqueued (always on the host
        // entry points, with spec_fill_iters >= 1 on the device ones): then the kernel may leave out the select that only such frames need
        p.filled = c.gaussian && k.assume_filled && (c.sync_loop || (c.spec_fill_iters >= 1 && c.max_fill_iters >= 1));
        p.n_redo = c.sync_loop ? c.max_fill_iters : (c.spec_fill_iters < c.max_fill_iters ? c.spec_fill_iters : c.max_fill_iters);
        // device entry points: everything behind k_fp_* is k_tail (dcmt_kernels_tail.h), also the second half of the f32 rerun behind
        // a 16-bit attempt; the host entry points (and spec_fill_iters = 0, where nothing follows) keep k_fp_s as a launch of its own
        p.tail = !c.sync_loop && p.n_redo > 0;
        p.fp_s_launch = !p.q16 || !p.tail;
        p.fp_q_grid = wave_grid(p.q_strips, batch, p.xcd_map);
        p.fp_s_grid = wave_grid(p.post_strips * p.fb_s, batch, p.xcd_map);
        path_append(p.path, p.q16 ? " + k_fp_q" : (p.fb_s > 1 ? " + k_fp_s (row bands)" : " + k_fp_s"));
        return p;
    }

    // staged tile kernels
    p.needs_colstat = true;
    p.few = batch < kFewFrames;
    p.tile_h = p.few ? FTH_FEW : TH;
    p.tiles_x = (cols + TW - 1) / TW;
    p.tiles_y = (rows + p.tile_h - 1) / p.tile_h;
    p.u16_convert = u16;         // the staged kernels take f32: converted into pp[0], which never overlaps dst
    if (u16) overlap = false;
    p.dump = stop <= kStageClose5 ? stop : 0;
    // Up to FILL7 the kernel that reads the frames writes the probe itself: stages 2..4 as its dump, FILL7 as its X5 output.  Into a
    // dst that overlaps src that would race with other workgroups still reading their halo from src, so the probe goes to
    // scratch and is copied: X5 for FILL7 (its own plane), pp[0] for the dumps (first written by the 31x31 fill, which these probes do
    // not run; the uint16 input converted into pp[0] never overlaps dst).
    p.out = stop <= kStageFill7 && overlap ? (stop == kStageFill7 ? Out::X5 : Out::PP0) : Out::DST;
    path_append(p.path, labeled ? "k_pre_labeled_v1" : "k_pre_v1");
    // (no extrapolation: k_post_v1 reads X5, behind the only kernel that reads the frames -- an overlapping dst needs no copy)
    p.no_extrapolate = no_extrapolate(c);
    p.valid_kind = p.no_extrapolate && c.valid && stop >= kStageBlur;
    path_append(p.path, p.valid_kind ? " + k_post_v1<VALID> (staged tile kernels)" :
                        p.no_extrapolate ? " + k_post_v1 (staged tile kernels)" : " + k_fill31_v1 + k_post_v1 (staged tile kernels)");
    if (p.out != Out::DST) path_append(p.path, kPathCopy);
    return p;
}

}  // namespace plan
}  // namespace dcmt

#endif
