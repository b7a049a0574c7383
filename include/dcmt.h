/*
 * dcmt.h -- C ABI of the MI355X-native (gfx950 / CDNA4) morphological depth-completion
 * cascade.  This is the drop-in boundary for the ONE hot path of
 * PatrizioPerugini/depth_completion_MT:
 *
 *   void img_completion(const cv::Mat&, cv::Mat&, const bool&, const std::string&)
 *        reference: src/DC_lidar_only/img_completion.cpp:17-20
 *   void interpolate_with_superpixels(Slic&, const cv::Mat&, cv::Mat&, const std::string&, int)
 *        reference: src/DC_lidar_camera/img_completion_lc.cpp:34-38
 *
 * The reference has no FFI or plugin registry: those two free-function signatures ARE the
 * interface, and the header that declares them (img_completion.h) is missing from the
 * reference repository.  include/img_completion.h in this repo is that header; it is a
 * thin C++ shim over the entry points below (INTEGRATION.md shows the binding).
 *
 * Plain C: no C++ types, no exceptions, no torch types cross this boundary.  Every
 * function returns DCMT_OK (0) or a negative dcmt_status.  A dcmt_ctx is bound to one
 * GPU and owns all scratch memory; it must not be used from two threads at once (one ctx
 * per GPU per host thread -- frames are independent, so multi-GPU is one ctx per device).
 * Successive *_dev calls on one ctx must be ordered on the device too: the same stream, or streams the caller has ordered with
 * events (a call's kernels use the scratch memory -- and clear flags -- the next call's kernels rely on).  Work that should overlap
 * goes to two contexts.
 *
 * Devices and threads: every entry point that takes a ctx makes ctx's device current for the
 * duration of the call and restores the calling thread's current device before it returns, so
 * one process may drive all GPUs of a node from one host thread per GPU (or from one thread,
 * ctx after ctx) without ever calling hipSetDevice itself.  Device pointers and the stream
 * passed to a *_dev entry point must belong to ctx's device; stream == NULL is that device's
 * default stream.
 *
 * Values: frames must be finite (no NaN, no +-Inf).  The library is built with
 * -ffinite-math-only (its max/min networks drop the NaN-quieting pass), so a NaN or Inf in an
 * input frame gives an unspecified (but memory-safe) result in the pixels its windows reach.
 * The reference's own result for such pixels depends on the min/max flavour of the OpenCV
 * build (SIMD vs scalar), so there is nothing to be bit-exact with.  -0.0 is treated as 0.0.
 *
 * Depth grids: frames whose depths are all multiples of 1/256 m below 120 m -- what a KITTI depth PNG / 256 holds,
 * DC_lidar_only/main.cpp:75-82 -- let large device batches keep their intermediate image as 16-bit integers.  The library
 * finds that out itself on the device (and repeats the step with its f32 kernels when a frame turns out otherwise); results
 * are the same bits either way, and no promise about the values is asked of the caller.  What it costs when the depths are NOT
 * such multiples: a call that makes the attempt runs both of its large kernels twice (the 16-bit attempt, then the f32 kernels
 * behind the flag the attempt raised), and the context then skips the attempt for its next 63 calls before trying once more --
 * arbitrary f32 depths pay one double run in 64 calls.  Depths beyond 119.996 m (inverted values below -20 m: outside the 15-bit code
 * range) count as "not on the grid" as well, also on the uint16 entry point (payloads above 30719).
 *
 * In place: on dcmt_complete_f32_dev, dcmt_complete_u16_dev and dcmt_complete_labeled_f32_dev, d_dst may be d_src (the
 * reference's function is in place by signature: dense = sparse.clone(), :27) or overlap it in any way -- shifted by frames, rows
 * or single elements; on the uint16 entry point d_src's 2 bytes per pixel anywhere inside or across d_dst's 4 -- at every
 * stop_after, with the bits of a call into separate memory.  In an overlapping call every kernel that writes d_dst runs after the
 * last one that reads d_src.  Where the kernel that reads d_src would itself write d_dst (the probes up to DCMT_STAGE_EXTEND, and DCMT_STAGE_NORMALIZE),
 * an overlapping call writes the result to context scratch and copies it to d_dst: one device-to-device copy more, and
 * dcmt_last_path ends in "+ copy to dst".  The 16-bit attempt is not made when d_dst overlaps d_src (f32 or uint16): its rerun would
 * read d_src again after d_dst was written.  The labeled entry point's attempt reads the label stage's output in scratch, so
 * overlap does not stop it there.  All of this holds with DCMT_FLAG_NO_EXTRAPOLATE: there the one kernel that reads d_src
 * (k_local) would write d_dst while other waves still read their halos, so an overlapping call writes to scratch that is free
 * because no fill runs, one copy follows and dcmt_last_path ends in "+ copy to dst"; the labeled entry point's kernel reads the
 * label stage's output and needs no copy, nor do the staged kernels or the bilateral finish.  d_labels must not overlap d_dst.  The host entry points stage through device buffers of their
 * own: src may be dst there too.
 *
 * Graph capture: every *_dev entry point may be called while its stream is being captured into a graph (hipStreamBeginCapture,
 * torch.cuda.graph) and the graph replayed any number of times; each replay gives the bits of the same call made eagerly on what
 * the buffers hold then (tests/test_gpu_graph_replay.py: every entry point, every route of the cascade, whole pipelines as one
 * graph, eager calls on the same context between the replays).  The rules:
 *   - Warm up first: make the same call -- same shapes, batch, parameters, n_labels, step -- once eagerly on that context.  It makes
 *     the documented first-use allocations; a capture in the strict mode (the default) fails on an allocation, and a call that has
 *     to allocate while its stream is capturing returns an error and leaves the capture invalid.  One warm-up is enough on every
 *     route.  A later call that GROWS context scratch (more labels, a smaller SLIC step, a larger projection target: the calls that
 *     say "grown on demand") frees what earlier graphs point to: capture them again.
 *   - One stream: capture a ctx's calls on one stream, as a straight line.  Graphs with parallel branches, captures that fork to
 *     other streams and multi-GPU captures are not supported.  Replays and eager calls on one ctx must be ordered on the device
 *     like any two calls (above); with that, they may be mixed freely.
 *   - What is frozen: every pointer and every by-value argument -- the parameter structs, scales, rows, cols, batch, n_points,
 *     n_labels, T and P of dcmt_project_points_dev, the workspace size -- as it was at capture time.  What is free to change between
 *     replays: the contents of every buffer, the *_calib_dev tables, d_offsets and the label planes among them.
 *   - The 16-bit form (above) of a captured call uses a flag of its own, cleared by a node in front of its kernels, and does not
 *     take part in the context's 63-call back-off: it is attempted on every replay, so a graph that is fed depths off the 1/256 m
 *     grid runs both large kernels twice every time.  Capture with DCMT_FP_Q16=0 in dcmt_create's environment for such data.  A frame
 *     off the grid in a replay still sends the context's EAGER calls into their back-off.
 *   - dcmt_project_points_dev, dcmt_reproject_depth_dev and their _calib twins clear the context's winner plane on every replay (a
 *     memset node of 4 bytes per output pixel of the largest such call so far), which their eager form does once in 255 calls.
 *   - dcmt_last_fill_iters and dcmt_last_holes_after_extend after a replay report THAT replay, once the caller has synchronised
 *     the stream the graph was launched on (they wait for the stream the call was captured on, not for the replay's; a replay on
 *     the capture stream needs no more).  While the last call's stream is capturing they return DCMT_E_INVALID: nothing has run.
 *     dcmt_last_path names the captured route; after a dcmt_rectify_dev it copies from the device, so it must not be called while
 *     a capture is open, and its route suffix describes the last rectify call made through the API only while no graph holding
 *     an older one has been replayed since.
 *   - Refused while the stream is capturing, with DCMT_E_INVALID and before anything is enqueued: a completion call with
 *     dcmt_set_kernel_timing on (its events would be recorded into the graph, not timed) or with params->verbose set.
 *   - The host (synchronous) entry points synchronise by design and stay eager-only.
 * What a replayed graph saves over eager calls (launch cost at batch 1-8, where it dominates) and what the extra clear and the
 * unconditional attempt cost has not been measured.
 * Empty pixels: the sign of a zero in an output pixel that stays empty (an all-empty frame) is +0.0 where the input held +0.0; an
 * input -0.0 counts as 0.0 (empty) and may come out as either zero.
 */
#ifndef DCMT_H
#define DCMT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCMT_VERSION 120 /* 0.1.2: dcmt_last_path; verbose == 2 (hole counts only: interpolate_with_superpixels) */

typedef struct dcmt_ctx dcmt_ctx;

typedef enum {
    DCMT_OK              = 0,
    DCMT_E_INVALID       = -1, /* bad argument (null pointer, size beyond the ctx limits, empty k0) */
    DCMT_E_UNSUPPORTED   = -2, /* blur == DCMT_BLUR_BILATERAL: the reference's call throws too (img_completion.cpp:174);
                                  stop_after = 6..8 with DCMT_FLAG_NO_EXTRAPOLATE: those stages do not exist then */
    DCMT_E_NOMEM         = -3, /* device or host allocation failed */
    DCMT_E_HIP           = -4, /* a HIP runtime call failed; dcmt_last_hip_error() has the code */
    DCMT_E_NOT_CONVERGED = -5, /* the hole-closure loop (img_completion.cpp:146-166) hit max_fill_iters with holes left */
    DCMT_E_NO_DEVICE     = -6  /* no gfx950 device visible / wrong architecture */
} dcmt_status;

typedef enum {
    DCMT_BLUR_NONE      = 0, /* any blur_type string other than the two below */
    DCMT_BLUR_GAUSSIAN  = 1, /* "gaussian": GaussianBlur 5x5 sigma 0 + masked select (img_completion.cpp:176-189) */
    DCMT_BLUR_BILATERAL = 2, /* "bilateral": rejected with DCMT_E_UNSUPPORTED */
    /* "bilateral_clone": what img_completion.cpp:174 computes when it is given a copy (an opt-in of this project; the reference's own
     * in-place call throws): after the 5x5 median, cv::bilateralFilter(clone, dense, 5, 1.5, 2.0) over the WHOLE plane (:174 has no
     * masked select, unlike the Gaussian's :184), as dcmt_bilateral5_dev states it, then the unchanged final invert.  With
     * stop_after >= DCMT_STAGE_BLUR the chain runs as for stop_after = DCMT_STAGE_MEDIAN5 on every route (the median plane goes to a
     * context plane that the first such call allocates, never to d_dst), then one more kernel writes d_dst, as the call's only and
     * last writer: every promise of the "In place" paragraph above holds.  dcmt_last_path ends in "+ bilateral5".  stop_after <=
     * DCMT_STAGE_MEDIAN5 ignores the blur, as with every value.  The labeled entry points force the Gaussian whatever this is. */
    DCMT_BLUR_BILATERAL_CLONE = 3,
    /* "gaussian_valid": the Gaussian that ignores holes (an opt-in of this project; normalised convolution), X10 = GV(X9) as
     * dcmt_gaussian5_valid_dev states GV, then the unchanged final invert.  Made for DCMT_FLAG_NO_EXTRAPOLATE, whose X9 is full of holes:
     * there DCMT_BLUR_GAUSSIAN averages a valid pixel next to a hole with the hole's zeros (a pixel 10 m away, 90 in inverted space,
     * becomes about 45 and the output says 55 m), along every border of the completed region.  On a plane without holes it is
     * DCMT_BLUR_GAUSSIAN bit for bit.  With the flag it is part of the one kernel (k_local) or of the staged post kernel.  Without
     * the flag it is planned as DCMT_BLUR_BILATERAL_CLONE is: the chain as for stop_after = DCMT_STAGE_MEDIAN5 into the context's
     * median plane, then one more kernel, the call's only and last writer of d_dst; dcmt_last_path ends in "+ gauss5_valid".  There it
     * differs from DCMT_BLUR_GAUSSIAN only in a frame whose hole-closure loop hit max_fill_iters.  stop_after <= DCMT_STAGE_MEDIAN5
     * ignores it, as with every value.  The labeled entry points honour it (every other value they replace by the Gaussian). */
    DCMT_BLUR_GAUSSIAN_VALID = 5 /* (4 is no blur and stays refused with DCMT_E_INVALID, as every value outside this enum) */
} dcmt_blur;

/* Stages of the cascade, for `stop_after` (parity probes; 11 = the whole chain). */
typedef enum {
    DCMT_STAGE_NORMALIZE = 1, /* only with DCMT_FLAG_NORMALIZE: the min-max normalised frames themselves
                                 (cv::normalize in front of the path, DC_stereo_lidar/main_sl.cpp:370, :523) */
    DCMT_STAGE_INVERT   = 2,  /* img_completion.cpp:55-67   */
    DCMT_STAGE_DILATE_K = 3,  /* :71-80   first dilate, element k0 */
    DCMT_STAGE_CLOSE5   = 4,  /* :84-85   5x5 close (LC: the label-masked stage, img_completion_lc.cpp:78-102) */
    DCMT_STAGE_FILL7    = 5,  /* :88-100  7x7 small-hole fill */
    DCMT_STAGE_EXTEND   = 6,  /* :103-129 column extension */
    DCMT_STAGE_FILL31   = 7,  /* :131-144 31x31 large-hole fill */
    DCMT_STAGE_FILLLOOP = 8,  /* :146-166 repeat until no holes */
    DCMT_STAGE_MEDIAN5  = 9,  /* :170     5x5 median */
    DCMT_STAGE_BLUR     = 10, /* :172-189 blur + masked select (DCMT_BLUR_BILATERAL_CLONE: the filter, no select) */
    DCMT_STAGE_FINAL    = 11  /* :191-202 invert back to metres */
} dcmt_stage;

/* All literals of the reference in one POD (SURVEY.md section 5 "Config / flags").
 * Domain of the two numeric fields: max_depth finite; valid_thresh finite and > 0 (0, -0.0 and negative values are refused:
 * every producer writes 0 for "no point" and the label stage writes 0 outside a label, which only means "empty" below a positive
 * threshold).  Every dcmt_complete_* entry point returns DCMT_E_INVALID otherwise, tested on the bit patterns, before anything
 * is allocated or enqueued.
 * The column extension's fill values for a column without a valid pixel, 100 and -1 (img_completion.cpp:109-110), are literals
 * of the reference, not its max_depth: they do not follow max_depth.
 * The 16-bit form of the streaming kernels (k_pre_p<Q16OUT> -> k_fp_q) is built on the reference's constants and is attempted
 * only at max_depth == 100 and valid_thresh == 0.1f; every other pair takes the f32 kernels. */
typedef struct {
    float   max_depth;       /* 100.0f                    img_completion.cpp:23 */
    float   valid_thresh;    /* 0.1f: valid <=> x >= valid_thresh, hole <=> x < valid_thresh.
                                The reference writes `depth > 0.1` / `depth < 0.1` against the DOUBLE
                                literal; for f32 inputs that is exactly x >= 0.1f / x < 0.1f. */
    uint8_t k0[25];          /* first structuring element, row-major 5x5, anchor centre, non-zero = tap.
                                Default: what the reference COMPILES to (2 taps), see dcmt_k0_as_compiled. */
    uint8_t _pad[3];
    int32_t blur;            /* dcmt_blur */
    int32_t max_fill_iters;  /* cap on the hole-closure loop (reference: unbounded); default 64 */
    int32_t spec_fill_iters; /* device-pointer entry points only: how many loop applications are enqueued
                                speculatively without a host round trip (each is skipped on the device for
                                frames that have no holes left).  Default 1.  If a frame still has holes
                                after them, dcmt_last_fill_iters() reports DCMT_E_NOT_CONVERGED for it. */
    int32_t stop_after;      /* dcmt_stage; DCMT_STAGE_FINAL for the whole chain */
    int32_t verbose;         /* host entry points: 1 = print what img_completion prints to stdout (dimensions :29, "max range is" :50, one
                                hole count per loop iteration :161); 2 = the hole counts only (all that interpolate_with_superpixels
                                prints, img_completion_lc.cpp:173); 0 = nothing */
    int32_t flags;           /* DCMT_FLAG_* */
    float   norm_lo;         /* DCMT_FLAG_NORMALIZE: the two range arguments of cv::normalize (alpha, beta); */
    float   norm_hi;         /* the stereo-lidar callers pass (0, 100) and (0, 80).  Defaults 0, 100. */
} dcmt_params;

/* Use the general staged kernels even where the fused fast path applies (A/B tests, debugging).
 * Both paths produce identical bits. */
#define DCMT_FLAG_FORCE_STAGED 1
/* Use the fused streaming kernels even for a batch too small to fill the GPU with them (by default
 * batches of fewer than 3 frames take the staged tile kernels, whose many small workgroups have the
 * lower latency for a single frame).  Both paths produce identical bits. */
#define DCMT_FLAG_FORCE_FUSED 2

/* The caller-side pre-step of the stereo-lidar executables fused in front of the cascade: every frame is first
 * min-max normalised, exactly as `cv::normalize(src, dst, norm_lo, norm_hi, cv::NORM_MINMAX)` does for a
 * CV_32F destination (DC_stereo_lidar/main_sl.cpp:370 before img_completion, :523 before
 * interpolate_with_superpixels): one extra read-only pass finds each frame's extrema, the first kernel of
 * the chain applies dst = src * a + b (f32, unfused) while it loads.  f32 entry points only
 * (dcmt_complete_u16_dev returns DCMT_E_UNSUPPORTED: the reference never combines the two ingests).
 * A frame whose values are all equal normalises to min(norm_lo, norm_hi) everywhere, as in OpenCV. */
#define DCMT_FLAG_NORMALIZE 4

/* The cascade without its extrapolation (an opt-in of this project).  The reference's signature has `const bool& extr` and never
 * reads it: the column extension and both large fills (img_completion.cpp:103-166, img_completion_lc.cpp:119-180) run under
 * `int densify = true;`.  Without the flag nothing changes, and the drop-in interfaces' `extr` argument stays ignored, as the
 * reference ignores it.  With the flag stages 6..8 do not exist: with X5 the plane after DCMT_STAGE_FILL7 exactly as without the
 * flag (the labeled entry point's label-masked stage, the uint16 ingest, DCMT_FLAG_NORMALIZE, either k0 preset or a custom k0
 * included), thr = valid_thresh and "valid" x >= thr,
 *     X9  = medianBlur5(X5)                                  (:170, replicated border)
 *     X10 = DCMT_BLUR_GAUSSIAN:        X9 >= thr ? GaussianBlur5(X9) : X9   (:178-188, reflect-101; forced by the labeled entry points)
 *           DCMT_BLUR_NONE:            X9
 *           DCMT_BLUR_GAUSSIAN_VALID:  GV(X9), as dcmt_gaussian5_valid_dev states it: weights from the valid taps only (honoured by the
 *                                      labeled entry points too)
 *           DCMT_BLUR_BILATERAL_CLONE: bilateral5(X9) over the whole plane, as dcmt_bilateral5_dev states it
 *           DCMT_BLUR_BILATERAL:       DCMT_E_UNSUPPORTED, as always
 *     X11 = X10 >= thr ? max_depth - X10 : X10               (:191-202)
 * A pixel whose median is valid but whose blurred value falls below thr is not inverted: those are the reference's statements.
 * X9 is full of holes here, and DCMT_BLUR_GAUSSIAN (the default) averages every valid pixel that has a hole among its 25 taps with
 * that hole's zeros, in inverted space: the depth along every border of the completed region comes out too large, by tens of metres
 * at worst.  DCMT_BLUR_GAUSSIAN_VALID is the finish that does not.
 * stop_after <= DCMT_STAGE_FILL7: the call without the flag, bit for bit (the flag is ignored).  DCMT_STAGE_EXTEND, _FILL31 and
 * _FILLLOOP: DCMT_E_UNSUPPORTED before anything is enqueued.  DCMT_STAGE_MEDIAN5, _BLUR, _FINAL: X9, X10, X11.
 * max_fill_iters and spec_fill_iters are ignored; dcmt_last_fill_iters and dcmt_last_holes_after_extend report 0 for every frame,
 * with DCMT_OK; verbose = 1 prints the reference's two header lines and no hole counts, verbose = 2 nothing.
 * Two consequences: an all-zero frame stays all zero (nothing is invented far from a measurement: no column-top values above the
 * highest lidar ring), and a frame whose X5 has no hole gives the bits of the call without the flag (there the extension and both
 * fills change nothing).
 * The cascade is then a local stencil (13 rows either way, 11 columns to the left, 13 to the right): wherever the streaming
 * kernels' other conditions hold (a k0 preset, rows and cols >= 8, no DCMT_FLAG_FORCE_STAGED) one kernel, k_local, reads the
 * frames once and writes d_dst once, at every batch size; otherwise the staged kernels run without the fill.  The 16-bit form is
 * never taken.  Every route gives the same bits; the call never synchronises and allocates nothing the call without the flag
 * would not. */
#define DCMT_FLAG_NO_EXTRAPOLATE 8

/* ---- lifetime --------------------------------------------------------------------- */

/* Number of usable devices (0 if none); never fails. */
int dcmt_device_count(void);

/* Creates a context on `device` able to process up to max_batch frames of up to
 * max_rows x max_cols per call.  Allocates the device scratch every path needs up front (8 B per
 * pixel per frame of max_batch); two buffers only one path uses are allocated by the first call that takes it and kept (the
 * 16-bit plane of large on-grid batches, 2 B per pixel; the column statistics of the small-batch tile kernels); SLIC scratch and
 * the partial-sum slab of the evaluate calls are allocated the same way by the first call that needs them, so no call
 * after the first of its kind allocates.  The min/max slab of dcmt_colorize* (8 B per 8192 pixels of a frame, times max_batch)
 * and the count slab of dcmt_depth_to_cloud* (16 B per 8192 pixels, times max_batch) are allocated here; the strip slab of
 * dcmt_slic_connectivity_dev (4 B per 64 columns of max_cols, times max_batch) by the first call of it.  A frame may hold at most 2^29 - 16 pixels (it is addressed with 32-bit byte offsets
 * and one offset just below 2^31 is kept free as "nowhere"); max_batch at most 65535. */
int dcmt_create(int device, int max_rows, int max_cols, int max_batch, dcmt_ctx **out);
void dcmt_destroy(dcmt_ctx *ctx);

/* ---- parameters ------------------------------------------------------------------- */

void dcmt_default_params(dcmt_params *p);
/* The element the reference's `cv::Mat(5,5,CV_8UC1,d)` over `int d[5][5]` really is
 * (img_completion.cpp:71-77): taps at (row 1,col 3) and (row 4,col 4) only. */
void dcmt_k0_as_compiled(uint8_t k0[25]);
/* The 13-tap radius-2 diamond the reference's comment intends. */
void dcmt_k0_diamond(uint8_t k0[25]);

/* ---- img_completion --------------------------------------------------------------- */

/* HOST pointers, synchronous: copies in, runs the cascade, copies out.  Backs the cv::Mat
 * shim (replaces the body of img_completion, img_completion.cpp:17-204).
 * src/dst: f32, `batch` frames of rows x cols; row and frame strides in BYTES (cv::Mat::step
 * for a single Mat; frame strides are ignored when batch == 1).  src is never written (unless it is dst: in place works).
 * The hole-closure loop runs exactly as many times as the reference would (up to
 * max_fill_iters); returns DCMT_E_NOT_CONVERGED if the cap was hit (dst is still written). */
int dcmt_complete_f32(dcmt_ctx *ctx,
                      const float *src, size_t src_row_stride, size_t src_frame_stride,
                      float *dst, size_t dst_row_stride, size_t dst_frame_stride,
                      int rows, int cols, int batch, const dcmt_params *params);

/* DEVICE pointers, stream-ordered, asynchronous: the measured path.  d_src/d_dst are
 * contiguous [batch][rows][cols] f32 in device memory of ctx's GPU; `stream` is a
 * hipStream_t (NULL = the default stream).  Never synchronises; never allocates (the labeled variant
 * grows its per-label bounding-box table the first time it sees a larger batch x n_labels). */
int dcmt_complete_f32_dev(dcmt_ctx *ctx, const float *d_src, float *d_dst,
                          int rows, int cols, int batch, const dcmt_params *params, void *stream);

/* The reference's ingest fused into the first kernel: d_src holds the KITTI uint16 depth PNG payload
 * ([batch][rows][cols], device memory), metres = value * scale -- what src/DC_lidar_only/main.cpp:75-82
 * does with imread(IMREAD_ANYDEPTH) + convertTo(CV_32F, 1./256) before calling img_completion.  Reads
 * 2 instead of 4 bytes per pixel; otherwise identical to dcmt_complete_f32_dev on the converted frame. */
int dcmt_complete_u16_dev(dcmt_ctx *ctx, const uint16_t *d_src, float scale, float *d_dst,
                          int rows, int cols, int batch, const dcmt_params *params, void *stream);

/* ---- interpolate_with_superpixels -------------------------------------------------- */

/* As above with a label plane: int32 [rows][cols] ROW-MAJOR per frame (the reference keeps
 * Slic::clusters[col][row]; the shim transposes), labels outside [0,n_labels) (e.g. -1)
 * are not touched by the masked stage.  use_superpixel == 0 runs the unmasked first stage
 * (img_completion_lc.cpp:59-64).  The Gaussian is applied whatever params->blur says, as in
 * the reference (img_completion_lc.cpp:183 ignores blur_type). */
int dcmt_complete_labeled_f32(dcmt_ctx *ctx,
                              const float *src, size_t src_row_stride, size_t src_frame_stride,
                              const int32_t *labels, size_t lab_row_stride, size_t lab_frame_stride,
                              int n_labels,
                              float *dst, size_t dst_row_stride, size_t dst_frame_stride,
                              int rows, int cols, int batch, const dcmt_params *params,
                              int use_superpixel);
int dcmt_complete_labeled_f32_dev(dcmt_ctx *ctx, const float *d_src, const int32_t *d_labels,
                                  int n_labels, float *d_dst, int rows, int cols, int batch,
                                  const dcmt_params *params, int use_superpixel, void *stream);

/* ---- producer of the path's input: LiDAR points -> sparse depth image (N2) ----------- */

/* What the stereo-lidar executables do between reading the velodyne .bin and calling the path
 * (DC_stereo_lidar/main_sl.cpp:478-520 in withSuperPixels, the same loop at :320-366 in vedi_pc):
 *     t = T * (x, y, z, 1)                 keep the point if t.z > 0                    (:480-490)
 *     p = P * (t.x, t.y, t.z, 1);  uf = p.x / p.z,  vf = p.y / p.z                      (:499-503)
 *     if 0 <= uf < cols and 0 <= vf < rows:  image(int(vf), int(uf)) = p.z              (:506-518)
 * in file order, so a later point overwrites an earlier one that fell into the same pixel.
 * d_points: device, [n_points][4] f32 = x, y, z, reflectance -- the KITTI .bin layout the reference reads (:468-472),
 * 16-byte aligned (every device allocation is; the records are read whole): DCMT_E_INVALID otherwise;
 * frame f owns points [d_offsets[f], d_offsets[f+1]) (device array of batch+1 ints, d_offsets[batch] == n_points).
 * T: 4x4, P: 3x4, both ROW-major host arrays (Eigen's default storage is column-major: pass the transposes' data()).
 * d_sparse: [batch][rows][cols] f32, written completely (0 = no point).  All arithmetic is f32, one rounding per
 * operation, sums left to right -- the order of the reference's hand-written transform; Eigen's evaluation order for
 * `P * p.homogeneous()` is not pinned, so against a real build a point whose uf or vf sits
 * within an ulp of an integer may land in the neighbouring pixel.  Stream-ordered, never synchronises; uses ctx
 * scratch (the winner plane, shared with dcmt_reproject_depth_dev: see there), so do not overlap it with another call
 * on the same ctx.  The closest point instead of the last: dcmt_project_points_nearest_dev, below. */
int dcmt_project_points_dev(dcmt_ctx *ctx, const float *d_points, const int32_t *d_offsets, int n_points,
                            int batch, const float T[16], const float P[12], float *d_sparse,
                            int rows, int cols, void *stream);

/* ---- producer of the label plane: SLIC superpixels (N3) -------------------------------- */

/* Slic::generate_superpixels (DC_lidar_camera/slic.cpp:101-182; called at main_lc.cpp:200 with 1200 superpixels and
 * DC_stereo_lidar/main_sl.cpp:450 with 100) on the device: the grid of centres moved to their 3x3 gradient minimum
 * (init_data :19-57), then NR_ITERATIONS = 10 rounds of "every pixel of a centre's [c - step, c + step) window takes the
 * centre with the smallest distance (compute_dist :59-68, f64), the lowest index on ties" and "every centre becomes the
 * mean of its pixels".  d_lab: [batch][rows][cols][3] uint8 -- the image the reference passes (its cv::cvtColor(BGR2Lab)
 * output: what dcmt_bgr_convert_dev writes from the camera's BGR bytes, on the same stream); step, nc: the reference's int arguments (step = (int)sqrt(w*h / n_superpixels), nc = 50 / 40).
 * d_labels: [batch][rows][cols] int32, row-major (the reference's clusters[col][row]), -1 = never reached: exactly what
 * dcmt_complete_labeled_f32_dev takes, with n_labels = dcmt_slic_num_centers(rows, cols, step).
 * d_centers (may be NULL): [batch][n][5] f64 = L, a, b, x, y after the last iteration.
 * The first call allocates SLIC scratch (per-centre and per-cell tables, a few hundred KiB per frame of max_batch);
 * later calls with the same or a larger step never allocate.
 * Requires step >= 6 (below that the reference's gradient probe reads outside the image) and nc >= 1. */
int dcmt_slic_num_centers(int rows, int cols, int step);
int dcmt_slic_labels_dev(dcmt_ctx *ctx, const uint8_t *d_lab, int rows, int cols, int batch, int step, int nc,
                         int32_t *d_labels, double *d_centers, void *stream);

/* Slic::create_connectivity (DC_lidar_camera/slic.cpp:186-254; called at main_lc.cpp:202 between generate_superpixels and
 * interpolate_with_superpixels) on the device: the connectivity pass of SLIC.  The label plane is relabelled so that every label is
 * one 4-connected region, and fragments smaller than a quarter of a superpixel take the label of a neighbour.  An OPT-IN: the
 * reference computes this relabelling into a local (new_clusters) that nothing reads, so its own results are those of the raw
 * k-means labels; call this between dcmt_slic_labels_dev and dcmt_complete_labeled_f32_dev to get what was intended.
 * The reference's sequential, order-dependent statements, as the data-parallel definition that gives the same labels.  A frame is
 * labels[rows][cols] int32 row-major (the reference's clusters[col][row]); x is the column, y the row, s(x, y) = x * rows + y the
 * reference's scan order (column outer, row inner):
 *   components  a component is a maximal 4-connected set of pixels with equal input label; any int32 compares, -1 ("never
 *               reached") and values >= n_centers included (:227 compares with == and nothing else)
 *   seed        a component's pixel with the smallest s
 *   count       size + (size >= 2 ? 1 : 0): the reference never marks the seed, reaches it again and counts it twice (:207, :227-230)
 *   threshold   lims = (rows * cols) / n_centers (integer division; n_centers is the reference's centers.size(), what
 *               dcmt_slic_num_centers returns); a component is SMALL iff count <= lims >> 2 (:238).  lims >= 4 is required (below
 *               that a one-pixel component is not small and the reference leaves -1 in it)
 *   non-small   its label is the number of non-small components whose seed has a smaller s (the reference's running `label`)
 *   small       of the seed's neighbours (x-1, y), (x, y-1), (x+1, y), (x, y+1), in this order, those inside the frame whose
 *               component's seed has a smaller s than this seed (the pixels already labelled when the scan arrives) are kept; the
 *               LAST of them is the neighbour (:210-219), and the component takes the FINAL label of that neighbour's component
 *               (chains of small components follow links to strictly smaller seeds until they reach a non-small one).  With no
 *               such neighbour -- only the component of pixel (0, 0) -- it takes label 0, the reference's initial adjlabel
 *   d_counts    [batch] or NULL: the number of non-small components of each frame.  Every output label lies in
 *               [0, max(1, count)), and count <= max(1, (rows * cols) / ((lims >> 2) + 1)) because a non-small component holds
 *               more than lims >> 2 pixels: dcmt_slic_connectivity_max_labels returns this bound (it needs no GPU; DCMT_E_INVALID
 *               where the call refuses the shape), and the caller passes it as n_labels to dcmt_complete_labeled_f32_dev with no
 *               host round trip.  Where the component of (0, 0) is small, label 0 can be shared by two regions: the reference's quirk.
 * Two places where this leaves the reference's text: :226 bounds y by image.cols, which on a landscape image indexes
 * new_clusters[x] past its end (undefined behaviour) -- y is bounded by rows here, as :213 does; and the result is stored.
 * Integer arithmetic throughout: the result is bit-exact and does not depend on the batch size, the frame's position in the batch,
 * alignment, the launch geometry or the run.
 * d_labels / d_out: [batch][rows][cols] int32, 4-byte aligned.  d_out == d_labels is allowed and gives the bits of an out-of-place
 * call (the last kernel is the only writer of d_out and reads no labels); any other overlap among d_labels, d_out and d_counts is
 * DCMT_E_INVALID, as are null pointers, sizes beyond the context's limits, n_centers < 1, lims < 4 and misaligned pointers.
 * Stream-ordered, never synchronises, a fixed number of launches (seven; six for a frame of at most 64 x 16 pixels): nothing the host
 * does depends on the data.  Scratch: the two planes dcmt_create allocates (8 B per pixel; the ones the in-place dcmt_gaussian5_dev
 * borrows, which every completion call rewrites before it reads them) and a slab of 4 B per 64 columns of max_cols, times
 * max_batch, which the first call of this kind allocates before it enqueues anything.  Of the context's carried state it touches
 * none: no flag ring, no winner plane, no bounding-box tables, no dcmt_last_path or probe.  Same standing behind other *_dev calls
 * as dcmt_depth_to_cloud_dev. */
int dcmt_slic_connectivity_max_labels(int rows, int cols, int n_centers);
int dcmt_slic_connectivity_dev(dcmt_ctx *ctx, const int32_t *d_labels, int rows, int cols, int batch, int n_centers,
                               int32_t *d_out, int32_t *d_counts /* [batch] or NULL */, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES); labels may be out. */
int dcmt_slic_connectivity(dcmt_ctx *ctx, const int32_t *labels, size_t row_stride, int rows, int cols, int n_centers,
                           int32_t *out, size_t out_row_stride, int32_t *count /* or NULL */);

/* Slic::display_contours (DC_lidar_camera/slic.cpp:337-384; slic.display_contours(image, CV_RGB(200,0,0)) at main_lc.cpp:214, the
 * first image the reference shows) and Slic::colour_with_cluster_means (slic.cpp:392-433; its call at main_lc.cpp:249 is commented
 * out) on the device: the two pixel renderings of a label plane.  Slic::display_center_grid (cv::circle) is not reproduced.
 * A frame is labels[rows][cols] int32 row-major (the reference's clusters[col][row]); x is the column, y the row.
 *
 * CONTOURS.  The reference scans x outer, y inner and keeps a matrix istaken; a pixel is TAKEN iff at least 2 of its 8 neighbours
 * are inside the frame, have a different label and are not taken yet (:357-372).  Any int32 compares, -1 and values >= n_centers
 * included (:363 uses != and nothing else).  Its sequential, order-dependent statements, as the definition that gives the same
 * bits.  The scan has visited four of the neighbours, the EARLIER ones (x-1, y-1), (x-1, y), (x-1, y+1), (x, y-1); the LATER ones
 * (x+1, y-1), (x+1, y), (x+1, y+1), (x, y+1) are never taken yet.  Per pixel:
 *   A      the number of in-frame later neighbours with a different label
 *   c      A + the number of in-frame pixels among (x-1, y-1), (x-1, y), (x-1, y+1) with a different label that are NOT taken
 *   taken  where (x, y-1) is outside the frame or has the same label: c >= 2.  Otherwise: c >= 2 -> taken; c == 0 -> not taken;
 *          c == 1 -> !taken(x, y-1).
 * So taken(x, y-1) -> taken(x, y) is a constant or a negation, never the identity: inside a column a maximal run of c == 1 pixels
 * under differing upper pixels alternates, taken(y) = taken(base) XOR ((y - base) & 1) with base the pixel just above the run, and
 * column x needs three bits per pixel of column x - 1.  Taken pixels of d_bgr get the bytes colour_bgr[0..2] = B, G, R
 * ((uchar)colour[0..2], :380-381; CV_RGB(200,0,0) is {0, 0, 200}); no other byte of d_bgr is written.  d_mask gets 255 where taken, 0
 * elsewhere.  At least one of d_bgr, d_mask must be given; colour_bgr is a HOST pointer, read before the call returns.
 *
 * CLUSTER MEANS.  For each label k in [0, n_labels): the sums of B, G and R over the frame's pixels with label k and their count (on the
 * raw k-means labels the count is what the reference's center_counts[k] holds, :142-163); every such pixel becomes sum / count per
 * channel.  The reference divides doubles and converts to uchar implicitly, with no saturate_cast: for a quotient in [0, 255] that
 * is truncation, so this is INTEGER DIVISION.  A pixel whose label is outside [0, n_labels) indexes `colours` out of bounds in the
 * reference (undefined behaviour): here it keeps its bytes and is not counted.  d_sums, [batch][n_labels][4] = sumB, sumG, sumR,
 * count as 32-bit words (labels that own no pixel: zeros), or NULL.  In place on d_bgr: the sums are complete before a byte is written.
 *
 * Both: integer arithmetic throughout, so the result is bit-exact and does not depend on the batch size, the frame's position in
 * the batch, the launch geometry or the run.  d_labels 4-byte aligned, d_sums 4-byte aligned.  DCMT_E_INVALID: null inputs (labels;
 * both outputs of the contours; the colour; d_bgr of the means), sizes beyond the context's limits, misaligned pointers, ANY overlap
 * among d_labels, d_bgr, d_mask / d_sums, and
 *   contours  rows > 262144 (the column pass keeps one 64-bit mask per 64 rows of a column in 32 KiB of LDS)
 *   means     n_labels < 1; batch * n_labels * 16 bytes more than ONE of the two scratch planes holds, that is
 *             n_labels > (max_rows * max_cols * max_batch) / (4 * batch) of dcmt_create's arguments -- with d_sums given as well,
 *             so that a call's validity does not depend on it; rows * cols * 255 >= 2^32 (the sums are 32-bit)
 * Stream-ordered, never synchronise, never allocate, three launches each whatever the data.  Scratch: the two planes dcmt_create
 * allocates (the ones dcmt_slic_connectivity_dev borrows, which every completion call rewrites before it reads them): 1 B per pixel
 * of code bytes in one and 1 B per pixel of taken bytes in the other for the contours, the sums in the first where d_sums is NULL
 * for the means.  Of the context's carried state they touch none.  Same standing behind other *_dev calls as
 * dcmt_slic_connectivity_dev. */
int dcmt_slic_contours_dev(dcmt_ctx *ctx, const int32_t *d_labels, int rows, int cols, int batch,
                           uint8_t *d_bgr /* [batch][rows][cols][3], painted in place, or NULL */, const uint8_t colour_bgr[3],
                           uint8_t *d_mask /* [batch][rows][cols], 255 taken / 0 not, or NULL */, void *stream);
int dcmt_slic_cluster_means_dev(dcmt_ctx *ctx, const int32_t *d_labels, int rows, int cols, int batch, int n_labels,
                                uint8_t *d_bgr /* [batch][rows][cols][3], in place */,
                                int32_t *d_sums /* [batch][n_labels][4] = sumB, sumG, sumR, count; or NULL */, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES).  bgr (or NULL) is painted in place, mask (or NULL) written. */
int dcmt_slic_contours(dcmt_ctx *ctx, const int32_t *labels, size_t row_stride, int rows, int cols, uint8_t *bgr, size_t bgr_row_stride,
                       const uint8_t colour_bgr[3], uint8_t *mask, size_t mask_row_stride);
int dcmt_slic_cluster_means(dcmt_ctx *ctx, const int32_t *labels, size_t row_stride, int rows, int cols, int n_labels, uint8_t *bgr,
                            size_t bgr_row_stride, int32_t *sums /* [n_labels][4] or NULL */);

/* ---- per-superpixel plane fitting of sparse depth ------------------------------------------------------ */

/* Image-guided completion of a sparse depth plane from a label plane (dcmt_slic_labels_dev, dcmt_slic_connectivity_dev): one
 * superpixel is, to first order, one planar facet, and a planar facet seen by a pinhole camera is AFFINE IN INVERSE DEPTH over the
 * pixel coordinates.  So every label gets one least-squares plane of inverse depth through the returns that fall in it, and the
 * label's pixels are painted with it.  A label without a return stays empty: nothing is invented.  Not in the reference; stated
 * here to the last bit.  An opt-in between the labels and dcmt_complete_*_dev, which then fills only what the planes left open.
 * u is the column, v the row.  Per frame:
 *
 * RETURN.  A pixel is a return of label k iff its label is k with 0 <= k < n_labels and its depth z is a finite float with
 *   valid_thresh <= z <= max_depth, decided on the bit pattern: NaN, +-inf, negatives and -0.0 are no returns.
 * CODE.  w = (uint32) rne(W / z): one correctly rounded f32 division with W = 65536.0f, then round to nearest even.  With
 *   valid_thresh >= 0.0625 and max_depth <= 16384 (both enforced) 4 <= w <= 2^20.
 * MOMENTS.  Per label, over its returns, as exact integers: n, Su, Sv, Suu, Suv, Svv, Sw, Suw, Svw (the sums of 1, u, v, u u, u v,
 *   v v, w, u w, v w) and the minima and maxima of u, v and w.  Integer adds commute: nothing below depends on the batch size, the
 *   frame's position in the batch, the launch geometry or the run.
 *   Bounds.  rows * cols <= 2^21 is enforced.  Then n <= 2^21 and, with u < cols, v < rows: Suu <= rows cols cols^2 < 2^63 (the
 *   largest of the sums: a frame of one row), Suw, Svw < 2^21 2^21 2^20 = 2^62: the sums are kept in unsigned 64-bit words.  The
 *   centred terms below are formed in 128-bit integers: |n Suw| and |Su Sw| < 2^21 2^62 = 2^83; Cuu <= n^2 (cols-1)^2 / 4 and Cvv
 *   likewise, so Cuu Cvv <= n^4 ((cols-1)(rows-1))^2 / 16 < 2^84 2^42 / 16 = 2^122, and Cuv^2 <= Cuu Cvv (Cauchy-Schwarz): the
 *   determinant is exact in a signed 128-bit integer, and "collinear" is an exact decision.
 * FIT.  With a label's moments, in this order:
 *   n = 0: kind NONE.
 *   wbar = f64(Sw) / f64(n)                                  (every f64 operation here rounded once, no contraction; f64(i) is the
 *                                                             integer i rounded to the nearest double, ties to even)
 *   Exact integers: Cuu = n Suu - Su Su, Cuv = n Suv - Su Sv, Cvv = n Svv - Sv Sv, Cuw = n Suw - Su Sw, Cvw = n Svw - Sv Sw,
 *   D = Cuu Cvv - Cuv Cuv: n^2 times the centred normal matrix, right-hand side and determinant.  Centring is what makes this
 *   well conditioned at u ~ 1200.
 *   kind PLANE iff n >= min_points and umax - umin + 1 >= min_extent and vmax - vmin + 1 >= min_extent and D > 0; then
 *     a = (f64(Cuw) f64(Cvv) - f64(Cvw) f64(Cuv)) / f64(D)
 *     b = (f64(Cvw) f64(Cuu) - f64(Cuw) f64(Cuv)) / f64(D)
 *     c = (wbar - a (f64(Su) / f64(n))) - b (f64(Sv) / f64(n))
 *   otherwise kind CONSTANT: a = b = +0.0, c = wbar.
 *   The fit at a pixel is w^(u, v) = (a f64(u) + b f64(v)) + c; for a constant that is c.
 * TRIMMED REFIT, where refit_tol > 0, for the labels whose first fit is a plane: the moments are accumulated a second time over only
 *   the returns with |f64(w) - w^| <= f64(refit_tol) w^ (w^ the first fit at that pixel, not clamped; the product rounded once) and
 *   fitted by the same rules.  If that fit is a plane it replaces the first, with the trimmed set's count, wmin and wmax; if not,
 *   the first fit stands.  One refit, not an iteration.
 * OUTPUT.  A pixel whose label is outside [0, n_labels) or of kind none: +0.0f, whatever its depth (it is no return of any label).
 *   A return, with keep_returns: its own bits.  Every other pixel of a label with a fit, and a return without keep_returns:
 *   (float)(65536.0 / clamp(w^(u, v), f64(wmin), f64(wmax))), an f64 division rounded to f32; wmin and wmax are the extremes of the
 *   codes of the returns the final fit used, so a plane never leaves its label's measured range.
 * d_fits, or NULL: [batch][n_labels] records dcmt_plane_fit of 48 bytes; a label of kind none (one that owns no pixel, or no return)
 *   gets zeros.  seen: the label's returns; used: those the final fit used.
 *
 * DEVICE pointers, stream-ordered; never synchronises, never allocates; four launches (clear, sum, solve, paint) and seven with a
 * refit (clear, sum and solve a second time), whatever the data.  d_out may BE d_depth: the moments are complete before a pixel is
 * written, and the result has the bits of an out-of-place call.  Scratch: the two planes dcmt_create allocates (the ones
 * dcmt_slic_cluster_means_dev borrows): the moment records, 96 bytes a label, in the first; the fits in the second where d_fits is
 * NULL.  Of the context's carried state it touches none: same standing behind other *_dev calls as dcmt_slic_cluster_means_dev.
 * DCMT_E_INVALID, nothing written: a null ctx, depth, labels, output or params; sizes beyond the context's limits; rows * cols > 2^21;
 * d_depth, d_labels or d_out not 4-byte aligned, d_fits not 8-byte aligned; any overlap among the buffers other than d_out == d_depth
 * exactly; n_labels < 1 or batch * n_labels * 96 bytes more than ONE scratch plane holds, that is n_labels >
 * (max_rows * max_cols * max_batch) / (24 * batch) of dcmt_create's arguments, with d_fits given as well; valid_thresh not finite or
 * < 0.0625; max_depth not finite, < valid_thresh or > 16384; min_points < 3; min_extent < 1; refit_tol not finite, < 0 or >= 1;
 * keep_returns neither 0 nor 1. */
typedef struct {
    float   valid_thresh;   /* 0.1   the smallest depth that is a return, metres; >= 0.0625                        */
    float   max_depth;      /* 100   the largest; <= 16384                                                         */
    int32_t min_points;     /* 3     returns a plane needs; >= 3                                                   */
    int32_t min_extent;     /* 2     columns and rows the returns of a plane must span, in pixels; >= 1            */
    float   refit_tol;      /* 0     0: no refit; else the relative tolerance of the trimmed refit, in (0, 1)      */
    int32_t keep_returns;   /* 1     1: a return keeps its bits; 0: it is painted like its label's other pixels    */
} dcmt_planes_params;       /* 24 bytes */
typedef struct {
    double   a, b, c;       /* w^ = a u + b v + c, in codes (65536 / metres)                                       */
    uint32_t seen, used;    /* the label's returns; those of the final fit                                         */
    uint32_t wmin, wmax;    /* the extremes of the codes the final fit used                                        */
    uint32_t kind;          /* 0 none, 1 constant, 2 plane                                                         */
    uint32_t reserved;      /* 0                                                                                   */
} dcmt_plane_fit;           /* 48 bytes */
#define DCMT_PLANES_NONE 0
#define DCMT_PLANES_CONSTANT 1
#define DCMT_PLANES_PLANE 2
void dcmt_default_planes_params(dcmt_planes_params *p);
int dcmt_superpixel_planes_max_labels(int max_rows, int max_cols, int max_batch, int batch);
int dcmt_superpixel_planes_dev(dcmt_ctx *ctx, const float *d_depth, const int32_t *d_labels, int rows, int cols, int batch, int n_labels,
                               const dcmt_planes_params *params, float *d_out /* may be d_depth */,
                               dcmt_plane_fit *d_fits /* [batch][n_labels] or NULL */, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES, >= 4 * cols); out may be depth; fits [n_labels] or NULL.  The same
 * bits as the device call.  What dcmt_shim::fit_superpixel_planes calls. */
int dcmt_superpixel_planes(dcmt_ctx *ctx, const float *depth, size_t depth_row_stride, const int32_t *labels, size_t labels_row_stride,
                           int rows, int cols, int n_labels, const dcmt_planes_params *params, float *out, size_t out_row_stride,
                           dcmt_plane_fit *fits);

/* ---- occlusion filter of projected LiDAR returns ------------------------------------------------------- */

/* The LiDAR and the camera sit in different places, so a sweep holds returns from surfaces the camera cannot see; projected, those
 * background returns land inside the silhouette of the foreground object that hides them, between its own returns.
 * dcmt_project_points_nearest_dev settles only two points on the SAME pixel; a background return one pixel beside a foreground one
 * survives, and the cascade, the planes above and the guided matcher all take it at its word.  This call removes from a sparse depth
 * plane every return that a nearer return in a small window shows to be hidden.  Not in the reference; stated here to the last bit:
 * all integers after one division per return.  It belongs between the projection and dcmt_complete_*_dev,
 * dcmt_superpixel_planes_dev and dcmt_sgm_guided_dev.  Per frame, on an f32 plane [rows][cols]:
 *
 * RETURN.  A pixel is a return iff its depth z is a finite float with valid_thresh <= z <= max_depth, decided on the bit pattern
 *   exactly as dcmt_superpixel_planes_dev decides it: NaN, +-inf, negatives and -0.0 are no returns.
 * CODE.  w = (uint32) rne(65536.0f / z): the planes' code (one correctly rounded f32 division, then round to nearest even).  With
 *   valid_thresh >= 0.0625 and max_depth <= 16384 (both enforced, as there) 4 <= w <= 2^20.  A pixel that is no return has code 0.
 * WINDOW MAXIMUM.  m(y, x) = the largest code over the pixels (y + dy, x + dx) with |dy| <= ry, |dx| <= rx that lie inside the
 *   frame.  The window is clipped: no border replication, and it never reaches into another frame of the batch.
 * OCCLUDED.  A return is occluded iff m - w > tol_code, in integers.  Every decision is taken on the INPUT plane: a return that is
 *   itself removed still hides others, so the result depends on no order.
 * OUTPUT.  An occluded return becomes +0.0f.  Every other pixel, the pixels that are no returns included, keeps its bits.
 * d_removed, or NULL: uint32 [batch], the number of pixels changed per frame.
 * Nothing depends on the batch size, the frame's position in the batch, alignment, the launch geometry, the run, or on whether
 * the call is in place.
 *
 * Why inverse depth: a planar surface is affine in inverse depth over the image, so a fixed tolerance in codes does not eat slanted
 * surfaces at range; a relative tolerance in metres does (on a ground plane 1.65 m below the camera, neighbouring rings at 50 m
 * differ by 20 % in depth).  The defaults are derived, not tuned.  rx = 3, ry = 6: an HDL-64's ring spacing of 0.4 deg is 5.04 rows
 * at KITTI's focal length of 721.5 and its azimuth step at most 2.3 columns, so the window holds a foreground return wherever the
 * foreground covers it.  tol_code = 655 (0.01 / m): a ground plane 1.65 m below the camera changes by 55 codes a row, 330 over
 * ry = 6: a margin of 2; and a background return whose gap to the foreground is below the tolerance is misplaced by under 0.01 f b ~ 2 pixels for a
 * sensor offset b of 0.3 m.  valid_thresh and max_depth are the planes' defaults.
 *
 * The payload form, dcmt_sparse_occlusion_u16_dev, is the same filter on the KITTI uint16 payload dcmt_complete_u16_dev ingests:
 * the depth of a payload value v is what that ingest states, the f32 product (float) v * scale rounded once; an occluded return
 * becomes 0.  The same kernels, instantiated on the element type.
 *
 * DEVICE pointers, stream-ordered; never synchronises, never allocates.  Out of place: one launch, which decides and writes.  In
 * place (d_out == d_sparse): two, because a neighbouring workgroup may already have zeroed what another still has to read: the
 * decisions go to a mask of one bit per pixel, then they are applied.  A clear of d_removed goes in front where it is given.  Both
 * routes give the same bytes.  Scratch: the first of the two planes dcmt_create allocates (the ones dcmt_slic_connectivity_dev and
 * dcmt_filter_speckles_dev borrow), in place only.  Of the context's carried state it touches none, dcmt_last_path included: it can
 * be queued in front of or behind any other *_dev call.
 * DCMT_E_INVALID, nothing written: a null ctx, plane, output or params; sizes or a batch beyond the context's limits; rx outside
 * 0..8, ry outside 0..16, tol_code outside 0..2^20; valid_thresh not finite or < 0.0625; max_depth not finite, < valid_thresh or
 * > 16384; scale not finite or <= 0 (the payload form); planes not aligned to their element, d_removed not 4-byte aligned; any
 * overlap among the buffers other than d_out == d_sparse exactly. */
typedef struct {
    int32_t rx;             /* 3     half width of the window, columns; 0..8                                       */
    int32_t ry;             /* 6     half height of the window, rows; 0..16                                        */
    int32_t tol_code;       /* 655   a return is occluded where the window's largest code exceeds its own by more  */
                            /*       than this; in codes of 1 / 65536 per metre (655 = 0.01 / m); 0..2^20          */
    float   valid_thresh;   /* 0.1   the smallest depth that is a return, metres; >= 0.0625                        */
    float   max_depth;      /* 100   the largest; <= 16384                                                         */
} dcmt_occlusion_params;    /* 20 bytes */
void dcmt_default_occlusion_params(dcmt_occlusion_params *p);
int dcmt_sparse_occlusion_dev(dcmt_ctx *ctx, const float *d_sparse, float *d_out /* may be d_sparse */, int rows, int cols, int batch,
                              const dcmt_occlusion_params *params, uint32_t *d_removed /* [batch] or NULL */, void *stream);
int dcmt_sparse_occlusion_u16_dev(dcmt_ctx *ctx, const uint16_t *d_sparse, float scale /* 1./256 for KITTI */,
                                  uint16_t *d_out /* may be d_sparse */, int rows, int cols, int batch,
                                  const dcmt_occlusion_params *params, uint32_t *d_removed /* [batch] or NULL */, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES, >= 4 * cols); out may be sparse; removed: one count or NULL.  The
 * same bits as the device call.  What dcmt_shim::filter_occluded_returns calls. */
int dcmt_sparse_occlusion(dcmt_ctx *ctx, const float *sparse, size_t sparse_row_stride, float *out, size_t out_row_stride, int rows, int cols,
                          const dcmt_occlusion_params *params, uint32_t *removed);

/* ---- distance to the nearest LiDAR return, and the trust mask ------------------------------------------ */

/* Every call that produces a dense plane (the cascade, dcmt_superpixel_planes_dev, the Gaussian and bilateral finishes, dcmt_sgm_dev
 * with its fallback depth) invents depth where nothing was measured, and none of them tells the consumer which pixels rest on a
 * measurement.  This call gives the support map of a sparse plane: for every pixel the exact squared Euclidean distance to the
 * nearest return; and one use of it fused behind: keep a dense plane within a trust radius of a return and write zero, or a second
 * plane (the stereo matcher's depth, say), beyond it.  Not in the reference; stated here to the last bit: integers throughout.  Per
 * frame, on a sparse plane [rows][cols]:
 *
 * RETURN.  Exactly the occlusion filter's rule above (dcmt_sparse_occlusion_dev), decided on the bit pattern: a finite float with
 *   valid_thresh <= z <= max_depth; NaN, +-inf, negatives and -0.0 are no returns.  The same bounds are enforced:
 *   valid_thresh >= 0.0625, max_depth <= 16384.
 * DISTANCE.  D2(y, x) = the minimum over the returns (y', x') of the same frame of (y - y')^2 + (x - x')^2, in integers: 0 at a
 *   return, infinite in a frame without returns.  It never reaches into another frame of the batch.
 * d_dist2, or NULL: uint16 [batch][rows][cols].  D2 where D2 <= R^2, R = max_radius in 1..255, and 65535 everywhere else:
 *   255^2 = 65025 < 65535, so the marker is never a distance, and no value between R^2 + 1 and 65534 is ever written.
 * d_out, or NULL: f32 [batch][rows][cols]; needs d_dense.  A pixel takes the four bytes of d_dense where D2 <= R^2; elsewhere the
 *   four bytes of d_fallback, or +0.0f where d_fallback is NULL.  The copy is opaque: a NaN keeps its bits.  d_out may BE d_dense.
 * d_beyond, or NULL: uint32 [batch], the pixels of the frame with D2 > R^2.
 * At least one of d_dist2 and d_out must be given; d_fallback without d_out is refused.
 * Nothing depends on the batch size, the frame's position in the batch, alignment, the launch geometry, the run, or on whether
 * the call is in place.
 *
 * The default R = 9 is the reach of H3..H5 (2 + 4 + 3): beyond it no value of the plane behind the 7x7 fill depends on
 * a measurement except through the column extension and the 31x31 fills.  Checked against the kernels of the no-extrapolation
 * cascade (dcmt_kernels_local.h, dcmt_kernels_fused.h): that holds for the plane behind H5, whose rows lag the input by PreS::LAT = 9
 * and whose strips lose PreS::HR = 2 + 2 + 2 + 3 = 9 columns, and it is a reach PER AXIS, a box of 19 x 19: the disc of R = 9 lies
 * inside it, so the default trusts nothing H3..H5 could not have reached, and leaves out the box's corners (up to 9 sqrt(2) = 12.7
 * away).  The FINISHED plane of that cascade reaches further: LocalS::REACH = 13 rows, the median and the Gaussian adding 2 + 2 (and
 * 4 columns either side); max_radius = 13 covers it in the same sense.
 *
 * The payload form, dcmt_support_distance_u16_dev, takes the sparse plane as the KITTI uint16 payload dcmt_complete_u16_dev ingests:
 * the depth of a payload value v is what that ingest states, the f32 product (float) v * scale rounded once.  Dense, fallback and
 * out stay f32.  The same kernels, instantiated on the element type.
 *
 * DEVICE pointers, stream-ordered; never synchronises, never allocates.  Two launches, in place or not: the distance in rows to the
 * nearest return of every pixel's own column, capped at R + 1 and kept as uint16 (so that 255 is told from "none within reach" on one
 * route for every R); then the minimum along the row, which writes d_dist2, selects into d_out and counts.  A clear of d_beyond goes
 * in front where it is given: three.  Scratch: the first of the two planes dcmt_create allocates (the one the occlusion filter,
 * dcmt_slic_connectivity_dev and dcmt_filter_speckles_dev borrow), half of it.  Of the context's carried state it touches none,
 * dcmt_last_path included: it can be queued in front of or behind any other *_dev call.
 * DCMT_E_INVALID, nothing written: a null ctx, sparse plane or params; neither d_dist2 nor d_out; d_out without d_dense; d_fallback
 * without d_out; sizes or a batch beyond the context's limits; max_radius outside 1..255; valid_thresh not finite or < 0.0625;
 * max_depth not finite, < valid_thresh or > 16384; scale not finite or <= 0 (the payload form); a plane not aligned to its element,
 * d_beyond not 4-byte aligned; any overlap among the buffers other than d_out == d_dense exactly. */
typedef struct {
    int32_t max_radius;     /* 9     R: distances up to R^2 are reported and trusted; 1..255                       */
    float   valid_thresh;   /* 0.1   the smallest depth that is a return, metres; >= 0.0625                        */
    float   max_depth;      /* 100   the largest; <= 16384                                                         */
} dcmt_support_params;      /* 12 bytes */
void dcmt_default_support_params(dcmt_support_params *p);
int dcmt_support_distance_dev(dcmt_ctx *ctx, const float *d_sparse, const float *d_dense /* or NULL */, const float *d_fallback /* or NULL */,
                              float *d_out /* may be d_dense, or NULL */, uint16_t *d_dist2 /* or NULL */, int rows, int cols, int batch,
                              const dcmt_support_params *params, uint32_t *d_beyond /* [batch] or NULL */, void *stream);
int dcmt_support_distance_u16_dev(dcmt_ctx *ctx, const uint16_t *d_sparse, float scale /* 1./256 for KITTI */, const float *d_dense /* or NULL */,
                                  const float *d_fallback /* or NULL */, float *d_out /* may be d_dense, or NULL */, uint16_t *d_dist2 /* or NULL */,
                                  int rows, int cols, int batch, const dcmt_support_params *params, uint32_t *d_beyond /* [batch] or NULL */,
                                  void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES, >= 4 * cols, dist2's >= 2 * cols; the stride of a plane that is not
 * given is not looked at); out may be dense; beyond: one count or NULL.  The same bits as the device call.  What
 * dcmt_shim::distance_to_returns and dcmt_shim::trust_mask call. */
int dcmt_support_distance(dcmt_ctx *ctx, const float *sparse, size_t sparse_row_stride, const float *dense, size_t dense_row_stride,
                          const float *fallback, size_t fallback_row_stride, float *out, size_t out_row_stride, uint16_t *dist2,
                          size_t dist2_row_stride, int rows, int cols, const dcmt_support_params *params, uint32_t *beyond);

/* ---- image-guided filling of a depth plane: the joint (cross) bilateral filter ---------------------------- */

/* Every finish of a depth plane so far is blind to the camera image, and dcmt_support_distance_dev leaves zeros beyond its radius
 * that nothing fills but a second plane or the cascade again.  This call fills (and, where asked, smooths) a depth plane under the
 * guidance of the camera image, as joint bilateral upsampling does (Kopf et al.): a pixel takes a weighted mean of the MEASURED
 * depths around it, a tap weighing more the closer it is and the more its camera pixel looks like the centre's.  Not in the
 * reference; stated here to the last bit.  The weights are integers out of two tables the host builds: no device exp is part of it.
 * Per frame, on a depth plane [rows][cols] and a guide [rows][cols][guide_channels] (uint8; 1 channel: grey, 3: BGR, Lab, any):
 *
 * VALID.  A pixel is valid when its bits pass the planes' return test (dcmt_superpixel_planes_dev, the occlusion filter, the support
 *   map): a finite float with valid_thresh <= v <= max_depth, decided on the bit pattern.  Everything else -- 0, NaN, +-inf,
 *   negatives, -0.0 -- is a HOLE.  The same bounds are enforced: valid_thresh >= 0.0625, max_depth <= 16384.
 * WHICH PIXELS.  A valid centre without DCMT_JOINT_SMOOTH and a hole without DCMT_JOINT_FILL are copied: the four bytes, opaque.
 *   Every other pixel is PROCESSED:
 * TAPS.  The offsets (dy, dx) with d2 = dy^2 + dx^2 <= R^2, R = radius in 1..9 (a disc; 253 taps at R = 9), in row-major order
 *   (dy ascending, then dx ascending).  A tap outside the frame or on a hole contributes nothing: nothing ever crosses a frame of the
 *   batch or wraps a row.
 * WEIGHT.  w = min(w_space[d2], 255) * min(w_guide[s], 255), s = the sum over the channels of |guide(tap) - guide(centre)|
 *   (0 .. 765): an integer <= 65025, exact as a float.
 * BASE.  base = the centre's value where the centre is valid; otherwise the value of the first tap in tap order with w > 0.
 * SUMS.  sw += w in integers: at most 253 * 65025 = 16 451 325 < 2^24, so (float) sw is exact -- this bound is why R stops at 9.
 *   acc = fadd_rn(acc, fmul_rn((float) w, fsub_rn(v, base))) in tap order from acc = +0.0f, every operation rounded once, nothing
 *   contracted.  (A valid tap with w = 0 adds +-0 to a sum that is never -0: skipping it changes no bit.)
 * RESULT.  sw < min_weight: the centre's four bytes are copied; a hole stays a hole.  Otherwise
 *   y = fadd_rn(base, fdiv_rn(acc, (float) sw)).
 * The difference form with this base is part of the statement: a constant region comes back bit for bit, and a hole whose only
 * weighted taps hold one value is filled with exactly that value.
 * d_counts, or NULL: uint32 [batch][2] = {holes filled, holes left}: a hole of the input that was processed and reached min_weight
 *   is filled; every other hole of the input is left, processed or not.  The two add up to the holes of the frame.
 * d_tables: ONE dcmt_joint_tables record for the whole call, built once per configuration (dcmt_make_joint_tables) and uploaded once.
 *   The device uses min(entry, 255): any bytes are a defined input, and w_space is only ever read at d2 <= R^2.
 * Nothing depends on the batch size, the frame's position in the batch, alignment, the launch geometry or the run.
 *
 * DEVICE pointers, stream-ordered; never synchronises, never allocates.  One launch; a clear of d_counts goes in front where they
 * are given: two.  No scratch plane of the context is touched and none of its carried state, dcmt_last_path included: it can be
 * queued in front of or behind any other *_dev call.
 * DCMT_E_INVALID, nothing written: a null ctx, depth plane, guide, tables, output or params; sizes or a batch beyond the context's
 * limits; guide_channels other than 1 or 3; radius outside 1..9; flags without DCMT_JOINT_FILL and DCMT_JOINT_SMOOTH, or with any
 * other bit; min_weight 0; valid_thresh not finite or < 0.0625; max_depth not finite, < valid_thresh or > 16384; d_depth, d_out or
 * d_counts not 4-byte aligned, d_tables not 2-byte aligned (the guide may start at any byte); any overlap between two of the
 * buffers, d_out with d_depth included: a neighbour's input would already be output. */
enum { DCMT_JOINT_FILL = 1, DCMT_JOINT_SMOOTH = 2 };
typedef struct {
    int32_t  radius;        /* 6     R: the taps are the disc dy^2 + dx^2 <= R^2; 1..9                              */
    uint32_t flags;         /* FILL  DCMT_JOINT_FILL: holes are processed; DCMT_JOINT_SMOOTH: valid pixels are      */
    uint32_t min_weight;    /* 1     a processed pixel whose sw stays below it is copied; >= 1                      */
    float    valid_thresh;  /* 0.1   the smallest depth that is valid, metres; >= 0.0625                            */
    float    max_depth;     /* 100   the largest; <= 16384                                                          */
} dcmt_joint_params;        /* 20 bytes */
typedef struct {
    uint16_t w_space[128];  /* indexed by dy^2 + dx^2 (read at <= R^2 <= 81 only)                                   */
    uint16_t w_guide[768];  /* indexed by the L1 distance of the guide pixels, 0 .. 765                              */
} dcmt_joint_tables;        /* 1792 bytes */
void dcmt_default_joint_params(dcmt_joint_params *p);
/* Host, no GPU: w_space[d2] = rne(255 exp(-d2 / (2 sigma_space^2))) for d2 <= radius^2, else 0; w_guide[s] = rne(255 exp(-s^2 /
 * (2 sigma_guide^2))); both in f64, rounded to nearest even.  DCMT_E_INVALID, nothing written: a null record, radius outside 1..9, a
 * sigma that is not finite or not > 0. */
int dcmt_make_joint_tables(int radius, double sigma_space, double sigma_guide, dcmt_joint_tables *tables);
int dcmt_joint_bilateral_dev(dcmt_ctx *ctx, const float *d_depth, const uint8_t *d_guide, int guide_channels, const dcmt_joint_tables *d_tables,
                             float *d_out, int rows, int cols, int batch, const dcmt_joint_params *params, uint32_t *d_counts /* [batch][2] or NULL */,
                             void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES: depth's and out's >= 4 * cols, the guide's >= guide_channels * cols);
 * tables: a HOST record; counts: two values or NULL.  The same bits as the device call.  What dcmt_shim::joint_bilateral_fill calls. */
int dcmt_joint_bilateral(dcmt_ctx *ctx, const float *depth, size_t depth_row_stride, const uint8_t *guide, size_t guide_row_stride,
                         int guide_channels, const dcmt_joint_tables *tables, float *out, size_t out_row_stride, int rows, int cols,
                         const dcmt_joint_params *params, uint32_t *counts);

/* ---- consumer of the path's output: stereo photometric refinement (N4) ----------------- */

/* What DC_stereo_lidar/main_sl.cpp does with the dense depth (:1165-1246): depth -> disparity (get_initial_disparity
 * :846-861), four damped Gauss-Newton sweeps that move every pixel's disparity along its epipolar line so that the right
 * image matches the left one (optimize_IG :804-843 with calculateObservationDerivatives :749-801 on images whose
 * derivatives calculateMeasuementDerivatives :715-747 made), disparity -> depth clamped to max_depth
 * (retrieve_optimized_depth :863-885).  Every pixel only ever touches its own disparity, so the sweeps are independent
 * per pixel.  d_left / d_right: [batch][rows][cols] uint8 grey images (the reference's cv::cvtColor(BGR2GRAY) outputs,
 * :1167-1171: what dcmt_bgr_convert_dev writes from the cameras' BGR bytes, on the same stream); d_depth: the path's output; d_refined: [batch][rows][cols] f32, 0 where the disparity ends up <= 0.
 * iterations < 0 selects the reference's 4; iterations == 0 is the pure depth -> disparity -> depth round trip
 * (its `depth_pre_optim`, :1225-1226). */
typedef struct {
    float   baseline;      /* 0.54f          :847 */
    float   focal;         /* 9.597910e+02f  :848 */
    float   damp;          /* 500            :808 */
    float   max_depth;     /* 100            :876 */
    int32_t iterations;    /* 4              :805 */
} dcmt_stereo_params;
void dcmt_default_stereo_params(dcmt_stereo_params *p);
int dcmt_stereo_refine_dev(dcmt_ctx *ctx, const float *d_depth, const uint8_t *d_left, const uint8_t *d_right,
                           float *d_refined, int rows, int cols, int batch, const dcmt_stereo_params *params,
                           void *stream);

/* ---- scoring the path's output against ground truth ---------------------------------- */

/* What every reference main does with the dense depth: evaluate_performance, DC_lidar_only/main.cpp:16-34 (the signed mean
 * error over gt > 0, returned as `mse`); evaluate_performance, DC_lidar_camera/main_lc.cpp:85-116 (RMSE -- named `mse` -- and
 * MAE over gt > 0 && pred > 0: its `int tolerance = 0.1;` truncates to 0); evaluate_performances, DC_stereo_lidar/main_sl.cpp:1031-1061
 * (MAE and RMSE over gt > 2 && pred > 2, run before and after the refinement, :1232 / :1247); plus the inverse-depth terms of the
 * KITTI depth-completion table that main_lc.cpp:93-98 holds as commented-out lines (iMAE, iRMSE).  The library returns per-frame
 * SUMS; the divisions (and the reference's f32 final arithmetic) are the caller's -- the Python layer's eval_summary /
 * evaluate_performance do them.
 *
 * Per pixel, exactly the reference's statements: e = gt - pred, d = fabsf(e), d * d are f32 operations (one rounding each, no FMA);
 * thresh compares as an f32 `>` (what `float > int` is in the reference).  The inverse term |1.0/(double)gt - 1.0/(double)pred| is
 * f64 and is taken only where pred > 0 too (nothing non-finite enters a library built with -ffinite-math-only).
 * Sums: f64, in a fixed reduction tree (dcmt_kernels_eval.h): a frame's 7 values depend only on its own pixels and on (rows, cols)
 * -- not on batch, the frame's position in the batch, the load widths its alignment allows, or the run.  No float atomics.  The
 * reference's running `float` sum is NOT reproduced: the f64 sum is closer to the exact value (the two agree where every partial
 * sum is exact in f32).  A frame whose mask is empty gives all zeros. */
typedef struct {                /* n and n_inv are integer counts stored as doubles (exact: a frame has < 2^29 pixels) */
    double n;                   /* pixels in the mask                                                                    */
    double sum_err;             /* sum of e = gt - pred, e an f32 difference             (LO main.cpp:27)                */
    double sum_abs;             /* sum of d = |e|, d an f32 value                         (LC main_lc.cpp:106, SL :1049)  */
    double sum_sq;              /* sum of d * d, product rounded to f32, no FMA           (LC :108, SL :1052)             */
    double n_inv;               /* pixels in the mask with pred > 0 (== n in DCMT_EVAL_BOTH mode)                         */
    double sum_inv_abs;         /* sum of |1.0/(double)gt - 1.0/(double)pred| over those  (main_lc.cpp:96, f64)           */
    double sum_inv_sq;          /* sum of its square, f64                                                                 */
} dcmt_eval_frame;

#define DCMT_EVAL_GT    0       /* mask: gt > thresh                   (DC_lidar_only)                                    */
#define DCMT_EVAL_BOTH  1       /* mask: gt > thresh && pred > thresh  (DC_lidar_camera, DC_stereo_lidar)                 */

/* DEVICE pointers, stream-ordered: d_gt, d_pred contiguous [batch][rows][cols]; d_out: [batch] dcmt_eval_frame, 8-byte aligned.
 * Never synchronises.  May be enqueued right behind a completion or refinement call on the same stream (same ordering rule as
 * every *_dev call on one ctx); it touches none of the state the cascade carries from call to call (the 16-bit flag ring, the
 * normalisation extrema, the bounding-box tables, the projection's winner plane) and leaves dcmt_last_path and the probes alone.
 * The first evaluate call on a ctx allocates a partial-sum slab (64 B per 8192 pixels of a max_rows x max_cols frame, times
 * max_batch) before it enqueues anything; later calls never allocate.
 * DCMT_E_INVALID: a null pointer, sizes beyond the ctx limits, thresh < 0 (or not finite), mode not DCMT_EVAL_GT / DCMT_EVAL_BOTH,
 * d_out not 8-byte aligned. */
int dcmt_evaluate_dev(dcmt_ctx *ctx, const float *d_gt, const float *d_pred, int rows, int cols, int batch,
                      float thresh, int mode, dcmt_eval_frame *d_out, void *stream);
/* Ground truth as the KITTI depth PNG payload: gt = __fmul_rn((float)v, gt_scale) (gt_scale 1/256 for KITTI), the conversion of
 * dcmt_complete_u16_dev and of LO main.cpp:82 / LC main_lc.cpp:180; the same bits as dcmt_evaluate_dev on the converted plane.
 * (SL passes the raw uint16 Mat to its float reader, main_sl.cpp:1232, :1247 -- a caller bug, not reproduced.) */
int dcmt_evaluate_u16_dev(dcmt_ctx *ctx, const uint16_t *d_gt, float gt_scale, const float *d_pred,
                          int rows, int cols, int batch, float thresh, int mode, dcmt_eval_frame *d_out, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES); the same bits as dcmt_evaluate_dev on the frame.  Uses the ctx's
 * slab like the device call, so it must not overlap a device evaluate call on the same ctx that is still in flight. */
int dcmt_evaluate(dcmt_ctx *ctx, const float *gt, size_t gt_row_stride, const float *pred, size_t pred_row_stride,
                  int rows, int cols, float thresh, int mode, dcmt_eval_frame *out);

/* ---- JET colourisation of the path's output ------------------------------------------------------------ */

/* The reference mains' toColorImage (DC_lidar_only/main.cpp:6-14, utils.cpp:6-13, DC_stereo_lidar/main_sl.cpp:42-49), run on
 * every dense plane after the path:
 *     cv::normalize(r_img, n, 1.0, 0, cv::NORM_MINMAX);  n.convertTo(u8, CV_8UC1, 255.0);  cv::applyColorMap(u8, out, COLORMAP_JET);
 * Per frame: smin / smax = its extrema; scale = 1 / (smax - smin) in double (0 when smax - smin <= DBL_EPSILON), rounded to f32;
 * shift = -(float)(smin * scale); v = x * scale + shift in f32 with two roundings (the arithmetic of DCMT_FLAG_NORMALIZE);
 * idx = v * 255 rounded half to even and saturated to 0..255; out = the JET palette's entry idx, 3 bytes in B, G, R order.
 * An AVX2 build of OpenCV fuses x * scale + shift into one FMA: that can move a pixel by one palette index, only in a frame
 * without a zero pixel and only where v * 255 lies within an ulp of a .5.  A constant frame maps to entry 0.  Inputs must be
 * finite, as for every entry point of this library (-ffinite-math-only); -0.0 is treated as 0.0. */

/* DEVICE pointers, stream-ordered: d_src contiguous f32 [batch][rows][cols], 4-byte aligned; d_bgr [batch][rows][cols][3] bytes,
 * any alignment (16-byte d_src and 4-byte d_bgr take the wide loads and stores).  Never synchronises.  May be enqueued right
 * behind a completion or refinement call on the same stream (same ordering rule as every *_dev call on one ctx); it touches none
 * of the state the cascade carries from call to call (the 16-bit flag ring, the normalisation extrema, the bounding-box tables,
 * the projection's winner plane) and leaves dcmt_last_path and the probes alone.  Uses a min/max slab that dcmt_create allocates
 * (8 B per 8192 pixels of a max_rows x max_cols frame, times max_batch); never allocates.  A frame's bytes depend only on its
 * own pixels, not on batch or its position in the batch.  No float atomics.
 * DCMT_E_INVALID: a null pointer, sizes beyond the ctx limits, d_src not 4-byte aligned. */
int dcmt_colorize_dev(dcmt_ctx *ctx, const float *d_src, int rows, int cols, int batch, uint8_t *d_bgr, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES: src_row_stride >= 4 * cols, bgr_row_stride >= 3 * cols); the same
 * bytes as dcmt_colorize_dev on the frame.  What dcmt_shim::to_color_image calls.  Uses the ctx's slab like the device call, so it
 * must not overlap a device colorize call on the same ctx that is still in flight. */
int dcmt_colorize(dcmt_ctx *ctx, const float *src, size_t src_row_stride, int rows, int cols, uint8_t *bgr, size_t bgr_row_stride);
/* The palette the kernels use: cv::COLORMAP_JET's 256 entries in index order, each B, G, R.  Needs no GPU. */
void dcmt_colormap_jet(uint8_t bgr[768]);

/* ---- the dense plane as an ordered point cloud, and the blur in front of it ------------------------------ */

/* What DC_stereo_lidar/main_sl.cpp does with the refined depth after the path (:1251-1270): an unmasked 5x5 Gaussian (:1253),
 * toColorImage (:1257, :1259: dcmt_colorize_dev), and reproject_pc_colors (:924-965; its colourless twin reproject_pc :887-922),
 * which turns the plane into the ordered, coloured point cloud the executable writes as colored_point_cloud.pcd.
 *
 * Back-projection: frames in batch order, pixels row-major (y outer, x inner: the reference's push_back order), one record
 * only where depth > 0 as an f32 compare (so -0.0, 0 and negatives give none), exactly the reference's statements (:934-955):
 *     z  = depth
 *     x_ = (float)(((double)x - cx) * (double)z / fx)      f64 subtraction, product and a true IEEE division, one rounding
 *     y_ = (float)(((double)y - cy) * (double)z / fy)      each, then one rounding to f32
 *     b, g, r = d_bgr[frame][y][x][0..2], a = 255          (PointXYZRGB sets alpha 255)
 *     d_bgr == NULL (reproject_pc): the fourth dword is 1.0f (PCL's PointXYZ padding; also the [x y z w] record that
 *                                   dcmt_project_points_dev reads, so a cloud can go straight back into the projection). */
typedef struct { double fx, fy, cx, cy; } dcmt_cloud_params;              /* 9.597910e+02, 9.569251e+02, 6.960217e+02, 2.241806e+02: main_sl.cpp:927-930 */
typedef struct { float x, y, z; uint8_t b, g, r, a; } dcmt_cloud_point;   /* 16 bytes */
void dcmt_default_cloud_params(dcmt_cloud_params *p);

/* DEVICE pointers, stream-ordered.  d_depth: contiguous f32 [batch][rows][cols], 4-byte aligned; d_bgr: [batch][rows][cols][3]
 * bytes, any alignment, or NULL -- the layout dcmt_colorize_dev writes, so the colourised depth (the reference's commented line
 * :943) or a camera image (:944) can be passed.
 * d_offsets: [batch + 1] int32; frame f owns records [d_offsets[f], d_offsets[f+1]), d_offsets[0] = 0, d_offsets[batch] = the
 * total: the convention of dcmt_project_points_dev.  The offsets are always the true counts.
 * d_points: ONE packed run for the whole batch, 16-byte aligned, room for `capacity` records.  A record whose global index is
 * >= capacity is not written and nothing at or beyond min(total, capacity) records is touched; the call never synchronises, so
 * the caller sees an overflow as d_offsets[batch] > capacity.  capacity = batch * rows * cols can never overflow.
 * Never synchronises.  May be enqueued right behind any other *_dev call of the ctx on the same stream (same ordering rule as
 * every *_dev call on one ctx); it touches none of the state the cascade carries from call to call (the 16-bit flag ring, the
 * normalisation extrema, the bounding-box tables, the projection's winner plane) and leaves dcmt_last_path and the probes alone.
 * Uses a count slab that dcmt_create allocates (16 B per 8192 pixels of a max_rows x max_cols frame, times max_batch); never
 * allocates.  Integer counts and an integer scan in a fixed order: no atomics, no memset.  A frame's records depend only on its
 * own pixels -- not on batch, its position in the batch, alignment or the run; only its offset depends on the frames before it.
 * DCMT_E_INVALID: null ctx / d_depth / d_points / d_offsets / params, sizes beyond the ctx limits, capacity < 0,
 * batch * rows * cols > INT32_MAX, d_depth not 4-byte or d_points not 16-byte aligned, a non-finite intrinsic, fx or fy zero. */
int dcmt_depth_to_cloud_dev(dcmt_ctx *ctx, const float *d_depth, const uint8_t *d_bgr /* or NULL */,
                            int rows, int cols, int batch, const dcmt_cloud_params *params,
                            dcmt_cloud_point *d_points, int64_t capacity, int32_t *d_offsets, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES; bgr may be NULL): the same bytes as the device call.  Writes
 * min(*n_points, capacity) records; *n_points is the true count. */
int dcmt_depth_to_cloud(dcmt_ctx *ctx, const float *depth, size_t depth_row_stride,
                        const uint8_t *bgr /* or NULL */, size_t bgr_row_stride, int rows, int cols,
                        const dcmt_cloud_params *params, dcmt_cloud_point *points, int64_t capacity, int64_t *n_points);

/* cv::GaussianBlur(src, dst, Size(5, 5), 0) on its own (main_sl.cpp:1253), WITHOUT the masked select of DCMT_STAGE_BLUR: the fixed
 * table [1 4 6 4 1]/16, rows then columns, BORDER_REFLECT_101, each pass c*k0 + (l1 + r1)*k1 + (l2 + r2)*k2 in f32, every
 * operation rounded once.  d_src / d_dst: contiguous f32 [batch][rows][cols], 4-byte aligned.  d_dst == d_src is allowed (the
 * reference's call is in place) and gives the bits of an out-of-place call: the result goes to context scratch (one of the two
 * planes dcmt_create allocates, which every completion call rewrites before it reads it) and one device-to-device copy moves it
 * to d_dst.  Any other overlap is DCMT_E_INVALID.  Stream-ordered, never synchronises, never allocates; same standing behind
 * other *_dev calls as dcmt_depth_to_cloud_dev. */
int dcmt_gaussian5_dev(dcmt_ctx *ctx, const float *d_src, float *d_dst, int rows, int cols, int batch, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES); src may be dst. */
int dcmt_gaussian5(dcmt_ctx *ctx, const float *src, size_t src_row_stride, float *dst, size_t dst_row_stride, int rows, int cols);

/* The 5x5 Gaussian that ignores holes (normalised convolution): for a plane with holes -- the cascade under DCMT_FLAG_NO_EXTRAPOLATE,
 * a trust-masked plane, dcmt_sgm_dev's depth, a speckle-filtered plane.  With G5 the filter of dcmt_gaussian5_dev, thr = valid_thresh
 * and v(x) = x >= thr (NaN is not valid):
 *     num   = G5( v(X) ? X : 0 )          a select, not a product: +inf stays +inf, nothing makes a NaN
 *     den   = G5( v(X) ? 1.0f : 0.0f )    exact: a multiple of 1/256
 *     GV(X) = v(X) ? num / den : X        one IEEE f32 division, round to nearest even
 * Consequences: at a valid pixel den >= 0.375^2 = 0.140625 (its own tap).  Where all 25 taps are valid den == 1.0f and GV(X) is
 * G5(X) bit for bit, so on a plane without holes this call is dcmt_gaussian5_dev.  An invalid pixel comes back bit for bit: zero,
 * -0.0, negatives, NaN.  A valid result lies in [min, max] of its valid taps up to the rounding of about 15 f32 operations on
 * non-negative terms (a few ulp; so does a constant region with holes: close, not bit for bit).  No NaN comes out of a
 * plane without one.
 * valid_thresh: finite and > 0, as dcmt_params.valid_thresh (DCMT_E_INVALID otherwise, nothing written).  Buffers, alignment,
 * d_dst == d_src (through context scratch and one copy), any other overlap (DCMT_E_INVALID), limits and the standing behind other
 * *_dev calls: as dcmt_gaussian5_dev.  A pixel's bits do not depend on batch, its frame's position in the batch or the launch
 * geometry.  Stream-ordered, never synchronises, never allocates. */
int dcmt_gaussian5_valid_dev(dcmt_ctx *ctx, const float *d_src, float *d_dst, int rows, int cols, int batch, float valid_thresh,
                             void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES); src may be dst. */
int dcmt_gaussian5_valid(dcmt_ctx *ctx, const float *src, size_t src_row_stride, float *dst, size_t dst_row_stride, int rows, int cols,
                         float valid_thresh);

/* cv::bilateralFilter(src, dst, 5, sigma_color, sigma_space) for CV_32FC1 with BORDER_DEFAULT, as this project states it (OpenCV is
 * never executed, and its 4096-bin interpolated exp table is not restated: DESIGN.md section 19): the edge-preserving alternative to
 * dcmt_gaussian5_dev in front of the point cloud, and the kernel behind DCMT_BLUR_BILATERAL_CLONE.
 *   taps     the 13 offsets (dy, dx) with dy*dy + dx*dx <= 4, BORDER_REFLECT_101 on both axes (also for 1 or 2 rows or columns)
 *   weights  ws(dy, dx) = (float)exp(-(dy*dy + dx*dx) / (2 sigma_space^2)), evaluated in double on the host;
 *            wc = exp(gc * d * d) with d = v(tap) - v(centre) and gc = -0.5f / sigma_color^2, in f32 (the device's exp)
 *   output   y = c + (sum ws wc d) / (sum ws wc), every operation in f32 and rounded once, both sums in tap order (row-major);
 *            the centre tap adds d = 0, w = 1.  A constant plane comes back bit for bit.
 * A pixel's bits do not depend on batch, its frame's position in the batch or the launch geometry.  Buffers, alignment, d_dst ==
 * d_src (through context scratch and one copy), any other overlap (DCMT_E_INVALID) and the standing behind other *_dev calls: as
 * dcmt_gaussian5_dev.  Also DCMT_E_INVALID: a sigma that is not finite and > 0, or a sigma_color whose square has no finite f32
 * reciprocal.  Stream-ordered, never synchronises, never allocates. */
int dcmt_bilateral5_dev(dcmt_ctx *ctx, const float *d_src, float *d_dst, int rows, int cols, int batch, float sigma_color,
                        float sigma_space, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES); src may be dst. */
int dcmt_bilateral5(dcmt_ctx *ctx, const float *src, size_t src_row_stride, float *dst, size_t dst_row_stride, int rows, int cols,
                    float sigma_color, float sigma_space);

/* ---- a dense plane seen by one camera -> the plane another camera sees --------------------------------- */

/* The data part of unrectify_sol (DC_stereo_lidar/main_sl.cpp:967-1028, called at :1228 on the pre-refinement depth so that "MAE
 * pre" can be scored against ground truth, which lives in the un-rectified frame, :1225-1234); its cv::circle / imshow / std::cout
 * lines are display and are not reproduced.  A forward warp: per source pixel (row y, column x), exactly the reference's statements
 *     z  = depth                                                                            (:986-988)
 *     x_ = (float)(((double)x - cx) * (double)z / fx)      f64 subtraction, product and a true IEEE division, one rounding
 *     y_ = (float)(((double)y - cy) * (double)z / fy)      each, then one rounding to f32    (:989-990)
 *     t  = M * (x_, y_, z, 1)                              rows 0..2                         (:993)
 *     skip unless t.z > 0          -- the only validity test: there is NO depth > 0 filter   (:999)
 *     c  = K * (t.x, t.y, t.z);  uf = c.x / t.z,  vf = c.y / t.z                             (:1000-1001)
 *     if 0 <= uf < out_cols and 0 <= vf < out_rows:  out(int(vf), int(uf)) = t.z             (:1008-1015)
 * in row-major source order, so a later source pixel overwrites an earlier one that fell into the same destination pixel (with
 * KITTI's R_rect_02 some 800 destination pixels of a 352x1216 plane are decided that way).  d_out is written completely, 0 where
 * nothing lands (the reference starts from Mat::zeros, :1227).
 * M: 4x4, K: 3x3, both ROW-major (Eigen's default storage is column-major: pass the transposes' data()); M's 4th row and K's 3rd
 * row are ignored.  M is the matrix that is APPLIED: the reference computes R_rect.inverse() with Eigen inside the loop; Eigen's
 * f32 inverse is not reproduced, the caller passes the inverse.  All arithmetic behind x_, y_ is f32, one rounding per operation,
 * sums left to right -- the order of the reference's hand-written transform in N2; Eigen's evaluation order for the
 * `Matrix4f * Vector4f` and `Matrix3f * Vector3f` products is not pinned, so against a real build a pixel
 * whose uf or vf sits within an ulp of an integer may land in the neighbouring pixel. */
typedef struct { double fx, fy, cx, cy; float M[16]; float K[9]; } dcmt_reproject_params;   /* row-major; M's 4th row is ignored */
/* fx, fy, cx, cy and K = camera_mat of :969-976; M = identity */
void dcmt_default_reproject_params(dcmt_reproject_params *p);

/* DEVICE pointers, stream-ordered.  d_depth: contiguous f32 [batch][rows][cols]; d_out: contiguous f32 [batch][out_rows][out_cols];
 * both 4-byte aligned (16-byte d_out with batch * out_rows * out_cols a multiple of 4 takes the widest stores).  Finite inputs, as
 * for every entry point of this library.  Never synchronises once it has allocated what it needs.  May be enqueued right behind any
 * other *_dev call of the ctx on the same stream (same ordering rule as every *_dev call on one ctx); of the state the cascade
 * carries from call to call it touches only the winner plane it SHARES with dcmt_project_points_dev: batch * out_rows * out_cols
 * uint32 tags (generation | frame-local source pixel index, at least 24 index bits: one layout for both calls).  A call of either
 * kind looks only at tags of its own generation, so the two may follow each other in any order; the plane is (re)allocated -- a
 * synchronising hipMalloc, before the call enqueues anything -- only when a call needs more entries than any call before it, and
 * cleared only then, when the generations run out (every 255 calls at 24 bits) or when a call needs more index bits.  The
 * layout never shrinks: once a dcmt_project_points_dev call with more than 2^24 points has raised the index bits to b, every later
 * call of either kind on that ctx runs out of generations after 2^(32-b) - 1 calls (7 at 29 bits), each time at the cost of
 * one clear of the whole plane; a caller to whom that matters gives the two kinds a ctx each.  Integer
 * atomicMax decides the winner: the result does not depend on arrival order, the batch size, a frame's position in the batch,
 * alignment or the run.  d_depth is not written.
 * DCMT_E_INVALID: a null pointer, rows x cols or out_rows x out_cols beyond the ctx limits, batch beyond max_batch, a non-finite
 * intrinsic or matrix entry (of the rows that are read), fx or fy zero, a pointer not 4-byte aligned, d_out overlapping d_depth in
 * any way (the reference's planes are distinct: there is no in-place form).  The warp as a z-buffer (the smallest t_2 instead of the
 * last): dcmt_reproject_depth_nearest_dev, below. */
int dcmt_reproject_depth_dev(dcmt_ctx *ctx, const float *d_depth, int rows, int cols, int batch,
                             const dcmt_reproject_params *params, float *d_out, int out_rows, int out_cols, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES); the same bits as the device call on the frame.  Uses the ctx's
 * winner plane like the device call. */
int dcmt_reproject_depth(dcmt_ctx *ctx, const float *depth, size_t depth_row_stride, int rows, int cols,
                         const dcmt_reproject_params *params, float *out, size_t out_row_stride, int out_rows, int out_cols);

/* ---- per-frame calibration tables for the four geometric *_dev calls ----------------------------------- */

/* dcmt_project_points_dev, dcmt_depth_to_cloud_dev, dcmt_reproject_depth_dev and dcmt_stereo_refine_dev take ONE camera geometry for
 * the whole batch (the reference runs one frame of one drive).  A real batch is mixed -- the KITTI depth-completion validation and
 * selection sets draw their frames from five recording days, each with its own P_rect, R_rect, Tr_velo_to_cam, focal length and
 * baseline -- so each of the four has a twin that takes a DEVICE table of [batch] records instead, record f for frame f:
 *     call                              record                  bytes   table alignment
 *     dcmt_project_points_calib_dev     dcmt_project_calib      96      16    T rows 0..2 at byte 0, P at byte 48, row-major
 *     dcmt_depth_to_cloud_calib_dev     dcmt_cloud_params       32      8     fx, fy, cx, cy at bytes 0, 8, 16, 24
 *     dcmt_reproject_depth_calib_dev    dcmt_reproject_params   136     8     fx fy cx cy at 0, M at 32, K at 96, 4 bytes of padding
 *     dcmt_stereo_refine_calib_dev      dcmt_stereo_calib       8       8     baseline at byte 0, focal at byte 4
 * The table is read by the kernels, on the caller's stream: it may be written by earlier work on that stream, and it must stay
 * unchanged until the call's kernels have run.  It is only read.  Typically it is uploaded once, outside the hot loop.
 * Everything else is as for the uniform twin -- the arithmetic operation by operation, the winner plane and its generations, the
 * packed cloud layout and its true offsets, the in-place and overlap rules, the load widths alignment allows, every argument
 * check that needs no table; the calls never synchronise and allocate nothing their twins do not.  Frame f of a table call is,
 * bit for bit, what the uniform call returns for frame f alone with record f.
 * DCMT_E_INVALID in addition: a null table, a table not aligned as listed, a table that overlaps an output buffer (d_sparse;
 * d_points or d_offsets; d_out; d_refined).
 *
 * BAD RECORDS.  The host cannot look into a device table without synchronising, so what the uniform calls refuse on the host is
 * tested per frame on the device: a non-finite entry (of the entries that are read: T rows 0..2 and P; the intrinsics; M rows
 * 0..2 and K rows 0..1; baseline and focal), fx or fy zero, focal zero.  A frame whose record fails gives the EMPTY result -- a zero
 * plane from the projection, the reprojection and the refinement; no records from the cloud, in its count pass too, so that
 * d_offsets[f + 1] == d_offsets[f] and every other frame's offsets stay true -- and the other frames are what they would be
 * with a good record there.  The library is built with -ffinite-math-only: the kernels test the BIT PATTERN of a record (its
 * exponent field, read as an integer), never a float compare the compiler may remove.  A record that is finite can still overflow
 * the arithmetic (Inf - Inf); its frame is then whatever that arithmetic gives, but every address that depends on a record's values
 * is formed only after an integer-domain bound has held ((unsigned)u < cols && (unsigned)v < rows in both scatter kernels), so the
 * calls are memory-safe on any table contents and no other frame is touched. */
typedef struct { float T[12]; float P[12]; } dcmt_project_calib;   /* rows 0..2 of T, then P; row-major; 96 B */
typedef struct { float baseline, focal; }    dcmt_stereo_calib;    /* 8 B */

int dcmt_project_points_calib_dev(dcmt_ctx *ctx, const float *d_points, const int32_t *d_offsets, int n_points, int batch,
                                  const dcmt_project_calib *d_calib /* [batch], 16-byte aligned */,
                                  float *d_sparse, int rows, int cols, void *stream);
int dcmt_depth_to_cloud_calib_dev(dcmt_ctx *ctx, const float *d_depth, const uint8_t *d_bgr /* or NULL */,
                                  int rows, int cols, int batch, const dcmt_cloud_params *d_params /* [batch], 8-byte aligned */,
                                  dcmt_cloud_point *d_points, int64_t capacity, int32_t *d_offsets, void *stream);
int dcmt_reproject_depth_calib_dev(dcmt_ctx *ctx, const float *d_depth, int rows, int cols, int batch,
                                   const dcmt_reproject_params *d_params /* [batch], 8-byte aligned */,
                                   float *d_out, int out_rows, int out_cols, void *stream);
/* params: HOST, as for dcmt_stereo_refine_dev: damp, max_depth and iterations are used, its baseline and focal are ignored */
int dcmt_stereo_refine_calib_dev(dcmt_ctx *ctx, const float *d_depth, const uint8_t *d_left, const uint8_t *d_right,
                                 float *d_refined, int rows, int cols, int batch, const dcmt_stereo_params *params,
                                 const dcmt_stereo_calib *d_calib /* [batch], 8-byte aligned */, void *stream);

/* ---- surface normals of a depth plane, and the flying-pixel filter ---------------------------------------- */

/* Every dense plane this library produces has been through a Gaussian or a weighted mean, and at a depth edge those write values
 * BETWEEN foreground and background: back-projected, a veil of points strung along the viewing rays.  And every consumer of a cloud
 * asks for normals next.  One observation serves both, the one dcmt_superpixel_planes_dev rests on: a pinhole camera sees a plane
 * affine in inverse depth.  With w = 1 / z and its gradient (gx, gy) per pixel, the local plane is n . P = 1 with
 * n = (fx gx, fy gy, w - gx (x - cx) - gy (y - cy)): P = z ((x - cx) / fx, (y - cy) / fy, 1) gives n . P = z w = 1.  So -n / |n| is the
 * unit normal towards the camera and 1 / |n| the distance of that plane from the camera centre.  A veil runs along viewing rays: a
 * plane through (nearly) the camera centre, 1 / |n| ~ 0, while a real surface cannot pass closer to the camera than the camera's
 * clearance (KITTI's ground: 1.65 m at every range, where an angle-of-incidence test would delete the far road).  Not in the
 * reference; stated here to the last bit.  Per frame, on a depth plane [rows][cols] f32 with intrinsics fx, fy, cx, cy:
 *
 * INTRINSICS.  A dcmt_cloud_params record, converted once to f32: fxf = (float) fx, and so on.
 * VALID.  The planes' return test (dcmt_superpixel_planes_dev), on the bit pattern: a finite float with valid_thresh <= z <=
 *   max_depth.  The same bounds are enforced: valid_thresh >= 0.0625, max_depth <= 16384.  Everything else is a HOLE.
 * INVERSE DEPTH.  w = fdiv_rn(1.0f, z) on a valid pixel.
 * GRADIENT, per axis.  F = fsub_rn(w(next), w(here)) where the next pixel on the axis lies in the frame and is valid;
 *   B = fsub_rn(w(here), w(previous)) likewise.  With both: g = F where |F| <= |B|, else B (a tie takes F).  With one: that one.  A
 *   valid pixel that has neither on one of the two axes (or on both) has NO NORMAL: a gradient that was not observed is not taken
 *   for zero, so a frame of one row or one column has none at all.  The smaller one-sided difference, not the central one, is part
 *   of the statement: it keeps the last pixel of a surface at a clean step on its own surface, so sharp planes lose nothing.
 *   Nothing crosses a frame of the batch or wraps a row.
 * PLANE.  a = fmul_rn(fxf, gx), b = fmul_rn(fyf, gy), dx = fsub_rn((float) x, cxf), dy = fsub_rn((float) y, cyf),
 *   c = fsub_rn(fsub_rn(w, fmul_rn(gx, dx)), fmul_rn(gy, dy)), len2 = fadd_rn(fadd_rn(fmul_rn(a, a), fmul_rn(b, b)), fmul_rn(c, c)):
 *   every operation rounded once, nothing contracted.  len2 > 0 always: a = b = 0 forces c = w > 0.
 * RECORD (dcmt_normal, 16 bytes a pixel).  len = fsqrt_rn(len2), dist = fdiv_rn(1.0f, len), nx = fmul_rn(-a, dist), ny =
 *   fmul_rn(-b, dist), nz = fmul_rn(-c, dist).  A hole or a pixel with no normal gets four +0.0f.
 * REMOVED.  dmin2 = fmul_rn(dmin, dmin), dmin = min_plane_dist, computed once on the host.  A valid pixel with a normal is removed
 *   when fmul_rn(len2, dmin2) > 1.0f.  min_plane_dist = 0 removes nothing.  Every decision is taken on the INPUT.
 * d_out (f32 plane), or NULL: +0.0f where removed; elsewhere the input's four bytes, opaque, so a NaN keeps its bits.
 * d_counts, or NULL: uint32 [batch][2] = {removed, valid pixels with no normal}.
 * Nothing depends on the batch size, the frame's position in the batch, alignment, the launch geometry, the run, or on whether
 * the call is in place.
 *
 * What the statement gives at its edges: a clean step loses nothing (each side's last pixel takes the difference on its own side),
 * and a column ONE pixel wide in front of a wall is removed: both its row differences cross the step, so its plane is a veil's.
 * Objects two pixels wide and wider keep their pixels.
 *
 * Bounds, enforced so that no operation above can overflow: fx, fy finite with 2^-10 <= |.| <= 2^20; |cx|, |cy| <= 2^20;
 * min_plane_dist finite in [0, 1024].  Then 2^-14 <= w <= 16, a difference of two w is 0 or at least 2^-37, |a|, |b| <= 2^24,
 * |c| < 2^27, len2 < 2^55 and, with a normal, len2 >= 2^-94, 2^-28 < dist <= 2^47.  Underflow is not excluded altogether, and the
 * statement is IEEE-754 binary32 WITH subnormals in every operation (what the kernel and the restatements compute).  Where |cx| and
 * |cy| are each zero or at least 2^-60 -- any calibration -- every intermediate is zero or a normal number but for three products
 * whose underflow changes no bit of the result: c * c where c has cancelled below 2^-63 (a or b is not zero then, and a * a + b * b
 * >= 2^-94 absorbs it as it absorbs zero), and dmin * dmin and len2 * dmin2, which underflow only far below the 1.0f the second is
 * compared with.  Checked: tests/test_normals.py asserts over the extreme inputs, through the literal restatement of
 * tests/normals_restatement.py, that every intermediate is finite and that none but those three is subnormal.
 *
 * The default min_plane_dist = 0.4 is a quarter of KITTI's camera height.  It is measured, not derived: on the cascade's output the
 * ground towards the left and right edges of a KITTI frame bends (within 0.25 m of the truth) into local planes as close as 0.50 m,
 * and 0.4 is the largest of the values tried that removes none of them; DESIGN.md section 38 has the table, with what 0.8 and 1.6
 * remove and keep.
 *
 * dcmt_depth_normals_calib_dev is the same call over a device table of per-frame dcmt_cloud_params records (what
 * dcmt_depth_to_cloud_calib_dev takes): frame f is bit for bit the uniform call on that frame alone with record f.  A record that
 * is bad on the device (outside the bounds above, tested on its bits) gives its frame no normals and removes nothing: its records
 * are zeros, d_out is the copy, its counts {0, its valid pixels}; no other frame is touched.
 *
 * DEVICE pointers, stream-ordered; never synchronises, never allocates.  Out of place: one launch.  In place (d_out == d_depth):
 * two, as the occlusion filter does it: a mask of one bit per pixel, then it is applied.  A clear of d_counts goes in front where
 * they are given.  Both routes give the same bytes.  Scratch: the first of the two planes dcmt_create allocates (the one the
 * occlusion filter borrows), in place only.  Of the context's carried state it touches none, dcmt_last_path included: it can be
 * queued in front of or behind any other *_dev call.
 * DCMT_E_INVALID, nothing written: a null ctx, plane, intrinsics (record or table) or params; neither d_normals nor d_out; sizes
 * or a batch beyond the context's limits; anything outside the bounds above; d_depth, d_out or d_counts not 4-byte aligned,
 * d_normals not 16-byte aligned, the table not 8-byte aligned; any overlap among the buffers other than d_out == d_depth exactly. */
typedef struct {
    float min_plane_dist;   /* 0.4   a pixel whose local plane passes closer to the camera centre is removed, metres; 0..1024 */
    float valid_thresh;     /* 0.1   the smallest depth that is valid, metres; >= 0.0625                                      */
    float max_depth;        /* 100   the largest; <= 16384                                                                    */
} dcmt_normals_params;      /* 12 bytes */
typedef struct {
    float nx, ny, nz;       /* the unit normal, towards the camera (nz < 0 on a surface that faces it)                        */
    float dist;             /* the distance of the pixel's local plane from the camera centre, metres                         */
} dcmt_normal;              /* 16 bytes */
void dcmt_default_normals_params(dcmt_normals_params *p);
int dcmt_depth_normals_dev(dcmt_ctx *ctx, const float *d_depth, int rows, int cols, int batch, const dcmt_cloud_params *cloud,
                           const dcmt_normals_params *params, dcmt_normal *d_normals /* or NULL */, float *d_out /* may be d_depth, or NULL */,
                           uint32_t *d_counts /* [batch][2] or NULL */, void *stream);
int dcmt_depth_normals_calib_dev(dcmt_ctx *ctx, const float *d_depth, int rows, int cols, int batch, const dcmt_cloud_params *d_cloud /* [batch] */,
                                 const dcmt_normals_params *params, dcmt_normal *d_normals /* or NULL */, float *d_out /* may be d_depth, or NULL */,
                                 uint32_t *d_counts /* [batch][2] or NULL */, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES: depth's and out's >= 4 * cols, the normals' >= 16 * cols; the stride
 * of a plane that is not given is not looked at); counts: two values or NULL.  The same bits as the device call.  What
 * dcmt_shim::depth_normals and dcmt_shim::filter_flying_pixels call. */
int dcmt_depth_normals(dcmt_ctx *ctx, const float *depth, size_t depth_row_stride, int rows, int cols, const dcmt_cloud_params *cloud,
                       const dcmt_normals_params *params, dcmt_normal *normals, size_t normals_row_stride, float *out, size_t out_row_stride,
                       uint32_t *counts);

/* ---- nearest wins: the two scatter calls as a z-buffer ------------------------------------------------ */

/* dcmt_project_points_dev and dcmt_reproject_depth_dev resolve a pixel that several points (source pixels) land on the way the
 * reference does: the LAST in file (row-major) order stays.  That is an accident of the order -- a KITTI sweep is ordered by laser
 * and azimuth, not by depth, and the velodyne sits behind and above the cameras, so along every object edge foreground and
 * background returns share pixels -- and it is not what producers of sparse depth do: the KITTI devkit's depth maps and the
 * velodyne_raw images dcmt_complete_u16_dev is fed with keep the CLOSEST return, and a forward warp is a z-buffer.  The reference
 * rule stays the default, bit-exact; each of the four geometric scatter calls (uniform and per-frame-table twins) has a
 * *_nearest* form with the SAME arguments:
 *   - a point / source pixel is transformed, accepted and rejected with exactly the statements and roundings of its twin, so the
 *     set of occupied output pixels is identical;
 *   - among all values the twin's rule would have stored into one output pixel (p.z for the projection -- P's third row carries a
 *     translation, so it need not be positive --, t_2 > 0 for the reprojection) the output holds the SMALLEST, in the usual total
 *     order on finite f32 with -0 below +0.  Equal values tie harmlessly: the output is the value itself;
 *   - everything else is the twin's: the output is written completely, 0 where nothing lands; a bad record of a table empties that
 *     frame only; memory-safe on any table contents; frame f of a table call is, bit for bit, the uniform call on frame f alone with
 *     record f; finite inputs only.
 * Mechanism (csrc/dcmt_kernels_nearest.h): hipMemsetAsync zeroes the output; a scatter kernel does one integer atomicMax per
 * landing point of an order-preserving key of the value INTO THE OUTPUT PLANE (key = ~ord, ord the sign-flip map of f32 bits to
 * unsigned order; never 0 for a finite value, so 0 is "nothing landed"); one pass over the plane, in place, turns keys back into
 * values.  No float atomics: the result is bit-reproducible and does not depend on arrival order, the batch size, a frame's position
 * in the batch, alignment or the run.
 * The nearest calls touch NONE of the state a ctx carries from call to call -- not the winner plane, not a generation, not an
 * allocation -- so they never allocate and never synchronise, and they may be mixed with the last-wins calls (and every other call)
 * on one ctx and stream in any order.
 * Because the output is cleared BEFORE the inputs are read, it must not overlap any input: DCMT_E_INVALID where d_sparse overlaps
 * d_points, d_offsets or the table, or d_out overlaps d_depth or the table.  Otherwise the argument checks are the twins'; in
 * addition d_sparse / d_out and d_offsets must be 4-byte aligned (the plane takes integer atomics), and n_points stays below 2^30.
 * 16-byte aligned outputs with batch * rows * cols a multiple of 4 take the widest accesses in the last pass. */
int dcmt_project_points_nearest_dev(dcmt_ctx *ctx, const float *d_points, const int32_t *d_offsets, int n_points,
                                    int batch, const float T[16], const float P[12], float *d_sparse,
                                    int rows, int cols, void *stream);
int dcmt_project_points_nearest_calib_dev(dcmt_ctx *ctx, const float *d_points, const int32_t *d_offsets, int n_points, int batch,
                                          const dcmt_project_calib *d_calib /* [batch], 16-byte aligned */,
                                          float *d_sparse, int rows, int cols, void *stream);
int dcmt_reproject_depth_nearest_dev(dcmt_ctx *ctx, const float *d_depth, int rows, int cols, int batch,
                                     const dcmt_reproject_params *params, float *d_out, int out_rows, int out_cols, void *stream);
int dcmt_reproject_depth_nearest_calib_dev(dcmt_ctx *ctx, const float *d_depth, int rows, int cols, int batch,
                                           const dcmt_reproject_params *d_params /* [batch], 8-byte aligned */,
                                           float *d_out, int out_rows, int out_cols, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES), staged like their last-wins twins; the same bits as the device
 * call on the frame. */
int dcmt_project_points_nearest(dcmt_ctx *ctx, const float *points, int n_points, const float T[16], const float P[12],
                                float *sparse, size_t sparse_row_stride, int rows, int cols);
int dcmt_reproject_depth_nearest(dcmt_ctx *ctx, const float *depth, size_t depth_row_stride, int rows, int cols,
                                 const dcmt_reproject_params *params, float *out, size_t out_row_stride, int out_rows, int out_cols);

/* ---- producer of the image inputs: camera BGR bytes -> 8-bit Lab and grey planes ----------------------- */

/* What the reference mains do with every camera frame before anything else: cv::cvtColor(image, lab_image, cv::COLOR_BGR2Lab)
 * (DC_lidar_camera/main_lc.cpp:183, DC_stereo_lidar/main_sl.cpp:439: the input of Slic::generate_superpixels) and
 * cv::cvtColor(..., cv::COLOR_BGR2GRAY) (main_sl.cpp:1167, :1171: the inputs of the stereo refinement), on CV_8UC3 pixels B, G, R.
 * Both are integer-only per pixel, in the fixed-point scheme OpenCV uses for 8-bit images -- restated from memory of its sources,
 * never run against an OpenCV: the definition is OURS and bit-exact from there on.
 *     grey  Y = (B * 3735 + G * 19235 + R * 9798 + 16384) >> 15
 *     Lab   R' = gamma[R], G' = gamma[G], B' = gamma[B]             gamma[i] = floor(2040 * lin(i / 255) + 0.5), the sRGB curve
 *           fX = cbrt[D(R' * C00 + G' * C01 + B' * C02, 12)]        cbrt[i] = floor(32768 * f(i / 2040) + 0.5), f = t^(1/3), or
 *           fY, fZ: rows 1 and 2 of C                               7.787 t + 16/116 below 0.008856; C = rint(4096 * M / white), D65
 *           L = D(296 * fY - 1336934, 15),  a = D(500 * (fX - fY) + 128 * 32768, 15),  b = D(200 * (fY - fZ) + 128 * 32768, 15)
 *     with D(v, n) = (v + (1 << (n - 1))) >> n.  L = L* * 255 / 100, a = a* + 128, b = b* + 128, as cv::cvtColor stores them in bytes.
 * Against the documented f64 formulas rounded to nearest, over all 2^24 colours: grey within 1 level, L within 2, a within 3, b
 * within 2 (DESIGN.md section 15 has the counts).
 *
 * DEVICE pointers, stream-ordered.  d_bgr, d_lab: [batch][rows][cols][3] bytes; d_gray: [batch][rows][cols] bytes; any byte
 * alignment (4-byte aligned pointers take the wide loads and stores).  d_lab or d_gray may be NULL, not both: one read of the image
 * serves both outputs (the left image of DC_stereo_lidar needs both, the right one grey only).  d_lab == d_bgr is allowed (in place)
 * and gives the bytes of an out-of-place call; any other overlap among the three buffers is DCMT_E_INVALID.  Never synchronises,
 * never allocates, uses no ctx scratch and carries no state from call to call; may be enqueued in front of or behind any other
 * *_dev call of the ctx on the same stream.  A pixel's bytes depend on that pixel alone.
 * DCMT_E_INVALID: a null ctx or d_bgr, both outputs NULL, sizes beyond the ctx limits, overlapping buffers. */
int dcmt_bgr_convert_dev(dcmt_ctx *ctx, const uint8_t *d_bgr, int rows, int cols, int batch,
                         uint8_t *d_lab /* or NULL */, uint8_t *d_gray /* or NULL */, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES: bgr and lab >= 3 * cols, gray >= cols; the stride of a NULL
 * output is ignored); the same bytes as the device call.  What dcmt_shim::bgr_to_lab / bgr_to_gray call. */
int dcmt_bgr_convert(dcmt_ctx *ctx, const uint8_t *bgr, size_t bgr_row_stride, int rows, int cols,
                     uint8_t *lab /* or NULL */, size_t lab_row_stride,
                     uint8_t *gray /* or NULL */, size_t gray_row_stride);
/* The constants the kernel uses: the two tables and C, row-major (rows X, Y, Z over columns R, G, B).  Any pointer may be NULL.
 * Needs no GPU. */
void dcmt_lab_tables(uint16_t gamma[256], uint16_t cbrt[3072], int32_t coef[9]);

/* ---- the library's two ends: ragged frames in, the uint16 payload out ---------------------------------- */

/* Every *_dev entry point takes [batch][rows][cols] with ONE rows x cols for the call, but the frames of a real batch have several
 * sizes: the five KITTI recording days deliver 375x1242, 370x1224, 374x1238, 370x1226 and 376x1241, the reference's
 * DC_stereo_lidar main reads such raw frames (image_02 / image_03 and the full-size velodyne projection) and scores them against
 * the 352x1216 val_selection_cropped ground truth.  dcmt_crop_frames_dev cuts one window out of each frame of such a ragged
 * batch into one uniform batch, in ONE launch: frame f of d_dst is rows y0 .. y0 + out_rows - 1 and columns x0 .. x0 + out_cols - 1
 * of source frame f, byte for byte -- numpy's src[y0:y0 + out_rows, x0:x0 + out_cols].  An element is elem_bytes OPAQUE bytes: grey
 * 1, uint16 depth or ground truth 2, BGR 3, f32 4.
 * A source frame lies anywhere inside [d_src, d_src + src_bytes) and may be pitched (a packed ragged buffer, a padded batch,
 * cv::Mat::step): record f of the device table says where.  d_src + offset and d_dst may have ANY byte alignment; the aligned part of
 * every destination row is written with 16-byte stores, assembled from naturally aligned 16-byte source loads (a byte shift that is
 * uniform per row), the row's ends with byte accesses; nothing rests on unaligned hardware accesses.  The same bytes either way.
 * The table is read by the kernel on the caller's stream, once per wave, with the rules of the calibration tables above: earlier
 * work on the stream may have written it, it stays unchanged until the kernel has run, it is only read.
 * BAD RECORDS are tested per frame on the device, in the integer domain, in 64-bit arithmetic that cannot wrap.  A record is good if
 *     rows >= 1, cols >= 1, x0 >= 0, y0 >= 0, x0 + out_cols <= cols, y0 + out_rows <= rows, row_stride >= cols * elem_bytes,
 *     offset <= src_bytes, (rows - 1) * row_stride + cols * elem_bytes <= src_bytes - offset
 * all hold.  A frame whose record fails is all ZERO bytes and no other frame is touched (the convention of the *_calib_dev calls).
 * For any table contents the call reads no byte outside [d_src, d_src + src_bytes) and writes none outside d_dst's
 * batch * out_rows * out_cols * elem_bytes bytes.
 * Never synchronises, never allocates, uses no ctx scratch and carries no state from call to call; may be enqueued in front of or
 * behind any other *_dev call of the ctx on the same stream.
 * DCMT_E_INVALID: a null pointer, elem_bytes outside 1..4, out_rows x out_cols or batch beyond the ctx limits (the SOURCE frames may
 * be larger), src_bytes == 0, a table that is not 8-byte aligned, d_dst overlapping [d_src, d_src + src_bytes) or the table. */
typedef struct {
    uint64_t offset;      /* bytes from d_src to element (0,0) of the frame                */
    uint32_t row_stride;  /* bytes between its rows; >= cols * elem_bytes                  */
    int32_t  rows, cols;  /* the frame's own size, in elements                             */
    int32_t  x0, y0;      /* column / row of the window's first element inside the frame   */
    uint32_t reserved;    /* ignored                                                       */
} dcmt_crop_src;          /* 32 bytes; table 8-byte aligned                                */

int dcmt_crop_frames_dev(dcmt_ctx *ctx, const void *d_src, size_t src_bytes,
                         const dcmt_crop_src *d_table /* [batch], device */, int elem_bytes /* 1, 2, 3 or 4 */,
                         void *d_dst /* [batch][out_rows][out_cols] elements, contiguous */,
                         int out_rows, int out_cols, int batch, void *stream);

/* A dense f32 plane as KITTI stores depth: uint16, round(metres * 256) -- what the benchmark takes, what the reference's commented
 * imwrite lines intend (DC_lidar_camera/main_lc.cpp:233-234), and the inverse of the ingest of dcmt_complete_u16_dev and
 * dcmt_evaluate_u16_dev: a dense batch leaves at 2 B/px.  Per pixel
 *     t = x * scale, one f32 rounding;  r = t rounded to nearest, ties to even;  out = r saturated to 0..65535
 * which is cv::Mat::convertTo(CV_16U, scale) on a CV_32F plane.  Negatives and both zeros give 0.  The saturation is taken on t's BIT
 * PATTERN (t may be +Inf for a finite x, and the library is built with -ffinite-math-only): a set sign bit gives 0, bits at or above
 * those of 65535.0f, as integers, give 65535.  Every payload v = 0..65535 survives v * (1/256) and back.
 * DEVICE pointers, stream-ordered: d_depth contiguous f32 [batch][rows][cols], 4-byte aligned; d_out uint16 of the same shape,
 * 2-byte aligned (both 16-byte aligned: eight pixels per access; the same bytes either way).  Never synchronises, never allocates,
 * keeps no state; same standing among other *_dev calls as dcmt_crop_frames_dev.
 * DCMT_E_INVALID: a null pointer, sizes beyond the ctx limits, a scale that is not finite and > 0, d_depth not 4-byte or d_out not
 * 2-byte aligned, any overlap of the two buffers. */
int dcmt_depth_to_u16_dev(dcmt_ctx *ctx, const float *d_depth, float scale /* 256 for KITTI */, uint16_t *d_out,
                          int rows, int cols, int batch, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES); the same bytes as the device call. */
int dcmt_depth_to_u16(dcmt_ctx *ctx, const float *depth, size_t depth_row_stride, float scale,
                      uint16_t *out, size_t out_row_stride, int rows, int cols);

/* ---- in front of the stereo calls: undistortion and rectification of camera frames ---------------------- */

/* Every stereo call of this header takes a RECTIFIED pair.  The reference's stereo-lidar main carries the step that makes one as its
 * rectify() (DC_stereo_lidar/main_sl.cpp:1350-1381, commented out there): cv::initUndistortRectifyMap on each camera's K, D, R, P,
 * then cv::remap(..., cv::INTER_LINEAR).  KITTI's unsynced+unrectified recordings and a rig of one's own deliver distorted frames
 * with exactly K_0x, D_0x (five coefficients), R_rect_0x and P_rect_0x (calib_cam_to_cam.txt).  Two device calls: the map of a
 * calibration, computed once, and the remap of a batch through it, in front of dcmt_crop_frames_dev and dcmt_bgr_convert_dev.
 * cv::stereoRectify itself is not here (the caller brings R and P), nor the rational or thin-prism models, 16-bit or f32 images, or a
 * nearest-neighbour remap of depth.  Sources of one call have ONE size: for ragged sources crop first and shift cx, cy by the
 * window's origin.
 *
 * The definition below is OURS, as with BGR->Lab and the bilateral filter: it is stated here, restated in numpy
 * (tests/rectify_restatement.py) and bit-exact from there on -- stated, never compared with an executing OpenCV.
 *
 * RECORD: dcmt_rectify_calib, 22 doubles: the distorted camera fx fy cx cy; k1 k2 p1 p2 k3; R[9] row-major, the rectifying rotation,
 * taken as orthonormal and not checked; the new camera fxp fyp cxp cyp (P_rect's left 3x3).
 *
 * MAP: for destination pixel (u, v), in f64, every operation rounded once, in exactly this order (no contraction):
 *     x  = (u - cxp) / fxp                 y  = (v - cyp) / fyp
 *     X  = (R[0]*x + R[3]*y) + R[6]        Y  = (R[1]*x + R[4]*y) + R[7]        W = (R[2]*x + R[5]*y) + R[8]     (R^T (x, y, 1))
 *     xn = X / W     yn = Y / W            x2 = xn*xn    y2 = yn*yn    r2 = x2 + y2    xy2 = (2*xn)*yn
 *     kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2
 *     xd = (xn*kr + p1*xy2) + p2*(r2 + 2*x2)
 *     yd = (yn*kr + p1*(r2 + 2*y2)) + p2*xy2
 *     mx = fx*xd + cx                      my = fy*yd + cy
 *     sx = rint(mx * 32)   sy = rint(my * 32)      ties to even: 1/32-pixel fixed point (OpenCV's INTER_BITS = 5)
 * The map element is int32 (sx, sy), 8 bytes; the map is [n_maps][rows][cols][2].  OUTSIDE is decided on the bit patterns of mx*32
 * and my*32 (the library is built with -ffinite-math-only): if either is NaN or +-Inf or has magnitude >= 2^30, BOTH coordinates of
 * the element are INT32_MIN.  A record is tested on its bits too, once per wave, as the calibration tables are: any entry that is
 * not finite, or fxp or fyp +-0, makes the whole map all-outside.
 *
 * REMAP: the source is 8-bit, 1 or 3 channels, every channel remapped on its own; samples outside the source are 0
 * (BORDER_CONSTANT).  With arithmetic shifts
 *     ix = sx >> 5   ax = sx & 31   iy = sy >> 5   ay = sy & 31
 *     out = ( (32-ay)*((32-ax)*p(iy,ix) + ax*p(iy,ix+1)) + ay*((32-ax)*p(iy+1,ix) + ax*p(iy+1,ix+1)) + 512 ) >> 10
 * where p(y, x) = 0 wherever y is not in [0, src_rows) or x not in [0, src_cols) -- which is where an outside element puts all
 * four samples.  The range test stands in front of any address arithmetic: for ANY map contents the call reads no byte outside the
 * source batch and writes none outside d_dst's.  This is OpenCV's 32 x 32 table of 15-bit bilinear weights: there 32 * wx * wy is
 * exact (an integer below 2^15), so no table is needed and none is kept.
 *
 * WHICH MAP: frame f uses map d_map_index[f]; with a NULL index, map f % n_maps -- one map for a whole batch, n_maps = 2 for
 * interleaved left and right frames, n_maps = batch for a map per frame.  An index outside 0 .. n_maps - 1 gives an all-zero frame
 * and touches no other (the convention of the *_calib_dev calls).
 *
 * rows x cols and batch are bounded by the ctx limits; the SOURCE may be larger, up to 16384 a side.  d_src and d_dst may have ANY
 * byte alignment (4-byte-aligned addresses take the wide accesses; the same bytes either way).  Two routes, bit-identical, chosen
 * per destination tile by the kernel: the tile's source bounding box staged in LDS once per frame ("lds"), or, where that box
 * exceeds the LDS budget (strong minification or rotation) or DCMT_RECTIFY_FORCE_GATHER asks, range-checked byte loads from global
 * memory ("gather").  dcmt_last_path names the routes the tiles of the last dcmt_rectify_dev call took, once that call has run:
 * "k_rectify<lds>", "k_rectify<gather>" or "k_rectify<lds+gather>".
 * Neither call synchronises, allocates or uses ctx scratch, and nothing is carried from call to call but that probe; both may be
 * enqueued in front of or behind any other *_dev call of the ctx on the same stream.  Table, map and index are read on the stream:
 * earlier work on it may have written them.
 * DCMT_E_INVALID: a null pointer (d_map_index may be NULL), channels not 1 or 3, n_maps < 1, rows x cols or batch beyond the ctx
 * limits, a source side outside 1 .. 16384, a table or map that is not 8-byte or an index that is not 4-byte aligned, unknown flag
 * bits, any overlap of d_dst with the source, the map or the index (there is no in-place form), or of d_map with the table. */
typedef struct {
    double fx, fy, cx, cy;          /* the distorted camera: K                                       */
    double k1, k2, p1, p2, k3;      /* D, in OpenCV's order                                          */
    double R[9];                    /* row-major rectifying rotation                                 */
    double fxp, fyp, cxp, cyp;      /* the new camera: P_rect's left 3x3                             */
} dcmt_rectify_calib;               /* 176 bytes; table 8-byte aligned                               */

#define DCMT_RECTIFY_FORCE_GATHER 1u /* every tile takes the gather route: tests and timing          */

int dcmt_rectify_map_dev(dcmt_ctx *ctx, const dcmt_rectify_calib *d_table /* [n_maps], device */, int n_maps, int rows, int cols,
                         int32_t *d_map /* [n_maps][rows][cols][2] */, void *stream);
int dcmt_rectify_dev(dcmt_ctx *ctx, const uint8_t *d_src /* [batch][src_rows][src_cols][channels] */, int src_rows, int src_cols,
                     int channels, const int32_t *d_map, int n_maps, const int32_t *d_map_index /* [batch] or NULL */, uint32_t flags,
                     uint8_t *d_dst /* [batch][rows][cols][channels] */, int rows, int cols, int batch, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES); the map is computed for the call.  The same bytes as the device
 * calls.  What dcmt_shim::undistort_rectify calls. */
int dcmt_rectify(dcmt_ctx *ctx, const uint8_t *src, size_t src_row_stride, int src_rows, int src_cols, int channels,
                 const dcmt_rectify_calib *calib, uint8_t *dst, size_t dst_row_stride, int rows, int cols);

/* ---- photometric error maps: get_initial_error ---------------------------------------------------------- */

/* get_initial_error(optimized_depth, img_left_copy, img_right_copy) (DC_stereo_lidar/main_sl.cpp:618-712, called at :1273), its data:
 * for every pixel of a dense depth plane, how well the right image agrees with the left one at the disparity that depth implies --
 * a confidence plane for the completion, the before / after picture of dcmt_stereo_refine_dev.  Not reproduced: error_map_show, which
 * is drawn with cv::circle (:689-701), the imshow and the prints.  The grey images are the caller's step (dcmt_bgr_convert_dev writes
 * what cv::cvtColor(BGR2GRAY) of :625, :630 writes), as for dcmt_stereo_refine_dev.
 * Per frame: depth f32 [rows][cols], left and right uint8 grey [rows][cols]; err uint8 [rows][cols].  For pixel (i = row, j = column):
 *   1. !(depth > 0): err = 0 and nothing is counted -- 0, -0, negatives and NaN (:646).
 *   2. disparity = (baseline * focal) / depth in f32: one rounded product, one rounded quotient (:648).
 *   3. t = (float)j - disparity in f32, pr = (int)t, truncated toward zero (:649).  Where t is NaN or outside int's range the
 *      reference's conversion is undefined; here such a pixel is "not inside": 0 < trunc(t) < cols is decided on the float
 *      (1 <= t < 2^31, then the exact integer against cols), before any conversion.
 *   4. !(pr > 0 && pr < cols): err = 0 (:656; both bounds as written, so column 0 is never a target).
 *   5. otherwise the pixel is VALID and ssd = sum of (left[i+p][j+k] - right[i+p][pr+k])^2 over k and p in [-window, window), a tap kept
 *      iff i+p > 0 && i+p < rows && j+k > 0 && j+k < cols && pr+k > 0 && pr+k < cols (:660-663: every lower bound strict, row 0 and
 *      column 0 are never read).  Each kept tap is one MATCH.
 *   6. err = min(255, floor(sqrt(ssd))).  The reference takes float e = sqrt(int), clamps at 255 and casts to uchar (:676-678); over
 *      every ssd a window of up to 8 x 8 taps can give, that f32 square root never crosses an integer, so the result is the integer
 *      square root (tests/test_photo_error.py checks all of them), and that is what the kernel computes, in integers.
 * Everything decided about a float is decided on its bit pattern (the library is built with -ffinite-math-only).
 * stats, four uint64 per frame: [0] valid pixels (the reference's row_cols, :657), [1] matches (:669), [2] pixels with err > 0 (counts,
 * :696), [3] the sum of err (not in the reference: the mean error without reading the plane back).  Integer sums: the same bits in
 * any order.
 *
 * DEVICE pointers, stream-ordered.  d_depth contiguous f32 [batch][rows][cols], 4-byte aligned; d_left, d_right, d_err uint8 of that
 * shape, any alignment; d_stats [batch][4] uint64, 8-byte aligned.  d_err or d_stats may be NULL, not both: without d_err the plane is
 * not stored.  16-byte aligned inputs, a 4-byte aligned d_err and cols a multiple of 16 take the wide accesses; the same bytes either
 * way.  Two enqueues whatever the data: a clear of d_stats (where given) and one kernel.  Never synchronises, never allocates, uses no
 * ctx scratch and touches none of the state a ctx carries (no flag ring, no winner plane, not what dcmt_last_path reports); may be
 * enqueued in front of or behind any other *_dev call of the ctx on the same stream, like dcmt_gaussian5_dev.
 * DCMT_E_INVALID: a null ctx, input or params, both outputs NULL, sizes beyond the ctx limits, window outside 1..4, a baseline or
 * focal that is not finite and > 0, d_depth not 4-byte or d_stats not 8-byte aligned, any overlap between an output and an input or
 * between the two outputs.  Nothing is written then. */
typedef struct {
    float   baseline;     /* 0.54f           main_sl.cpp:632 */
    float   focal;        /* 9.597910e+02f   :634            */
    int32_t window;       /* 2               :638; 1..4      */
} dcmt_photo_error_params;
void dcmt_default_photo_error_params(dcmt_photo_error_params *p);
int dcmt_photo_error_dev(dcmt_ctx *ctx, const float *d_depth, const uint8_t *d_left, const uint8_t *d_right,
                         int rows, int cols, int batch, const dcmt_photo_error_params *params,
                         uint8_t *d_err /* or NULL */, uint64_t *d_stats /* [batch][4] or NULL */, void *stream);
/* The same with each frame's own baseline and focal length: d_calib holds [batch] of the 8-byte records dcmt_stereo_refine_calib_dev
 * takes, on the device, 8-byte aligned, read by the kernel on the caller's stream with the rules of the calibration tables above;
 * params gives the window only.  Frame f is, bit for bit, what the uniform call returns for it alone with record f.  A record is
 * tested on the device, on its bits, as the uniform call tests its params (both entries finite and > 0); a frame whose record fails
 * has an all-zero plane and zero stats, and no other frame is touched.  Also DCMT_E_INVALID: a null or misaligned d_calib, or one
 * that overlaps an output. */
int dcmt_photo_error_calib_dev(dcmt_ctx *ctx, const float *d_depth, const uint8_t *d_left, const uint8_t *d_right,
                               int rows, int cols, int batch, const dcmt_photo_error_params *params,
                               const dcmt_stereo_calib *d_calib /* [batch], 8-byte aligned */,
                               uint8_t *d_err /* or NULL */, uint64_t *d_stats /* [batch][4] or NULL */, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES: depth >= 4 * cols, the images and err >= cols; the stride of a NULL
 * err is ignored); stats: four uint64 or NULL.  The same bits as the device call.  What dcmt_shim::get_initial_error calls. */
int dcmt_photo_error(dcmt_ctx *ctx, const float *depth, size_t depth_row_stride,
                     const uint8_t *left, size_t left_row_stride, const uint8_t *right, size_t right_row_stride,
                     int rows, int cols, const dcmt_photo_error_params *params,
                     uint8_t *err /* or NULL */, size_t err_row_stride, uint64_t *stats /* [4] or NULL */);

/* ---- dense stereo matching: semi-global matching on a rectified grey pair ------------------------------- */

/* The "PERFORM STEREO MATCHING" block of DC_stereo_lidar/main_sl.cpp:1293-1339 (cv::StereoSGBM, numDisparity * 16 = 64 disparities,
 * block size 4, a 16-bit fixed-point disparity map of the rectified pair), as an algorithm of this library's own: OpenCV's SGBM --
 * Birchfield-Tomasi costs on a prefiltered image, its own buffering -- cannot be restated to the bit without a running OpenCV, so the
 * matcher is STATED HERE, in integers, and the library is bit-exact against this statement (tests/sgm_restatement.py).
 * Per frame: left, right uint8 grey [rows][cols] (what dcmt_bgr_convert_dev writes).  D = num_disparities, the minimum disparity is 0,
 * the block is 5 x 5 (block sizes 4 and 5 both give half-width 2 in the reference's call).
 *   1. pixel cost  AD(y,x,d) = |left(y,x) - right(y, max(x - d, 0))|.
 *   2. block cost  C(y,x,d) = sum over dy, dx in -2..2 of AD(clamp(y+dy, 0, rows-1), clamp(x+dx, 0, cols-1), d): the clamp replicates the
 *      AD plane, not the images.  C <= 25 * 255 = 6375.
 *   1c, 2c. the census cost, only with dcmt_sgm_cost_dev and cost == DCMT_SGM_COST_CENSUS, in place of steps 1 and 2 (two cameras of a rig
 *      never share exposure, gain and vignetting; a census code depends only on the order of the grey values around a pixel):
 *      1c. codes: each image I gets a 24-bit code per pixel, K_I(y,x), one bit per (dy,dx) in -2..2 x -2..2 without the centre, set iff
 *          I(clamp(y+dy, 0, rows-1), clamp(x+dx, 0, cols-1)) < I(y,x): the comparison is strict (equal is 0) and the clamp replicates
 *          the image.  Only the popcount of an XOR of two codes is ever used, so the order of the bits is the implementation's own.
 *          pixel cost  H(y,x,d) = popcount(K_left(y,x) ^ K_right(y, max(x - d, 0))), 0..24.
 *      2c. block cost  C(y,x,d) = 10 * sum over dy, dx in -2..2 of H(clamp(y+dy, 0, rows-1), clamp(x+dx, 0, cols-1), d): this clamp
 *          replicates the H plane, exactly as step 2 replicates the AD plane.  C <= 10 * 25 * 24 = 6000.
 *      The factor 10 is part of the definition, not a tunable: it puts C on the scale of the absolute-difference cost (on uniform
 *      noise the largest C is about 4500 with census and about 4000 with absolute differences), so p1, p2, guide_weight and guide_cap
 *      keep their meaning and their defaults.  Since 6000 <= 6375 every bound of this statement holds as written with either cost:
 *      S <= paths * (6375 + p2 + guide_cap), the limits 10000 and 1800 on p2 (+ guide_cap), and uint16 volumes.  Steps 2b and 3..9
 *      read C as before.
 *   2b. guide, only with dcmt_sgm_guided_dev and a d_guide: an f32 depth plane [rows][cols] in the left camera, in metres, 0 where there is
 *      none -- what dcmt_project_points_nearest_dev writes, or a completed plane, in which every pixel is hinted.  With bf = baseline *
 *      focal, one rounded f32 product (step 9's), pixel (y,x) HAS A HINT iff the bits of z = guide(y,x) are those of a finite number > 0
 *      (decided on the bits, as dcmt_photo_error_dev decides), and t = q + 0.5f with q = bf / z, one rounded f32 quotient and one rounded
 *      f32 sum, satisfies t < (float)D.  The hint is h = (int)t, 0 <= h <= D-1.  NaN, +-inf, negatives, -0.0 and a z so small that q
 *      overflows or lands beyond the range give no hint; a very large z gives h = 0, which is a hint.  At a hinted pixel
 *        C'(y,x,d) = C(y,x,d) + min(guide_weight * |d - h|, guide_cap),
 *      elsewhere C' = C; steps 3..9 read C' wherever they read C, and the cost volume in the workspace holds C'.  The term is
 *      additive, integer and capped: C' <= 6375 + guide_cap, C' <= L_r <= C' + p2 and S <= paths * (6375 + p2 + guide_cap), so with a
 *      guide the limit on p2 (10000, with eight paths 1800) bounds p2 + guide_cap.  The bound is attained: a comb image with a hint of 0
 *      on every pixel reaches S = 65500 with four paths (p1 = p2 = guide_cap = 5000) and 65400 with eight (900).  guide_weight = 0 or
 *      guide_cap = 0 is the unguided matcher bit for bit, in both volumes.
 *   3. paths, four directions r (left->right, right->left, top->bottom, bottom->top).  On the first pixel of a path L_r = C; otherwise,
 *      with m = min over k of L_r(p-r, k):
 *        L_r(p,d) = C(p,d) + min(L_r(p-r,d), L_r(p-r,d-1) + p1, L_r(p-r,d+1) + p1, m + p2) - m,
 *      neighbours d-1 < 0 and d+1 >= D absent.  Then C <= L_r <= C + p2, so S = sum over r of L_r <= 4 * (6375 + 10000) = 65500: S and
 *      every L_r fit uint16, which is why p2 <= 10000.  With p1 = p2 = 0: L_r = C, S = 4 C, plain block matching.
 *      With paths == 8 (dcmt_sgm_paths_dev) four more directions r = (dy, dx) are added: (+1,+1), (-1,-1), (+1,-1), (-1,+1).  Each path
 *      is a maximal diagonal line of the frame: it starts on the pixel of the line that has no predecessor p - r inside the frame,
 *      where L_r = C, and ends where it leaves the frame; the recurrence, p1, p2 and the absent neighbours are those above.  S is the
 *      sum of all eight L_r <= 8 * (6375 + p2), which fits uint16 for p2 <= 1816: with eight paths p2 <= 1800, so S <= 65400.  With
 *      p1 = p2 = 0: S = 8 C.  Steps 4..9 do not depend on the number of paths.
 *   4. winner      d* = the lowest d that minimises S(y,x,.).
 *   5. uniqueness  invalid if some d with |d - d*| > 1 has S(d) * (100 - uniqueness) < S(d*) * 100.
 *   6. inside      invalid if x - d* < 0.
 *   7. left-right check, if disp12_max_diff >= 0: dR(y,x') = the lowest k that minimises S(y, x'+k, k) over k < D with x'+k < cols;
 *      invalid if |dR(y, x - d*) - d*| > disp12_max_diff.
 *   8. sub-pixel   d* = 0 or d* = D-1: frac = 0.  Otherwise a = S(d*-1), b = S(d*+1), den = max(a + b - 2 S(d*), 1),
 *      frac = floor(((a - b) * 16 + den) / (2 den)) -- the floor, not C's truncation; since |a - b| <= den the unsigned form
 *      ((a - b + den) * 16 + den) / (2 den) - 8 is the same number.  disp16 = 16 d* + frac.
 *   9. outputs     d_disp16 int16 [batch][rows][cols]: disp16, -16 where invalid (StereoSGBM::compute's CV_16S convention: 4 fractional
 *      bits, (minDisparity - 1) * 16).  d_depth f32 [batch][rows][cols]: where disp16 > 0,
 *      min((baseline * focal) / (disp16 / 16.0f), max_depth), one rounded product and one rounded quotient in f32 (the disparity > 0 /
 *      clamp rule of retrieve_optimized_depth, :871-879); otherwise 0.  dcmt_stereo_refine_dev, dcmt_photo_error_dev, dcmt_evaluate_dev
 *      and dcmt_colorize_dev take this plane as it is.  Either output may be NULL, not both.
 *
 * DEVICE pointers, stream-ordered.  d_work is the CALLER's workspace (the cost volume C and the sum volume S, uint16 [rows][cols][D]
 * each, per frame in flight): dcmt_sgm_workspace_bytes(rows, cols, D, frames) bytes hold `frames` frames (0 for arguments the call
 * would refuse); the call works through the batch in chunks of as many frames as work_bytes holds, at most `batch`.  At
 * 352 x 1216 x 64 one frame is 110 MB, which is why the workspace is not a context buffer sized by max_batch.  Nothing is carried in
 * it from call to call and nothing in it need be initialised.  Three kernels per chunk (rows, columns, winner).  Never synchronises,
 * never allocates, touches none of the state a ctx carries; may be enqueued in front of or behind any other *_dev call.
 * DCMT_E_INVALID, nothing written: a null ctx, image, params or workspace; both outputs NULL; sizes beyond the ctx limits;
 * num_disparities not a multiple of 16 in 16..128; p1 < 0, p1 > p2 or p2 > 10000; uniqueness outside 0..100; with d_depth, a baseline,
 * focal or max_depth that is not finite and > 0; d_disp16 not 2-byte, d_depth not 4-byte or d_work not 16-byte aligned; work_bytes
 * below one frame; any overlap among the outputs, the inputs and the workspace. */
typedef struct {
    int32_t num_disparities;  /* 64      main_sl.cpp:1306 (numDisparity * 16); a multiple of 16 in 16..128 */
    int32_t p1;               /* 200     0 <= p1 <= p2                                                      */
    int32_t p2;               /* 800     <= 10000                                                           */
    int32_t uniqueness;       /* 10      0..100, per cent                                                   */
    int32_t disp12_max_diff;  /* 1       < 0: no left-right check                                           */
    float   baseline;         /* 0.54f           main_sl.cpp:632                                            */
    float   focal;            /* 9.597910e+02f   :634                                                       */
    float   max_depth;        /* 100.0f                                                                     */
} dcmt_sgm_params;
void dcmt_default_sgm_params(dcmt_sgm_params *p);
size_t dcmt_sgm_workspace_bytes(int rows, int cols, int num_disparities, int frames);
int dcmt_sgm_dev(dcmt_ctx *ctx, const uint8_t *d_left, const uint8_t *d_right,
                 int16_t *d_disp16 /* or NULL */, float *d_depth /* or NULL */, int rows, int cols, int batch,
                 const dcmt_sgm_params *params, void *d_work /* 16-byte aligned */, size_t work_bytes, void *stream);
/* The same with the number of paths of step 3 as an argument: 4 (dcmt_sgm_dev itself, bit for bit and launch for launch) or 8 (the four
 * diagonals as well: two more launches per chunk, one per orientation of the diagonals, between the columns and the winner).  The
 * workspace (dcmt_sgm_workspace_bytes serves both), the chunking, every refusal and every guarantee are those of dcmt_sgm_dev;
 * besides, DCMT_E_INVALID, nothing written: paths other than 4 or 8; paths == 8 with p2 > 1800. */
int dcmt_sgm_paths_dev(dcmt_ctx *ctx, const uint8_t *d_left, const uint8_t *d_right,
                       int16_t *d_disp16 /* or NULL */, float *d_depth /* or NULL */, int rows, int cols, int batch,
                       const dcmt_sgm_params *params, int paths,
                       void *d_work /* 16-byte aligned */, size_t work_bytes, void *stream);
/* The same with a guide (step 2b): d_guide f32 [batch][rows][cols], or NULL.  With d_guide == NULL this IS dcmt_sgm_paths_dev -- the
 * same launches of the same kernels, guide_weight and guide_cap not looked at -- and dcmt_sgm_paths_dev is that case of this entry
 * point.  With a guide the rows kernel is its guided variant, which converts each guide row once (one division a pixel); every
 * other kernel, the workspace (dcmt_sgm_workspace_bytes serves all three entry points), the chunking and every guarantee are
 * unchanged.  The defaults of the Python interface are guide_weight = 100 and guide_cap = 1000: with p2 = 800 exactly the eight-path
 * limit.  Besides the refusals of dcmt_sgm_paths_dev, DCMT_E_INVALID, nothing written, when a guide is given: d_guide not 4-byte
 * aligned; guide_weight outside 0..10000; guide_cap < 0; p2 + guide_cap > 10000 (with eight paths 1800); a baseline or focal that
 * is not finite and > 0, also when d_depth is NULL (max_depth is still tested only with d_depth); any overlap of the guide with an
 * output or the workspace (it may share memory with the images). */
int dcmt_sgm_guided_dev(dcmt_ctx *ctx, const uint8_t *d_left, const uint8_t *d_right, const float *d_guide /* or NULL */,
                        int16_t *d_disp16 /* or NULL */, float *d_depth /* or NULL */, int rows, int cols, int batch,
                        const dcmt_sgm_params *params, int paths, int guide_weight, int guide_cap,
                        void *d_work /* 16-byte aligned */, size_t work_bytes, void *stream);
/* The same with the pixel cost as an argument: DCMT_SGM_COST_ABSDIFF (steps 1 and 2: dcmt_sgm_guided_dev itself, which is that case of
 * this entry point -- the same launches of the same kernels) or DCMT_SGM_COST_CENSUS (steps 1c and 2c).  With census the rows kernel is
 * its census variant, with or without a guide, which makes the codes of the rows it needs while it stages them (16 bytes of LDS a column,
 * 18 with a guide, as with absolute differences); every other kernel, the workspace (dcmt_sgm_workspace_bytes serves all four entry points: census needs nothing
 * beyond C and S), the chunking, every refusal and every guarantee are those of dcmt_sgm_guided_dev.  Besides, DCMT_E_INVALID,
 * nothing written: a cost other than these two. */
#define DCMT_SGM_COST_ABSDIFF 0
#define DCMT_SGM_COST_CENSUS 1
int dcmt_sgm_cost_dev(dcmt_ctx *ctx, const uint8_t *d_left, const uint8_t *d_right, const float *d_guide /* or NULL */,
                      int16_t *d_disp16 /* or NULL */, float *d_depth /* or NULL */, int rows, int cols, int batch,
                      const dcmt_sgm_params *params, int paths, int guide_weight, int guide_cap, int cost,
                      void *d_work /* 16-byte aligned */, size_t work_bytes, void *stream);
/* HOST pointers, one pair, synchronous (row strides in BYTES: the images >= cols, disp16 >= 2 * cols, depth >= 4 * cols; the stride
 * of a NULL output is ignored).  The workspace of one frame is allocated for the call.  The same bits as the device call.  What
 * dcmt_shim::stereo_sgm calls. */
int dcmt_sgm(dcmt_ctx *ctx, const uint8_t *left, size_t left_row_stride, const uint8_t *right, size_t right_row_stride,
             int rows, int cols, const dcmt_sgm_params *params,
             int16_t *disp16 /* or NULL */, size_t disp16_row_stride, float *depth /* or NULL */, size_t depth_row_stride);
/* dcmt_sgm with the number of paths, 4 or 8, as dcmt_sgm_paths_dev takes it; dcmt_sgm is its paths = 4.  What
 * dcmt_shim::stereo_sgm_paths calls. */
int dcmt_sgm_paths(dcmt_ctx *ctx, const uint8_t *left, size_t left_row_stride, const uint8_t *right, size_t right_row_stride,
                   int rows, int cols, const dcmt_sgm_params *params,
                   int16_t *disp16 /* or NULL */, size_t disp16_row_stride, float *depth /* or NULL */, size_t depth_row_stride,
                   int paths);
/* dcmt_sgm_paths with a guide, as dcmt_sgm_guided_dev takes it: guide f32 [rows][cols] with a row stride in BYTES >= 4 * cols, or NULL
 * (its stride is then ignored: dcmt_sgm_paths, which is that case).  What dcmt_shim::stereo_sgm_guided calls. */
int dcmt_sgm_guided(dcmt_ctx *ctx, const uint8_t *left, size_t left_row_stride, const uint8_t *right, size_t right_row_stride,
                    const float *guide /* or NULL */, size_t guide_row_stride, int rows, int cols, const dcmt_sgm_params *params,
                    int16_t *disp16 /* or NULL */, size_t disp16_row_stride, float *depth /* or NULL */, size_t depth_row_stride,
                    int paths, int guide_weight, int guide_cap);
/* dcmt_sgm_guided with the pixel cost, as dcmt_sgm_cost_dev takes it; dcmt_sgm_guided is its DCMT_SGM_COST_ABSDIFF.  What
 * dcmt_shim::stereo_sgm_cost calls. */
int dcmt_sgm_cost(dcmt_ctx *ctx, const uint8_t *left, size_t left_row_stride, const uint8_t *right, size_t right_row_stride,
                  const float *guide /* or NULL */, size_t guide_row_stride, int rows, int cols, const dcmt_sgm_params *params,
                  int16_t *disp16 /* or NULL */, size_t disp16_row_stride, float *depth /* or NULL */, size_t depth_row_stride,
                  int paths, int guide_weight, int guide_cap, int cost);

/* ---- the speckle filter of a disparity map ------------------------------------------------------------- */

/* The step cv::StereoSGBM runs on its own output: small connected blobs of disparity that disagree with their surroundings become
 * invalid.  The reference names its parameters beside the matcher in every stereo main (DC_stereo_lidar/main_sl.cpp:1301-1302,
 * :1315-1316: speckleWindowSize = 200, speckleRange = 2), and StereoSGBM applies them as filterSpeckles on (disp,
 * (minDisparity - 1) * 16, speckleWindowSize, 16 * speckleRange).  This is cv::filterSpeckles with (img, newVal, maxSpeckleSize,
 * maxDiff) for CV_16S as OpenCV documents it: a flood fill over a symmetric neighbour relation, so its result is the connected
 * components of a graph, independent of the scan order, and it is STATED HERE to the last bit, in integers.  No OpenCV is run; the
 * library is bit-exact against two restatements of this statement (tests/speckle_restatement.py).
 * Per frame: disp16 int16 [rows][cols]; parameters max_size, max_diff, new_val.
 *   1. a pixel is LIVE iff its value != new_val.
 *   2. two live pixels that are 4-neighbours share an EDGE iff |a - b| <= max_diff, the difference taken in int arithmetic: -32768
 *      against 32767 is 65535, never a wrapped value.
 *   3. a COMPONENT is a connected component of the live pixels under those edges.  The relation is not transitive: the ramp 0,
 *      max_diff, 2 * max_diff, ... is one component.
 *   4. a component of size <= max_size is a speckle: each of its pixels becomes new_val.  max_size = 0 changes nothing.
 *   5. every other pixel keeps its bits; pixels equal to new_val are never touched.
 * d_depth, f32 [batch][rows][cols], modified IN PLACE, or NULL: a pixel whose disparity this call turned into new_val becomes +0.0f,
 * every other pixel keeps its bits -- the plane dcmt_sgm_dev wrote beside disp16 stays consistent without being recomputed.
 * d_removed, uint32 [batch], or NULL: the number of pixels the call changed in each frame.  Integer sums: the same bits in any order.
 * The result is independent of the batch size, the frame's position in the batch, alignment, launch geometry and the run.
 *
 * DEVICE pointers, stream-ordered.  d_disp16 and d_out contiguous int16 [batch][rows][cols], 2-byte aligned (8-byte aligned planes of
 * frames of a multiple of 4 pixels take the wide accesses; the same bits either way); d_out may BE d_disp16, which gives the bits of
 * an out-of-place call: the last kernel is the only writer of d_out and d_depth.  A clear of d_removed (where given) and four kernels,
 * three where a frame is a single tile of 64 x 16 pixels, whatever the data.  Never synchronises, never allocates.  Scratch: the two
 * planes of one 32-bit word per pixel the ctx allocates when it is created, the ones dcmt_slic_connectivity_dev borrows; no other
 * ctx state is touched (no flag ring, no winner plane, not what dcmt_last_path reports): may be enqueued in front of or behind any
 * other *_dev call of the ctx on the same stream.
 * DCMT_E_INVALID, nothing written: a null ctx, input, output or params; sizes or batch beyond the ctx limits; max_size < 0; max_diff
 * outside 0..65535; new_val outside int16; d_disp16 or d_out not 2-byte aligned, d_depth or d_removed not 4-byte aligned; any overlap
 * among the buffers other than d_out == d_disp16 exactly. */
typedef struct {
    int32_t max_size;     /* 200   main_sl.cpp:1301 speckleWindowSize; >= 0                                  */
    int32_t max_diff;     /* 32    16 * speckleRange (:1302), in sixteenths, the unit of disp16; 0..65535    */
    int32_t new_val;      /* -16   what dcmt_sgm_dev writes for "none"; an int16                             */
} dcmt_speckle_params;
void dcmt_default_speckle_params(dcmt_speckle_params *p);
int dcmt_filter_speckles_dev(dcmt_ctx *ctx, const int16_t *d_disp16, int16_t *d_out /* may be d_disp16 */,
                             float *d_depth /* in place, or NULL */, int rows, int cols, int batch,
                             const dcmt_speckle_params *params, uint32_t *d_removed /* [batch] or NULL */, void *stream);
/* HOST pointers, one frame, synchronous (row strides in BYTES: disp16 and out >= 2 * cols, depth >= 4 * cols; the stride of a NULL
 * depth is ignored); out may be disp16; removed: one uint32 or NULL.  The same bits as the device call.  What
 * dcmt_shim::filter_speckles calls. */
int dcmt_filter_speckles(dcmt_ctx *ctx, const int16_t *disp16, size_t row_stride, int16_t *out, size_t out_row_stride,
                         float *depth /* or NULL */, size_t depth_row_stride, int rows, int cols,
                         const dcmt_speckle_params *params, uint32_t *removed /* or NULL */);

/* ---- the same three on HOST memory (one frame, synchronous): what the cv::Mat shim calls ---------------- */

/* Each copies its inputs to the device, runs the device entry point above and copies the result back; device buffers
 * are allocated for the call and freed again (these calls are bound by the PCIe copies, not by that).
 * Row strides in BYTES (cv::Mat::step); labels / centres / points are contiguous. */
int dcmt_project_points(dcmt_ctx *ctx, const float *points, int n_points, const float T[16], const float P[12],
                        float *sparse, size_t sparse_row_stride, int rows, int cols);
int dcmt_slic_labels(dcmt_ctx *ctx, const uint8_t *lab, size_t lab_row_stride, int rows, int cols, int step, int nc,
                     int32_t *labels /* [rows][cols] */, double *centers /* [n][5] or NULL */);
int dcmt_stereo_refine(dcmt_ctx *ctx, const float *depth, size_t depth_row_stride,
                       const uint8_t *left, size_t left_row_stride, const uint8_t *right, size_t right_row_stride,
                       float *refined, size_t refined_row_stride, int rows, int cols,
                       const dcmt_stereo_params *params);

/* ---- probes ------------------------------------------------------------------------ */

/* Per frame of the last call on ctx: the number of iterations the reference's while-loop
 * (img_completion.cpp:146-166) ran (>= 1), i.e. the length of the hole-count sequence it
 * prints.  Synchronises with the last call's stream.  out[i] = -1 for a frame that still
 * had holes when the launches ran out (then the return value is DCMT_E_NOT_CONVERGED). */
int dcmt_last_fill_iters(dcmt_ctx *ctx, int *out, int n);
/* Per frame of the last call: holes seen by the first 31x31 fill (img_completion.cpp:131-144). */
int dcmt_last_holes_after_extend(dcmt_ctx *ctx, int *out, int n);

const char *dcmt_strerror(int status);
int dcmt_last_hip_error(const dcmt_ctx *ctx);
/* The kernels the last cascade call on ctx dispatched, e.g. "k_pre_p<Q16OUT> + k_fp_q" (the dispatch depends on batch size,
 * frame shape, alignment and -- for the 16-bit form -- on what earlier calls found in their frames).  Owned by ctx.  After a
 * dcmt_rectify_dev call: the routes its tiles took, "k_rectify<lds>", "k_rectify<gather>" or "k_rectify<lds+gather>" (static
 * strings); the kernel says which, so this copies two words back from the device and is meaningful once that call has run (plain
 * "k_rectify" before). */
const char *dcmt_last_path(const dcmt_ctx *ctx);

/* Measurement aid (bench.py's live per-kernel split).  With timing on, the streaming path of every following *_dev call
 * records HIP events on the caller's stream around its kernel groups (a few microseconds per call; off by default).
 * dcmt_last_kernel_times synchronises with the last call's stream and returns milliseconds:
 *   ms[0] the kernels in front of H5 that the call added (label-masked stage, normalisation scan; 0 for img_completion),
 *   ms[1] k_pre_s (H2..H6, or H5..H6 behind the label stage),  ms[2] k_fp_s (H7..H11),
 *   ms[3] the launches behind it (hole-closure redo / loop / recompute: near zero unless a frame needed the loop).
 * DCMT_E_INVALID if timing was off for the last call or the call did not take the streaming path. */
#define DCMT_N_KERNEL_TIMES 4
int dcmt_set_kernel_timing(dcmt_ctx *ctx, int on);
int dcmt_last_kernel_times(dcmt_ctx *ctx, float ms[DCMT_N_KERNEL_TIMES]);
int dcmt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DCMT_H */
