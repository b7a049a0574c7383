// dcmt_host.hip -- the synchronous host entry points: copy the caller's planes to the device, run the device call on the context's
// own stream, copy the results back, synchronise.  The single-frame variants of the *_dev entry points stage in temporary buffers
// and call dcmt.h's public *_dev function with batch = 1.  dcmt_complete_f32 and dcmt_complete_labeled_f32 (the cv::Mat entry
// points, called once per frame in a loop) stage batches in buffers the context keeps, and reach the cascade through the two
// internal declarations of dcmt_ctx.h -- check_params and complete_sync -- because they run the hole-closure loop with the counters
// read back, which the public ABI does not offer.  No kernel is compiled: this translation unit emits no device code.
#include <algorithm>
#include <cstdio>
#include <initializer_list>

#include "dcmt.h"
#include "dcmt_ctx.h"

using namespace dcmt;

namespace {

// One plane of a call: `rows` rows of `row_bytes` bytes, `pitch` bytes apart in host memory and packed in its device copy, which
// is freed when the call returns, whatever path it takes.  A null host pointer is an optional plane the caller left out: it
// gets no device copy and dev stays null.
struct Plane {
    void* host;
    size_t pitch, row_bytes, rows;
    void* dev = nullptr;
    Plane(const void* h, size_t p, size_t rb, size_t r) : host(const_cast<void*>(h)), pitch(p), row_bytes(rb), rows(r) {}
    Plane(const void* h, size_t bytes) : Plane(h, bytes, bytes, 1) {}          // a flat buffer
    ~Plane() { if (dev) (void)hipFree(dev); }
    Plane(const Plane&) = delete;
    Plane& operator=(const Plane&) = delete;
};
using Planes = std::initializer_list<Plane*>;

// One plane between host rows `pitch` bytes apart and its packed device copy, enqueued on the context's own stream: a linear copy
// where the host rows are packed too (the usual cv::Mat), a pitched one otherwise.
int copy_plane(dcmt_ctx* ctx, void* dev, void* host, size_t pitch, size_t row_bytes, size_t rows, hipMemcpyKind kind)
{
    const bool up = kind == hipMemcpyHostToDevice;
    if (pitch == row_bytes || rows == 1) DCMT_HIP(ctx, hipMemcpyAsync(up ? dev : host, up ? host : dev, row_bytes * rows, kind, ctx->own_stream));
    else DCMT_HIP(ctx, hipMemcpy2DAsync(up ? dev : host, up ? row_bytes : pitch, up ? host : dev, up ? pitch : row_bytes, row_bytes, rows, kind, ctx->own_stream));
    return DCMT_OK;
}

// Checks the pitches, gets the context's own stream (created on first use), allocates every plane and only then enqueues the
// uploads of `ins`: an allocation that fails leaves nothing of the call in the stream.
int stage(dcmt_ctx* ctx, Planes ins, Planes outs)
{
    for (Planes l : {ins, outs})
        for (Plane* p : l) if (p->host && p->pitch < p->row_bytes) return DCMT_E_INVALID;
    if (!ctx->own_stream) DCMT_HIP(ctx, hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    for (Planes l : {ins, outs})
        for (Plane* p : l) if (p->host) DCMT_HIP(ctx, hipMalloc(&p->dev, std::max<size_t>(p->row_bytes * p->rows, 1)));
    for (Plane* p : ins)
        if (p->host && p->row_bytes) DCMT_TRY(copy_plane(ctx, p->dev, p->host, p->pitch, p->row_bytes, p->rows, hipMemcpyHostToDevice));
    return DCMT_OK;
}

// Copies `outs` back behind whatever the call enqueued and waits for it all.
int fetch(dcmt_ctx* ctx, Planes outs)
{
    for (Plane* p : outs)
        if (p->host && p->row_bytes) DCMT_TRY(copy_plane(ctx, p->dev, p->host, p->pitch, p->row_bytes, p->rows, hipMemcpyDeviceToHost));
    DCMT_HIP(ctx, hipStreamSynchronize(ctx->own_stream));
    return DCMT_OK;
}

// dcmt_complete_f32 / dcmt_complete_labeled_f32: frame f of a plane starts f * its frame stride (sfs / lfs / dfs) bytes behind the
// pointer.  The staging buffers are the context's, sized for its maxima by the first call and kept (d_lab by the first labeled call).
int host_call(dcmt_ctx* ctx, const float* src, size_t srs, size_t sfs, const int32_t* labels, size_t lrs, size_t lfs,
              int n_labels, int use_superpixel, float* dst, size_t drs, size_t dfs, int rows, int cols, int batch,
              const dcmt_params* p, bool force_gaussian)
{
    DCMT_TRY(check_params(ctx, src, dst, rows, cols, batch, p));
    if (srs < sizeof(float) * (size_t)cols || drs < sizeof(float) * (size_t)cols) return DCMT_E_INVALID;
    if (labels && lrs < sizeof(int32_t) * (size_t)cols) return DCMT_E_INVALID;
    const size_t staged = ctx->frame_elems * (size_t)ctx->max_batch;
    DCMT_TRY(ctx->d_in.reserve(ctx, staged));
    DCMT_TRY(ctx->d_out.reserve(ctx, staged));
    if (labels) DCMT_TRY(ctx->d_lab.reserve(ctx, staged));
    if (!ctx->own_stream) DCMT_HIP(ctx, hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    hipStream_t st = ctx->own_stream;
    const size_t fe = (size_t)rows * cols, row_b = sizeof(float) * (size_t)cols;
    if (p->verbose == 1) {
        // what img_completion prints before it starts (LO :29, :41-50): the dimensions and the largest input value (start value 0.0, :22)
        std::printf("NUMERO ROWS, COLS: %d %d\n", rows, cols);
        for (int f = 0; f < batch; ++f) {
            float mx = 0.0f;
            for (int r = 0; r < rows; ++r) {
                const float* row = reinterpret_cast<const float*>(reinterpret_cast<const char*>(src) + f * sfs + r * srs);
                for (int c = 0; c < cols; ++c) mx = row[c] > mx ? row[c] : mx;
            }
            std::printf("max range is%g\n", (double)mx);               // operator<<(float): six significant digits, as %g
        }
    }
    for (int f = 0; f < batch; ++f) {
        DCMT_TRY(copy_plane(ctx, ctx->d_in + f * fe, (char*)src + f * sfs, srs, row_b, rows, hipMemcpyHostToDevice));
        if (labels) DCMT_TRY(copy_plane(ctx, ctx->d_lab + f * fe, (char*)labels + f * lfs, lrs, row_b, rows, hipMemcpyHostToDevice));
    }
    if (ctx->knobs.poison)   // DCMT_POISON=1: stale output can never pass for fresh output (tests)
        DCMT_HIP(ctx, hipMemsetAsync(ctx->d_out, 0xFF, sizeof(float) * fe * batch, st));
    const Frames fr = {ctx->d_in, nullptr, 1.0f, labels && use_superpixel ? ctx->d_lab.p : nullptr, n_labels, ctx->d_out, rows, cols, batch};
    const int chain_rc = complete_sync(ctx, fr, p, force_gaussian, st);
    if (chain_rc != DCMT_OK && chain_rc != DCMT_E_NOT_CONVERGED) return chain_rc;
    for (int f = 0; f < batch; ++f) DCMT_TRY(copy_plane(ctx, ctx->d_out + f * fe, (char*)dst + f * dfs, drs, row_b, rows, hipMemcpyDeviceToHost));
    DCMT_HIP(ctx, hipStreamSynchronize(st));
    return chain_rc;
}

}  // namespace

// Every single-frame variant: its own null checks and the frame against the context's maxima (before anything is allocated), stage, the
// *_dev call -- which reports what only it can detect (a NaN matrix, step < 6) --, fetch.
extern "C" {

int dcmt_complete_f32(dcmt_ctx* ctx, const float* src, size_t srs, size_t sfs, float* dst, size_t drs, size_t dfs,
                      int rows, int cols, int batch, const dcmt_params* params)
{
    DCMT_ON_DEVICE(ctx);
    return host_call(ctx, src, srs, sfs, nullptr, 0, 0, 0, 0, dst, drs, dfs, rows, cols, batch, params, false);
}

int dcmt_complete_labeled_f32(dcmt_ctx* ctx, const float* src, size_t srs, size_t sfs, const int32_t* labels, size_t lrs,
                              size_t lfs, int n_labels, float* dst, size_t drs, size_t dfs, int rows, int cols, int batch,
                              const dcmt_params* params, int use_superpixel)
{
    DCMT_ON_DEVICE(ctx);
    if (!labels) return DCMT_E_INVALID;
    return host_call(ctx, src, srs, sfs, labels, lrs, lfs, n_labels, use_superpixel, dst, drs, dfs, rows, cols, batch,
                     params, true);
}

// dcmt_project_points and dcmt_project_points_nearest: the same staging around dev_call, the *_dev entry point of either rule
static int project_points_host(decltype(&dcmt_project_points_dev) dev_call, dcmt_ctx* ctx, const float* points, int n_points, const float T[16],
                               const float P[12], float* sparse, size_t srs, int rows, int cols)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !sparse || !T || !P || n_points < 0 || (n_points > 0 && !points) || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const int32_t offsets[2] = {0, n_points};
    Plane pts(points, sizeof(float) * 4 * (size_t)n_points), off(offsets, sizeof offsets), out(sparse, srs, sizeof(float) * (size_t)cols, rows);
    int rc = stage(ctx, {&pts, &off}, {&out});
    if (rc == DCMT_OK)
        rc = dev_call(ctx, (const float*)pts.dev, (const int32_t*)off.dev, n_points, 1, T, P, (float*)out.dev, rows, cols, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&out}) : rc;
}

int dcmt_project_points(dcmt_ctx* ctx, const float* points, int n_points, const float T[16], const float P[12],
                        float* sparse, size_t srs, int rows, int cols)
{
    return project_points_host(dcmt_project_points_dev, ctx, points, n_points, T, P, sparse, srs, rows, cols);
}

int dcmt_project_points_nearest(dcmt_ctx* ctx, const float* points, int n_points, const float T[16], const float P[12],
                                float* sparse, size_t srs, int rows, int cols)
{
    return project_points_host(dcmt_project_points_nearest_dev, ctx, points, n_points, T, P, sparse, srs, rows, cols);
}

int dcmt_slic_labels(dcmt_ctx* ctx, const uint8_t* lab, size_t lrs, int rows, int cols, int step, int nc, int32_t* labels, double* centers)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !lab || !labels || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const int n = dcmt_slic_num_centers(rows, cols, step);
    Plane in(lab, lrs, 3 * (size_t)cols, rows), out(labels, sizeof(int32_t) * (size_t)rows * cols), cen(centers, sizeof(double) * 5 * (size_t)n);
    int rc = stage(ctx, {&in}, {&out, &cen});
    if (rc == DCMT_OK) rc = dcmt_slic_labels_dev(ctx, (const uint8_t*)in.dev, rows, cols, 1, step, nc, (int32_t*)out.dev, (double*)cen.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&out, &cen}) : rc;
}

int dcmt_stereo_refine(dcmt_ctx* ctx, const float* depth, size_t drs, const uint8_t* left, size_t lrs, const uint8_t* right, size_t rrs,
                       float* refined, size_t ors, int rows, int cols, const dcmt_stereo_params* params)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !depth || !left || !right || !refined || !params || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const size_t frow = sizeof(float) * (size_t)cols;
    Plane d(depth, drs, frow, rows), l(left, lrs, cols, rows), r(right, rrs, cols, rows), out(refined, ors, frow, rows);
    int rc = stage(ctx, {&d, &l, &r}, {&out});
    if (rc == DCMT_OK)
        rc = dcmt_stereo_refine_dev(ctx, (const float*)d.dev, (const uint8_t*)l.dev, (const uint8_t*)r.dev, (float*)out.dev, rows, cols, 1, params, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&out}) : rc;
}

int dcmt_photo_error(dcmt_ctx* ctx, const float* depth, size_t drs, const uint8_t* left, size_t lrs, const uint8_t* right, size_t rrs, int rows, int cols,
                     const dcmt_photo_error_params* params, uint8_t* err, size_t ers, uint64_t* stats)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !depth || !left || !right || (!err && !stats) || !params || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    Plane d(depth, drs, sizeof(float) * (size_t)cols, rows), l(left, lrs, cols, rows), r(right, rrs, cols, rows);
    Plane e(err, ers, cols, rows), s(stats, 4 * sizeof(uint64_t));
    int rc = stage(ctx, {&d, &l, &r}, {&e, &s});
    if (rc == DCMT_OK)
        rc = dcmt_photo_error_dev(ctx, (const float*)d.dev, (const uint8_t*)l.dev, (const uint8_t*)r.dev, rows, cols, 1, params, (uint8_t*)e.dev,
                                  (uint64_t*)s.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&e, &s}) : rc;
}

int dcmt_sgm_cost(dcmt_ctx* ctx, const uint8_t* left, size_t lrs, const uint8_t* right, size_t rrs, const float* guide, size_t grs, int rows, int cols,
                  const dcmt_sgm_params* params, int16_t* disp16, size_t drs, float* depth, size_t zrs, int paths, int guide_weight, int guide_cap, int cost)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !left || !right || (!disp16 && !depth) || !params || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    if (paths != 4 && paths != 8) return DCMT_E_INVALID;    // before anything is allocated or staged
    if (cost != DCMT_SGM_COST_ABSDIFF && cost != DCMT_SGM_COST_CENSUS) return DCMT_E_INVALID;
    const size_t work_bytes = dcmt_sgm_workspace_bytes(rows, cols, params->num_disparities, 1);
    if (!work_bytes) return DCMT_E_INVALID;
    Plane l(left, lrs, cols, rows), r(right, rrs, cols, rows), g(guide, grs, sizeof(float) * (size_t)cols, rows);     // a null guide: no plane
    Plane d(disp16, drs, sizeof(int16_t) * (size_t)cols, rows), z(depth, zrs, sizeof(float) * (size_t)cols, rows);
    struct Workspace {                      // the one frame of workspace: device memory only, freed when the call returns
        void* dev = nullptr;
        ~Workspace() { if (dev) (void)hipFree(dev); }
    } work;
    DCMT_HIP(ctx, hipMalloc(&work.dev, work_bytes));        // before stage(): nothing of the call is in the stream if it fails
    int rc = stage(ctx, {&l, &r, &g}, {&d, &z});
    if (rc == DCMT_OK)
        rc = dcmt_sgm_cost_dev(ctx, (const uint8_t*)l.dev, (const uint8_t*)r.dev, (const float*)g.dev, (int16_t*)d.dev, (float*)z.dev, rows, cols, 1, params,
                               paths, guide_weight, guide_cap, cost, work.dev, work_bytes, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&d, &z}) : rc;
}

int dcmt_sgm_guided(dcmt_ctx* ctx, const uint8_t* left, size_t lrs, const uint8_t* right, size_t rrs, const float* guide, size_t grs, int rows, int cols,
                    const dcmt_sgm_params* params, int16_t* disp16, size_t drs, float* depth, size_t zrs, int paths, int guide_weight, int guide_cap)
{
    return dcmt_sgm_cost(ctx, left, lrs, right, rrs, guide, grs, rows, cols, params, disp16, drs, depth, zrs, paths, guide_weight, guide_cap,
                         DCMT_SGM_COST_ABSDIFF);
}

int dcmt_sgm_paths(dcmt_ctx* ctx, const uint8_t* left, size_t lrs, const uint8_t* right, size_t rrs, int rows, int cols, const dcmt_sgm_params* params,
                   int16_t* disp16, size_t drs, float* depth, size_t zrs, int paths)
{
    return dcmt_sgm_guided(ctx, left, lrs, right, rrs, nullptr, 0, rows, cols, params, disp16, drs, depth, zrs, paths, 0, 0);
}

int dcmt_sgm(dcmt_ctx* ctx, const uint8_t* left, size_t lrs, const uint8_t* right, size_t rrs, int rows, int cols, const dcmt_sgm_params* params,
             int16_t* disp16, size_t drs, float* depth, size_t zrs)
{
    return dcmt_sgm_paths(ctx, left, lrs, right, rrs, rows, cols, params, disp16, drs, depth, zrs, 4);
}

int dcmt_filter_speckles(dcmt_ctx* ctx, const int16_t* disp16, size_t drs, int16_t* out, size_t ors, float* depth, size_t zrs, int rows, int cols,
                         const dcmt_speckle_params* params, uint32_t* removed)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !disp16 || !out || !params || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const size_t row = sizeof(int16_t) * (size_t)cols;
    Plane in(disp16, drs, row, rows), o(out, ors, row, rows), z(depth, zrs, sizeof(float) * (size_t)cols, rows), n(removed, sizeof(uint32_t));
    int rc = stage(ctx, {&in, &z}, {&o, &n});
    if (rc == DCMT_OK)
        rc = dcmt_filter_speckles_dev(ctx, (const int16_t*)in.dev, (int16_t*)o.dev, (float*)z.dev, rows, cols, 1, params, (uint32_t*)n.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&o, &z, &n}) : rc;
}

int dcmt_evaluate(dcmt_ctx* ctx, const float* gt, size_t grs, const float* pred, size_t prs, int rows, int cols, float thresh, int mode,
                  dcmt_eval_frame* out)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !gt || !pred || !out || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const size_t frow = sizeof(float) * (size_t)cols;
    Plane g(gt, grs, frow, rows), p(pred, prs, frow, rows), sums(out, sizeof *out);
    int rc = stage(ctx, {&g, &p}, {&sums});
    if (rc == DCMT_OK) rc = dcmt_evaluate_dev(ctx, (const float*)g.dev, (const float*)p.dev, rows, cols, 1, thresh, mode, (dcmt_eval_frame*)sums.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&sums}) : rc;
}

int dcmt_colorize(dcmt_ctx* ctx, const float* src, size_t srs, int rows, int cols, uint8_t* bgr, size_t ors)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !src || !bgr || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    Plane in(src, srs, sizeof(float) * (size_t)cols, rows), out(bgr, ors, 3 * (size_t)cols, rows);
    int rc = stage(ctx, {&in}, {&out});
    if (rc == DCMT_OK) rc = dcmt_colorize_dev(ctx, (const float*)in.dev, rows, cols, 1, (uint8_t*)out.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&out}) : rc;
}

int dcmt_depth_to_cloud(dcmt_ctx* ctx, const float* depth, size_t drs, const uint8_t* bgr, size_t brs, int rows, int cols,
                        const dcmt_cloud_params* params, dcmt_cloud_point* points, int64_t capacity, int64_t* n_points)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !depth || !points || !n_points || !params || capacity < 0 || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const int64_t room = std::min<int64_t>(capacity, (int64_t)rows * cols);         // a frame never has more records than pixels
    int32_t offsets[2] = {0, 0};
    Plane d(depth, drs, sizeof(float) * (size_t)cols, rows), c(bgr, brs, 3 * (size_t)cols, rows);
    Plane pts(points, sizeof(dcmt_cloud_point) * (size_t)room), off(offsets, sizeof offsets);
    int rc = stage(ctx, {&d, &c}, {&pts, &off});
    if (rc == DCMT_OK)
        rc = dcmt_depth_to_cloud_dev(ctx, (const float*)d.dev, (const uint8_t*)c.dev, rows, cols, 1, params, (dcmt_cloud_point*)pts.dev, room,
                                     (int32_t*)off.dev, ctx->own_stream);
    if (rc == DCMT_OK) rc = fetch(ctx, {&off});          // the count first; then only the records there are, or there is room for
    if (rc != DCMT_OK) return rc;
    const int64_t have = std::min<int64_t>(offsets[1], room);
    if (have > 0) DCMT_HIP(ctx, hipMemcpy(points, pts.dev, sizeof(dcmt_cloud_point) * (size_t)have, hipMemcpyDeviceToHost));
    *n_points = offsets[1];
    return DCMT_OK;
}

int dcmt_gaussian5(dcmt_ctx* ctx, const float* src, size_t srs, float* dst, size_t drs, int rows, int cols)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !src || !dst || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const size_t frow = sizeof(float) * (size_t)cols;
    Plane in(src, srs, frow, rows), out(dst, drs, frow, rows);
    int rc = stage(ctx, {&in}, {&out});
    if (rc == DCMT_OK) rc = dcmt_gaussian5_dev(ctx, (const float*)in.dev, (float*)out.dev, rows, cols, 1, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&out}) : rc;
}

int dcmt_gaussian5_valid(dcmt_ctx* ctx, const float* src, size_t srs, float* dst, size_t drs, int rows, int cols, float valid_thresh)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !src || !dst || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const size_t frow = sizeof(float) * (size_t)cols;
    Plane in(src, srs, frow, rows), out(dst, drs, frow, rows);
    int rc = stage(ctx, {&in}, {&out});
    if (rc == DCMT_OK) rc = dcmt_gaussian5_valid_dev(ctx, (const float*)in.dev, (float*)out.dev, rows, cols, 1, valid_thresh, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&out}) : rc;
}

int dcmt_bilateral5(dcmt_ctx* ctx, const float* src, size_t srs, float* dst, size_t drs, int rows, int cols, float sigma_color, float sigma_space)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !src || !dst || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const size_t frow = sizeof(float) * (size_t)cols;
    Plane in(src, srs, frow, rows), out(dst, drs, frow, rows);
    int rc = stage(ctx, {&in}, {&out});
    if (rc == DCMT_OK) rc = dcmt_bilateral5_dev(ctx, (const float*)in.dev, (float*)out.dev, rows, cols, 1, sigma_color, sigma_space, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&out}) : rc;
}

int dcmt_slic_connectivity(dcmt_ctx* ctx, const int32_t* labels, size_t lrs, int rows, int cols, int n_centers, int32_t* out, size_t ors,
                           int32_t* count)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !labels || !out || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const size_t row = sizeof(int32_t) * (size_t)cols;
    Plane in(labels, lrs, row, rows), o(out, ors, row, rows), n(count, sizeof(int32_t));
    int rc = stage(ctx, {&in}, {&o, &n});
    if (rc == DCMT_OK) rc = dcmt_slic_connectivity_dev(ctx, (const int32_t*)in.dev, rows, cols, 1, n_centers, (int32_t*)o.dev, (int32_t*)n.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&o, &n}) : rc;
}

int dcmt_slic_contours(dcmt_ctx* ctx, const int32_t* labels, size_t lrs, int rows, int cols, uint8_t* bgr, size_t brs, const uint8_t colour_bgr[3],
                       uint8_t* mask, size_t mrs)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !labels || (!bgr && !mask) || !colour_bgr || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    Plane in(labels, lrs, sizeof(int32_t) * (size_t)cols, rows), img(bgr, brs, 3 * (size_t)cols, rows), m(mask, mrs, (size_t)cols, rows);
    int rc = stage(ctx, {&in, &img}, {&m});
    if (rc == DCMT_OK) rc = dcmt_slic_contours_dev(ctx, (const int32_t*)in.dev, rows, cols, 1, (uint8_t*)img.dev, colour_bgr, (uint8_t*)m.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&img, &m}) : rc;
}

int dcmt_slic_cluster_means(dcmt_ctx* ctx, const int32_t* labels, size_t lrs, int rows, int cols, int n_labels, uint8_t* bgr, size_t brs,
                            int32_t* sums)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !labels || !bgr || n_labels < 1 || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    if ((size_t)n_labels > sizeof(float) * ctx->frame_elems * (size_t)ctx->max_batch / 16) return DCMT_E_INVALID;   // the *_dev call's bound, before anything is staged
    Plane in(labels, lrs, sizeof(int32_t) * (size_t)cols, rows), img(bgr, brs, 3 * (size_t)cols, rows), s(sums, sizeof(int32_t) * 4 * (size_t)n_labels);
    int rc = stage(ctx, {&in, &img}, {&s});
    if (rc == DCMT_OK) rc = dcmt_slic_cluster_means_dev(ctx, (const int32_t*)in.dev, rows, cols, 1, n_labels, (uint8_t*)img.dev, (int32_t*)s.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&img, &s}) : rc;
}

int dcmt_superpixel_planes(dcmt_ctx* ctx, const float* depth, size_t drs, const int32_t* labels, size_t lrs, int rows, int cols, int n_labels,
                           const dcmt_planes_params* params, float* out, size_t ors, dcmt_plane_fit* fits)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !depth || !labels || !out || !params || n_labels < 1 || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    if (n_labels > dcmt_superpixel_planes_max_labels(ctx->max_rows, ctx->max_cols, ctx->max_batch, 1)) return DCMT_E_INVALID;   // the *_dev call's bound, before anything is staged
    const size_t rb = sizeof(float) * (size_t)cols;
    Plane z(depth, drs, rb, rows), l(labels, lrs, rb, rows), o(out, ors, rb, rows), f(fits, sizeof(dcmt_plane_fit) * (size_t)n_labels);
    int rc = stage(ctx, {&z, &l}, {&o, &f});
    if (rc == DCMT_OK) rc = dcmt_superpixel_planes_dev(ctx, (const float*)z.dev, (const int32_t*)l.dev, rows, cols, 1, n_labels, params, (float*)o.dev, (dcmt_plane_fit*)f.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&o, &f}) : rc;
}

int dcmt_sparse_occlusion(dcmt_ctx* ctx, const float* sparse, size_t srs, float* out, size_t ors, int rows, int cols, const dcmt_occlusion_params* params,
                          uint32_t* removed)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !sparse || !out || !params || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const size_t rb = sizeof(float) * (size_t)cols;
    Plane z(sparse, srs, rb, rows), o(out, ors, rb, rows), n(removed, sizeof(uint32_t));
    int rc = stage(ctx, {&z}, {&o, &n});
    if (rc == DCMT_OK) rc = dcmt_sparse_occlusion_dev(ctx, (const float*)z.dev, (float*)o.dev, rows, cols, 1, params, (uint32_t*)n.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&o, &n}) : rc;
}

int dcmt_support_distance(dcmt_ctx* ctx, const float* sparse, size_t srs, const float* dense, size_t drs, const float* fallback, size_t frs, float* out, size_t ors,
                          uint16_t* dist2, size_t d2rs, int rows, int cols, const dcmt_support_params* params, uint32_t* beyond)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !sparse || !params || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    if ((!out && !dist2) || (out && !dense) || (fallback && !out)) return DCMT_E_INVALID;
    const size_t rb = sizeof(float) * (size_t)cols;
    Plane z(sparse, srs, rb, rows), d(out ? dense : nullptr, drs, rb, rows), f(fallback, frs, rb, rows), o(out, ors, rb, rows);
    Plane q(dist2, d2rs, sizeof(uint16_t) * (size_t)cols, rows), n(beyond, sizeof(uint32_t));
    int rc = stage(ctx, {&z, &d, &f}, {&o, &q, &n});
    if (rc == DCMT_OK)
        rc = dcmt_support_distance_dev(ctx, (const float*)z.dev, (const float*)d.dev, (const float*)f.dev, (float*)o.dev, (uint16_t*)q.dev, rows, cols, 1, params,
                                       (uint32_t*)n.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&o, &q, &n}) : rc;
}

// the tables go up as one more input plane
int dcmt_joint_bilateral(dcmt_ctx* ctx, const float* depth, size_t drs, const uint8_t* guide, size_t grs, int channels, const dcmt_joint_tables* tables,
                         float* out, size_t ors, int rows, int cols, const dcmt_joint_params* params, uint32_t* counts)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !depth || !guide || !tables || !out || !params || !dims_ok(ctx, rows, cols, 1) || (channels != 1 && channels != 3)) return DCMT_E_INVALID;
    const size_t rb = sizeof(float) * (size_t)cols;
    Plane z(depth, drs, rb, rows), g(guide, grs, (size_t)channels * (size_t)cols, rows), t(tables, sizeof *tables), o(out, ors, rb, rows),
        n(counts, 2 * sizeof(uint32_t));
    int rc = stage(ctx, {&z, &g, &t}, {&o, &n});
    if (rc == DCMT_OK)
        rc = dcmt_joint_bilateral_dev(ctx, (const float*)z.dev, (const uint8_t*)g.dev, channels, (const dcmt_joint_tables*)t.dev, (float*)o.dev, rows, cols, 1,
                                      params, (uint32_t*)n.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&o, &n}) : rc;
}

int dcmt_depth_normals(dcmt_ctx* ctx, const float* depth, size_t drs, int rows, int cols, const dcmt_cloud_params* cloud, const dcmt_normals_params* params,
                       dcmt_normal* normals, size_t nrs, float* out, size_t ors, uint32_t* counts)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !depth || !cloud || !params || (!normals && !out) || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const size_t rb = sizeof(float) * (size_t)cols;
    Plane z(depth, drs, rb, rows), q(normals, nrs, sizeof(dcmt_normal) * (size_t)cols, rows), o(out, ors, rb, rows), n(counts, 2 * sizeof(uint32_t));
    int rc = stage(ctx, {&z}, {&q, &o, &n});
    if (rc == DCMT_OK)
        rc = dcmt_depth_normals_dev(ctx, (const float*)z.dev, rows, cols, 1, cloud, params, (dcmt_normal*)q.dev, (float*)o.dev, (uint32_t*)n.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&q, &o, &n}) : rc;
}

// dcmt_reproject_depth and dcmt_reproject_depth_nearest, likewise
static int reproject_depth_host(decltype(&dcmt_reproject_depth_dev) dev_call, dcmt_ctx* ctx, const float* depth, size_t drs, int rows, int cols,
                                const dcmt_reproject_params* params, float* out, size_t ors, int out_rows, int out_cols)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !depth || !out || !params || !dims_ok(ctx, rows, cols, 1) || !dims_ok(ctx, out_rows, out_cols, 1)) return DCMT_E_INVALID;
    Plane in(depth, drs, sizeof(float) * (size_t)cols, rows), warped(out, ors, sizeof(float) * (size_t)out_cols, out_rows);
    int rc = stage(ctx, {&in}, {&warped});
    if (rc == DCMT_OK)
        rc = dev_call(ctx, (const float*)in.dev, rows, cols, 1, params, (float*)warped.dev, out_rows, out_cols, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&warped}) : rc;
}

int dcmt_reproject_depth(dcmt_ctx* ctx, const float* depth, size_t drs, int rows, int cols, const dcmt_reproject_params* params,
                         float* out, size_t ors, int out_rows, int out_cols)
{
    return reproject_depth_host(dcmt_reproject_depth_dev, ctx, depth, drs, rows, cols, params, out, ors, out_rows, out_cols);
}

int dcmt_reproject_depth_nearest(dcmt_ctx* ctx, const float* depth, size_t drs, int rows, int cols, const dcmt_reproject_params* params,
                                 float* out, size_t ors, int out_rows, int out_cols)
{
    return reproject_depth_host(dcmt_reproject_depth_nearest_dev, ctx, depth, drs, rows, cols, params, out, ors, out_rows, out_cols);
}

int dcmt_bgr_convert(dcmt_ctx* ctx, const uint8_t* bgr, size_t brs, int rows, int cols, uint8_t* lab, size_t lrs, uint8_t* gray, size_t grs)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !bgr || (!lab && !gray) || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    Plane in(bgr, brs, 3 * (size_t)cols, rows), l(lab, lrs, 3 * (size_t)cols, rows), g(gray, grs, cols, rows);
    int rc = stage(ctx, {&in}, {&l, &g});
    if (rc == DCMT_OK) rc = dcmt_bgr_convert_dev(ctx, (const uint8_t*)in.dev, rows, cols, 1, (uint8_t*)l.dev, (uint8_t*)g.dev, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&l, &g}) : rc;
}

// the record goes up as a table of one, and its map is a plane of the call that is never fetched (its host pointer only marks it
// as wanted)
int dcmt_rectify(dcmt_ctx* ctx, const uint8_t* src, size_t srs, int src_rows, int src_cols, int channels, const dcmt_rectify_calib* calib,
                 uint8_t* dst, size_t drs, int rows, int cols)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !src || !calib || !dst || !dims_ok(ctx, rows, cols, 1) || (channels != 1 && channels != 3)) return DCMT_E_INVALID;
    if (src_rows < 1 || src_cols < 1 || src_rows > 16384 || src_cols > 16384) return DCMT_E_INVALID;
    const size_t ch = (size_t)channels;
    Plane in(src, srs, ch * (size_t)src_cols, src_rows), table(calib, sizeof *calib), map(dst, 8 * (size_t)rows * (size_t)cols),
        out(dst, drs, ch * (size_t)cols, rows);
    int rc = stage(ctx, {&in, &table}, {&map, &out});
    if (rc == DCMT_OK) rc = dcmt_rectify_map_dev(ctx, (const dcmt_rectify_calib*)table.dev, 1, rows, cols, (int32_t*)map.dev, ctx->own_stream);
    if (rc == DCMT_OK)
        rc = dcmt_rectify_dev(ctx, (const uint8_t*)in.dev, src_rows, src_cols, channels, (const int32_t*)map.dev, 1, nullptr, 0, (uint8_t*)out.dev, rows,
                              cols, 1, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&out}) : rc;
}

int dcmt_depth_to_u16(dcmt_ctx* ctx, const float* depth, size_t drs, float scale, uint16_t* out, size_t ors, int rows, int cols)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !depth || !out || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    Plane in(depth, drs, sizeof(float) * (size_t)cols, rows), o(out, ors, sizeof(uint16_t) * (size_t)cols, rows);
    int rc = stage(ctx, {&in}, {&o});
    if (rc == DCMT_OK) rc = dcmt_depth_to_u16_dev(ctx, (const float*)in.dev, scale, (uint16_t*)o.dev, rows, cols, 1, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&o}) : rc;
}

}  // extern "C"
