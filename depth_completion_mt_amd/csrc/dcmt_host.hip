// dcmt_host.hip -- the synchronous single-frame host variants of the *_dev entry points: stage the caller's planes in temporary
// device buffers, run the public *_dev function with batch = 1 on the context's own stream, fetch the results, synchronise.
// Nothing but dcmt.h's ABI is called here and no kernel is compiled: this translation unit emits no device code.
#include <algorithm>
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

// Checks the pitches, gets the context's own stream (created on first use), allocates every plane and only then enqueues the
// uploads of `ins`: an allocation that fails leaves nothing of the call in the stream.
int stage(dcmt_ctx* ctx, Planes ins, Planes outs)
{
    for (Planes l : {ins, outs})
        for (Plane* p : l) if (p->host && p->pitch < p->row_bytes) return DCMT_E_INVALID;
    if (!ctx->own_stream) DCMT_HIP(ctx, hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    for (Planes l : {ins, outs})
        for (Plane* p : l) if (p->host) DCMT_HIP(ctx, hipMalloc(&p->dev, std::max<size_t>(p->row_bytes * p->rows, 1)));
    for (Plane* p : ins) {
        if (!p->host || !p->row_bytes) continue;
        if (p->rows == 1) DCMT_HIP(ctx, hipMemcpyAsync(p->dev, p->host, p->row_bytes, hipMemcpyHostToDevice, ctx->own_stream));
        else DCMT_HIP(ctx, hipMemcpy2DAsync(p->dev, p->row_bytes, p->host, p->pitch, p->row_bytes, p->rows, hipMemcpyHostToDevice, ctx->own_stream));
    }
    return DCMT_OK;
}

// Copies `outs` back behind whatever the call enqueued and waits for it all.
int fetch(dcmt_ctx* ctx, Planes outs)
{
    for (Plane* p : outs) {
        if (!p->host || !p->row_bytes) continue;
        if (p->rows == 1) DCMT_HIP(ctx, hipMemcpyAsync(p->host, p->dev, p->row_bytes, hipMemcpyDeviceToHost, ctx->own_stream));
        else DCMT_HIP(ctx, hipMemcpy2DAsync(p->host, p->pitch, p->dev, p->row_bytes, p->row_bytes, p->rows, hipMemcpyDeviceToHost, ctx->own_stream));
    }
    DCMT_HIP(ctx, hipStreamSynchronize(ctx->own_stream));
    return DCMT_OK;
}

}  // namespace

// Every variant: its own null checks and the frame against the context's maxima (before anything is allocated), stage, the
// *_dev call -- which reports what only it can detect (a NaN matrix, step < 6) --, fetch.
extern "C" {

int dcmt_project_points(dcmt_ctx* ctx, const float* points, int n_points, const float T[16], const float P[12],
                        float* sparse, size_t srs, int rows, int cols)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !sparse || !T || !P || n_points < 0 || (n_points > 0 && !points) || !dims_ok(ctx, rows, cols, 1)) return DCMT_E_INVALID;
    const int32_t offsets[2] = {0, n_points};
    Plane pts(points, sizeof(float) * 4 * (size_t)n_points), off(offsets, sizeof offsets), out(sparse, srs, sizeof(float) * (size_t)cols, rows);
    int rc = stage(ctx, {&pts, &off}, {&out});
    if (rc == DCMT_OK)
        rc = dcmt_project_points_dev(ctx, (const float*)pts.dev, (const int32_t*)off.dev, n_points, 1, T, P, (float*)out.dev, rows, cols, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&out}) : rc;
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

int dcmt_reproject_depth(dcmt_ctx* ctx, const float* depth, size_t drs, int rows, int cols, const dcmt_reproject_params* params,
                         float* out, size_t ors, int out_rows, int out_cols)
{
    DCMT_ON_DEVICE(ctx);
    if (!ctx || !depth || !out || !params || !dims_ok(ctx, rows, cols, 1) || !dims_ok(ctx, out_rows, out_cols, 1)) return DCMT_E_INVALID;
    Plane in(depth, drs, sizeof(float) * (size_t)cols, rows), warped(out, ors, sizeof(float) * (size_t)out_cols, out_rows);
    int rc = stage(ctx, {&in}, {&warped});
    if (rc == DCMT_OK)
        rc = dcmt_reproject_depth_dev(ctx, (const float*)in.dev, rows, cols, 1, params, (float*)warped.dev, out_rows, out_cols, ctx->own_stream);
    return rc == DCMT_OK ? fetch(ctx, {&warped}) : rc;
}

}  // extern "C"
