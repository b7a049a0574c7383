// Exercises the cascade without its extrapolation through include/img_completion.h: dcmt_shim::img_completion_no_extrapolate and
// dcmt_shim::interpolate_with_labels_no_extrapolate against dcmt_complete_f32 / dcmt_complete_labeled_f32 with
// DCMT_FLAG_NO_EXTRAPOLATE, bit for bit, on a raw f32 frame written by the pytest driver into a cv::Mat with padded rows.  The
// reference-named img_completion must keep ignoring `extr`.  Prints what the shim prints (the two header lines, once: the labeled
// twin prints nothing).  Writes both shim results as raw f32.  Returns 0 when everything agreed.
//   shim_no_extrapolate_test <rows> <cols> <in.f32> <out_plain.f32> <out_labeled.f32>
#include "img_completion.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

static bool read_all(const char* path, void* dst, size_t bytes)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = std::fread(dst, 1, bytes, f);
    std::fclose(f);
    return got == bytes;
}

static bool write_rows(const char* path, const cv::Mat& m)
{
    FILE* o = std::fopen(path, "wb");
    if (!o) return false;
    bool ok = true;
    for (int r = 0; r < m.rows; ++r) ok = ok && std::fwrite(m.ptr<float>(r), sizeof(float), (size_t)m.cols, o) == (size_t)m.cols;
    std::fclose(o);
    return ok;
}

static bool same_bits(const cv::Mat& m, const std::vector<float>& packed)
{
    for (int r = 0; r < m.rows; ++r)
        if (std::memcmp(m.ptr<float>(r), &packed[(size_t)r * m.cols], sizeof(float) * (size_t)m.cols) != 0) return false;
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]);
    const size_t pad = 8, px = (size_t)rows * cols;                           // ROI-like strided input
    const size_t step = (size_t)(cols + pad) * sizeof(float);
    std::vector<float> packed(px), storage((size_t)rows * (cols + pad), -7.0f);
    if (!read_all(argv[3], packed.data(), px * sizeof(float))) return 3;
    for (int r = 0; r < rows; ++r) std::memcpy(&storage[(size_t)r * (cols + pad)], &packed[(size_t)r * cols], (size_t)cols * 4);
    const cv::Mat sparse(rows, cols, CV_32FC1, storage.data(), step);
    if (DCMT_FLAG_NO_EXTRAPOLATE != 8 || DCMT_VERSION != 120) return 4;

    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 6;
    const size_t row = sizeof(float) * (size_t)cols;
    dcmt_params p;
    dcmt_default_params(&p);
    p.flags |= DCMT_FLAG_NO_EXTRAPOLATE;

    // the plain form, printing as the reference does: two header lines, no hole counts
    cv::Mat dense;
    dcmt_shim::img_completion_no_extrapolate(sparse, dense, "gaussian");
    std::fflush(stdout);
    if (dense.rows != rows || dense.cols != cols || dense.type() != CV_32FC1) return 5;
    dcmt_shim::quiet() = true;
    std::vector<float> want(px, -1.0f);
    if (dcmt_complete_f32(ctx, packed.data(), row, 0, want.data(), row, 0, rows, cols, 1, &p) != DCMT_OK) return 7;
    if (!same_bits(dense, want)) return 8;
    if (std::strstr(dcmt_last_path(ctx), "k_local") == nullptr) return 9;
    int probe[1] = {-1};
    if (dcmt_last_fill_iters(ctx, probe, 1) != DCMT_OK || probe[0] != 0) return 10;
    probe[0] = -1;
    if (dcmt_last_holes_after_extend(ctx, probe, 1) != DCMT_OK || probe[0] != 0) return 10;
    // holes stay: the plane differs from the reference-named call's, which ignores extr whatever it is
    cv::Mat with_true, with_false;
    img_completion(sparse, with_true, true, "gaussian");
    img_completion(sparse, with_false, false, "gaussian");
    std::vector<float> def(px, -1.0f);
    dcmt_params q;
    dcmt_default_params(&q);
    if (dcmt_complete_f32(ctx, packed.data(), row, 0, def.data(), row, 0, rows, cols, 1, &q) != DCMT_OK) return 11;
    if (!same_bits(with_true, def) || !same_bits(with_false, def)) return 12;
    if (same_bits(dense, def)) return 13;
    // the other blurs, and the refusals
    for (const char* blur : {"none", "bilateral_clone"}) {
        cv::Mat d;
        dcmt_shim::img_completion_no_extrapolate(sparse, d, blur);
        p.blur = dcmt_shim::blur_from_string(blur);
        if (dcmt_complete_f32(ctx, packed.data(), row, 0, want.data(), row, 0, rows, cols, 1, &p) != DCMT_OK) return 14;
        if (!same_bits(d, want)) return 15;
    }
    bool thrown = false;
    try { cv::Mat t; dcmt_shim::img_completion_no_extrapolate(sparse, t, "bilateral"); } catch (const std::runtime_error&) { thrown = true; }
    if (!thrown) return 16;
    p.blur = DCMT_BLUR_GAUSSIAN;
    for (int stop = DCMT_STAGE_EXTEND; stop <= DCMT_STAGE_FILLLOOP; ++stop) {
        p.stop_after = stop;
        if (dcmt_complete_f32(ctx, packed.data(), row, 0, want.data(), row, 0, rows, cols, 1, &p) != DCMT_E_UNSUPPORTED) return 17;
    }
    p.stop_after = DCMT_STAGE_FINAL;

    // the labeled twin: clusters[col][row] as Slic::clusters, a grid of 9 x 9 cells
    const int cell = 9, gx = (cols + cell - 1) / cell, n_labels = gx * ((rows + cell - 1) / cell);
    std::vector<std::vector<int> > clusters((size_t)cols, std::vector<int>((size_t)rows));
    std::vector<int32_t> lab(px);
    for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) { clusters[j][i] = (i / cell) * gx + j / cell; lab[(size_t)i * cols + j] = clusters[j][i]; }
    dcmt_shim::quiet() = false;                                               // verbose = 2 prints nothing without the loop
    cv::Mat dense_l;
    dcmt_shim::interpolate_with_labels_no_extrapolate(clusters, n_labels, sparse, dense_l, "gaussian", 1);
    std::fflush(stdout);
    dcmt_shim::quiet() = true;
    if (dcmt_complete_labeled_f32(ctx, packed.data(), row, 0, lab.data(), sizeof(int32_t) * (size_t)cols, 0, n_labels, want.data(), row, 0,
                                  rows, cols, 1, &p, 1) != DCMT_OK) return 18;
    if (!same_bits(dense_l, want)) return 19;
    if (std::strstr(dcmt_last_path(ctx), "k_local<START4>") == nullptr) return 20;
    cv::Mat dense_l0;
    dcmt_shim::interpolate_with_labels_no_extrapolate(clusters, n_labels, sparse, dense_l0, "gaussian", 0);
    if (!same_bits(dense_l0, std::vector<float>(dense.ptr<float>(0), dense.ptr<float>(0) + px))) return 21;    // use_superpixel = 0: the plain form

    if (!write_rows(argv[4], dense) || !write_rows(argv[5], dense_l)) return 22;
    dcmt_destroy(ctx);
    return 0;
}
