// Exercises the bilateral finish through include/img_completion.h: img_completion(cv::Mat, ..., "bilateral_clone") against
// dcmt_complete_f32 with DCMT_BLUR_BILATERAL_CLONE, and dcmt_shim::bilateral_filter5 against dcmt_bilateral5, bit for bit, on a raw
// f32 frame written by the pytest driver into a cv::Mat with padded rows.  "bilateral" must still throw.  Writes both shim results as
// raw f32.  Returns 0 when everything agreed.
//   shim_bilateral_test <rows> <cols> <in.f32> <out_complete.f32> <out_filter.f32>
#include "img_completion.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

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
    dcmt_shim::quiet() = true;

    // the cascade: the string maps to the new value, and the shim's call is the C ABI's
    if (dcmt_shim::blur_from_string("bilateral_clone") != DCMT_BLUR_BILATERAL_CLONE || DCMT_BLUR_BILATERAL_CLONE != 3) return 4;
    if (dcmt_shim::blur_from_string("bilateral") != DCMT_BLUR_BILATERAL || dcmt_shim::blur_from_string("gaussian") != DCMT_BLUR_GAUSSIAN) return 4;
    cv::Mat dense;
    img_completion(sparse, dense, false, "bilateral_clone");
    if (dense.rows != rows || dense.cols != cols || dense.type() != CV_32FC1) return 5;
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 6;
    dcmt_params p;
    dcmt_default_params(&p);
    p.blur = DCMT_BLUR_BILATERAL_CLONE;
    std::vector<float> want(px, -1.0f);
    const size_t row = sizeof(float) * (size_t)cols;
    if (dcmt_complete_f32(ctx, packed.data(), row, 0, want.data(), row, 0, rows, cols, 1, &p) != DCMT_OK) return 7;
    if (!same_bits(dense, want)) return 8;
    if (std::strstr(dcmt_last_path(ctx), "bilateral5") == nullptr) return 9;

    // the reference's own string still throws
    bool thrown = false;
    try { cv::Mat t; img_completion(sparse, t, false, "bilateral"); } catch (const std::runtime_error&) { thrown = true; }
    if (!thrown) return 10;

    // the filter on its own, on the completed plane (as the stereo-lidar main blurs its refined depth); src and dst the same Mat
    cv::Mat filtered;
    dcmt_shim::bilateral_filter5(dense, filtered);
    if (filtered.rows != rows || filtered.cols != cols || filtered.type() != CV_32FC1) return 11;
    std::vector<float> fwant(px, -1.0f);
    if (dcmt_bilateral5(ctx, want.data(), row, fwant.data(), row, rows, cols, 1.5f, 2.0f) != DCMT_OK) return 12;
    if (!same_bits(filtered, fwant)) return 13;
    cv::Mat again = dense;
    dcmt_shim::bilateral_filter5(again, again, 1.5f, 2.0f);
    if (!same_bits(again, fwant)) return 14;
    bool refused = false;
    try { cv::Mat t; dcmt_shim::bilateral_filter5(dense, t, 0.0f, 2.0f); } catch (const std::runtime_error&) { refused = true; }
    if (!refused) return 15;
    dcmt_destroy(ctx);
    if (!write_rows(argv[4], dense) || !write_rows(argv[5], filtered)) return 16;
    return 0;
}
