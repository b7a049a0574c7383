// Exercises the Gaussian that ignores holes through include/img_completion.h: img_completion_no_extrapolate(cv::Mat, ..., "gaussian_valid")
// and img_completion(cv::Mat, ..., "gaussian_valid") against dcmt_complete_f32 with DCMT_BLUR_GAUSSIAN_VALID, and
// dcmt_shim::gaussian_blur5_valid against dcmt_gaussian5_valid, bit for bit, on a raw f32 frame written by the pytest driver into a
// cv::Mat with padded rows.  Writes the three shim results as raw f32.  Returns 0 when everything agreed.
//   shim_gauss_valid_test <rows> <cols> <in.f32> <out_noext.f32> <out_complete.f32> <out_filter.f32>
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
    if (argc < 7) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]);
    const size_t pad = 8, px = (size_t)rows * cols;                           // ROI-like strided input
    const size_t step = (size_t)(cols + pad) * sizeof(float);
    std::vector<float> packed(px), storage((size_t)rows * (cols + pad), -7.0f);
    if (!read_all(argv[3], packed.data(), px * sizeof(float))) return 3;
    for (int r = 0; r < rows; ++r) std::memcpy(&storage[(size_t)r * (cols + pad)], &packed[(size_t)r * cols], (size_t)cols * 4);
    const cv::Mat sparse(rows, cols, CV_32FC1, storage.data(), step);
    dcmt_shim::quiet() = true;

    // the string maps to the new value; the others map as they did
    if (dcmt_shim::blur_from_string("gaussian_valid") != DCMT_BLUR_GAUSSIAN_VALID || DCMT_BLUR_GAUSSIAN_VALID != 5) return 4;
    if (dcmt_shim::blur_from_string("gaussian") != DCMT_BLUR_GAUSSIAN || dcmt_shim::blur_from_string("bilateral_clone") != DCMT_BLUR_BILATERAL_CLONE ||
        dcmt_shim::blur_from_string("valid") != DCMT_BLUR_NONE)
        return 4;

    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 5;
    const size_t row = sizeof(float) * (size_t)cols;
    dcmt_params p;
    dcmt_default_params(&p);
    p.blur = DCMT_BLUR_GAUSSIAN_VALID;

    // without the extrapolation: the finish is a kind of the one kernel
    cv::Mat noext;
    dcmt_shim::img_completion_no_extrapolate(sparse, noext, "gaussian_valid");
    if (noext.rows != rows || noext.cols != cols || noext.type() != CV_32FC1) return 6;
    p.flags = DCMT_FLAG_NO_EXTRAPOLATE;
    std::vector<float> want_ne(px, -1.0f);
    if (dcmt_complete_f32(ctx, packed.data(), row, 0, want_ne.data(), row, 0, rows, cols, 1, &p) != DCMT_OK) return 7;
    if (!same_bits(noext, want_ne)) return 8;
    if (std::strstr(dcmt_last_path(ctx), "VALID") == nullptr) return 9;
    cv::Mat plain;
    dcmt_shim::img_completion_no_extrapolate(sparse, plain, "gaussian");
    if (same_bits(plain, want_ne)) return 10;                                 // the two finishes differ on a plane with holes

    // with it: the chain to the median, then the stand-alone kernel
    cv::Mat dense;
    img_completion(sparse, dense, false, "gaussian_valid");
    p.flags = 0;
    std::vector<float> want(px, -1.0f);
    if (dcmt_complete_f32(ctx, packed.data(), row, 0, want.data(), row, 0, rows, cols, 1, &p) != DCMT_OK) return 11;
    if (!same_bits(dense, want)) return 12;
    if (std::strstr(dcmt_last_path(ctx), "gauss5_valid") == nullptr) return 13;

    // the filter on its own, on the plane with holes; src and dst the same Mat; a threshold that is refused
    cv::Mat filtered;
    dcmt_shim::gaussian_blur5_valid(noext, filtered);
    if (filtered.rows != rows || filtered.cols != cols || filtered.type() != CV_32FC1) return 14;
    std::vector<float> fwant(px, -1.0f);
    if (dcmt_gaussian5_valid(ctx, want_ne.data(), row, fwant.data(), row, rows, cols, 0.1f) != DCMT_OK) return 15;
    if (!same_bits(filtered, fwant)) return 16;
    cv::Mat again = noext;
    dcmt_shim::gaussian_blur5_valid(again, again, 0.1f);
    if (!same_bits(again, fwant)) return 17;
    bool refused = false;
    try { cv::Mat t; dcmt_shim::gaussian_blur5_valid(noext, t, 0.0f); } catch (const std::runtime_error&) { refused = true; }
    if (!refused) return 18;
    dcmt_destroy(ctx);
    if (!write_rows(argv[4], noext) || !write_rows(argv[5], dense) || !write_rows(argv[6], filtered)) return 19;
    return 0;
}
