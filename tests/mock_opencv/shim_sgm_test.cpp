// Exercises the stereo matcher through include/img_completion.h: dcmt_shim::stereo_sgm on cv::Mats (the left image with padded rows)
// against dcmt_sgm on the same planes, byte for byte, on raw planes written by the pytest driver.  Arguments the call refuses must
// throw.  Writes the disparity map the shim returned.  Returns 0 when everything agreed.
//   shim_sgm_test <rows> <cols> <num_disparities> <left.u8> <right.u8> <disp16.i16>
#include "img_completion.h"

#include <cstdio>
#include <cstdlib>

static bool read_all(const char* path, void* p, size_t bytes)
{
    FILE* f = std::fopen(path, "rb");
    const bool ok = f && std::fread(p, 1, bytes, f) == bytes;
    if (f) std::fclose(f);
    return ok;
}

static bool write_all(const char* path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path, "wb");
    const bool ok = f && std::fwrite(p, 1, bytes, f) == bytes;
    if (f) std::fclose(f);
    return ok;
}

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), disparities = std::atoi(argv[3]);
    const size_t px = (size_t)rows * cols;
    std::vector<unsigned char> left(px), right(px);
    if (!read_all(argv[4], left.data(), px) || !read_all(argv[5], right.data(), px)) return 3;

    cv::Mat r(rows, cols, CV_8UC1);
    std::memcpy(r.ptr<unsigned char>(), right.data(), px);
    const size_t step = (size_t)cols + 5;                    // the left image's rows are 5 bytes further apart than they need to be
    std::vector<unsigned char> padded(step * rows, 0xEE);
    cv::Mat l(rows, cols, CV_8UC1, padded.data(), step);
    for (int i = 0; i < rows; ++i) std::memcpy(l.ptr<unsigned char>(i), left.data() + (size_t)cols * i, cols);

    dcmt_sgm_params p;
    dcmt_default_sgm_params(&p);
    if (p.num_disparities != 64 || p.p1 != 200 || p.p2 != 800 || p.uniqueness != 10 || p.disp12_max_diff != 1 || p.baseline != 0.54f ||
        p.focal != 9.597910e+02f || p.max_depth != 100.0f)
        return 4;
    p.num_disparities = disparities;
    cv::Mat disp, by_default;
    dcmt_shim::stereo_sgm(l, r, disp, &p);
    if (disp.type() != CV_16SC1 || disp.rows != rows || disp.cols != cols) return 5;
    dcmt_shim::stereo_sgm(l, r, by_default);                 // the default parameters
    if (by_default.type() != CV_16SC1 || by_default.rows != rows) return 5;

    // the C ABI on the same planes
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 6;
    std::vector<int16_t> want(px, 9), want_default(px, 9);
    if (dcmt_sgm(ctx, left.data(), cols, right.data(), cols, rows, cols, &p, want.data(), 2 * (size_t)cols, nullptr, 0) != DCMT_OK) return 7;
    p.num_disparities = 64;
    if (dcmt_sgm(ctx, left.data(), cols, right.data(), cols, rows, cols, &p, want_default.data(), 2 * (size_t)cols, nullptr, 0) != DCMT_OK) return 7;
    dcmt_destroy(ctx);
    for (int i = 0; i < rows; ++i) {
        if (std::memcmp(disp.ptr<int16_t>(i), want.data() + (size_t)cols * i, 2 * (size_t)cols) != 0) return 8;
        if (std::memcmp(by_default.ptr<int16_t>(i), want_default.data() + (size_t)cols * i, 2 * (size_t)cols) != 0) return 10;
    }
    for (int i = 0; i < rows; ++i)
        for (size_t k = cols; k < step; ++k)
            if (padded[step * i + k] != 0xEE) return 11;      // the padding is not the image's

    // a BGR image, an image of another size, an f32 plane for an image, parameters the library refuses: thrown
    int thrown = 0;
    cv::Mat sink;
    try { cv::Mat c(rows, cols, CV_8UC3); dcmt_shim::stereo_sgm(c, r, sink); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat s(rows, cols + 1, CV_8UC1); dcmt_shim::stereo_sgm(l, s, sink); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat f(rows, cols, CV_32FC1); dcmt_shim::stereo_sgm(l, f, sink); } catch (const std::runtime_error&) { ++thrown; }
    try { p.num_disparities = 24; dcmt_shim::stereo_sgm(l, r, sink, &p); } catch (const std::runtime_error&) { ++thrown; }
    try { p.num_disparities = 64; p.p2 = 10001; dcmt_shim::stereo_sgm(l, r, sink, &p); } catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 5) return 12;

    std::vector<int16_t> got(px);
    for (int i = 0; i < rows; ++i) std::memcpy(got.data() + (size_t)cols * i, disp.ptr<int16_t>(i), 2 * (size_t)cols);
    if (!write_all(argv[6], got.data(), 2 * px)) return 13;
    std::printf("ok\n");
    return 0;
}
