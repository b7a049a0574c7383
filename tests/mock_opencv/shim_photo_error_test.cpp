// Exercises get_initial_error through include/img_completion.h: dcmt_shim::get_initial_error on cv::Mats (the depth packed, the left image
// with padded rows) against dcmt_photo_error on the same planes, byte for byte, on raw planes written by the pytest driver.
// Arguments the call refuses must throw.  Writes the map and the four counts the shim returned.  Returns 0 when everything agreed.
//   shim_photo_error_test <rows> <cols> <window> <depth.f32> <left.u8> <right.u8> <err.u8> <stats.u64>
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
    if (argc < 9) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), window = std::atoi(argv[3]);
    const size_t px = (size_t)rows * cols;
    std::vector<float> depth(px);
    std::vector<unsigned char> left(px), right(px);
    if (!read_all(argv[4], depth.data(), 4 * px) || !read_all(argv[5], left.data(), px) || !read_all(argv[6], right.data(), px)) return 3;

    cv::Mat d(rows, cols, CV_32FC1), r(rows, cols, CV_8UC1);
    std::memcpy(d.ptr<float>(), depth.data(), 4 * px);
    std::memcpy(r.ptr<unsigned char>(), right.data(), px);
    const size_t step = (size_t)cols + 5;                    // the left image's rows are 5 bytes further apart than they need to be
    std::vector<unsigned char> padded(step * rows, 0xEE);
    cv::Mat l(rows, cols, CV_8UC1, padded.data(), step);
    for (int i = 0; i < rows; ++i) std::memcpy(l.ptr<unsigned char>(i), left.data() + (size_t)cols * i, cols);

    dcmt_photo_error_params p;
    dcmt_default_photo_error_params(&p);
    if (p.window != 2 || p.baseline != 0.54f || p.focal != 9.597910e+02f) return 4;
    p.window = window;
    uint64_t stats[4] = {7, 7, 7, 7};
    const cv::Mat map = dcmt_shim::get_initial_error(d, l, r, &p, stats);
    if (map.type() != CV_8UC1 || map.rows != rows || map.cols != cols) return 5;
    const cv::Mat by_default = dcmt_shim::get_initial_error(d, l, r);              // the reference's constants, no counts

    // the C ABI on the same planes
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 6;
    std::vector<unsigned char> want(px, 9), want_default(px, 9);
    uint64_t want_stats[4] = {0, 0, 0, 0};
    if (dcmt_photo_error(ctx, depth.data(), 4 * (size_t)cols, left.data(), cols, right.data(), cols, rows, cols, &p, want.data(), cols, want_stats) != DCMT_OK) return 7;
    p.window = 2;
    if (dcmt_photo_error(ctx, depth.data(), 4 * (size_t)cols, left.data(), cols, right.data(), cols, rows, cols, &p, want_default.data(), cols, nullptr) != DCMT_OK) return 7;
    dcmt_destroy(ctx);
    for (int i = 0; i < rows; ++i) {
        if (std::memcmp(map.ptr<unsigned char>(i), want.data() + (size_t)cols * i, cols) != 0) return 8;
        if (std::memcmp(by_default.ptr<unsigned char>(i), want_default.data() + (size_t)cols * i, cols) != 0) return 9;
    }
    for (int k = 0; k < 4; ++k) if (stats[k] != want_stats[k]) return 10;
    for (int i = 0; i < rows; ++i)
        for (size_t k = cols; k < step; ++k)
            if (padded[step * i + k] != 0xEE) return 11;      // the padding is not the image's

    // a BGR image, an image of another size, a depth that is no CV_32FC1, a window the library refuses: thrown
    int thrown = 0;
    try { cv::Mat c(rows, cols, CV_8UC3); dcmt_shim::get_initial_error(d, c, r); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat s(rows, cols + 1, CV_8UC1); dcmt_shim::get_initial_error(d, l, s); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::get_initial_error(r, l, r); } catch (const std::runtime_error&) { ++thrown; }
    try { p.window = 5; dcmt_shim::get_initial_error(d, l, r, &p); } catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 4) return 12;

    std::vector<unsigned char> got(px);
    for (int i = 0; i < rows; ++i) std::memcpy(got.data() + (size_t)cols * i, map.ptr<unsigned char>(i), cols);
    if (!write_all(argv[7], got.data(), px) || !write_all(argv[8], stats, sizeof stats)) return 13;
    std::printf("ok\n");
    return 0;
}
