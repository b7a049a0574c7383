// Exercises the path count of the stereo matcher through include/img_completion.h: dcmt_shim::stereo_sgm_paths on cv::Mats (the left
// image with padded rows) with 8 paths against dcmt_sgm_paths on the same planes, byte for byte, and with 4 paths against
// dcmt_shim::stereo_sgm.  Path counts and penalties the call refuses must throw.  Writes the eight-path map the shim returned.
// Returns 0 when everything agreed.
//   shim_sgm_paths_test <rows> <cols> <num_disparities> <left.u8> <right.u8> <disp16.i16>
#include "img_completion.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

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

static bool same_rows(const cv::Mat& m, const int16_t* want, int rows, int cols)
{
    for (int i = 0; i < rows; ++i)
        if (std::memcmp(m.ptr<int16_t>(i), want + (size_t)cols * i, 2 * (size_t)cols) != 0) return false;
    return true;
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
    p.num_disparities = disparities;
    cv::Mat eight, four, plain, by_default;
    dcmt_shim::stereo_sgm_paths(l, r, eight, 8, &p);
    dcmt_shim::stereo_sgm_paths(l, r, four, 4, &p);
    dcmt_shim::stereo_sgm(l, r, plain, &p);
    dcmt_shim::stereo_sgm_paths(l, r, by_default, 8);        // the default parameters
    for (const cv::Mat* m : {&eight, &four, &plain, &by_default})
        if (m->type() != CV_16SC1 || m->rows != rows || m->cols != cols) return 5;

    // the C ABI on the same planes
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 6;
    std::vector<int16_t> want8(px, 9), want4(px, 9), want_default(px, 9);
    if (dcmt_sgm_paths(ctx, left.data(), cols, right.data(), cols, rows, cols, &p, want8.data(), 2 * (size_t)cols, nullptr, 0, 8) != DCMT_OK) return 7;
    if (dcmt_sgm(ctx, left.data(), cols, right.data(), cols, rows, cols, &p, want4.data(), 2 * (size_t)cols, nullptr, 0) != DCMT_OK) return 7;
    p.num_disparities = 64;
    if (dcmt_sgm_paths(ctx, left.data(), cols, right.data(), cols, rows, cols, &p, want_default.data(), 2 * (size_t)cols, nullptr, 0, 8) != DCMT_OK) return 7;
    // refused by the C call: nothing written
    std::vector<int16_t> untouched(px, 9);
    if (dcmt_sgm_paths(ctx, left.data(), cols, right.data(), cols, rows, cols, &p, untouched.data(), 2 * (size_t)cols, nullptr, 0, 5) != DCMT_E_INVALID) return 8;
    for (size_t i = 0; i < px; ++i)
        if (untouched[i] != 9) return 8;
    dcmt_destroy(ctx);
    if (!same_rows(eight, want8.data(), rows, cols)) return 9;
    if (!same_rows(four, want4.data(), rows, cols) || !same_rows(plain, want4.data(), rows, cols)) return 10;
    if (!same_rows(by_default, want_default.data(), rows, cols)) return 11;
    if (std::memcmp(want8.data(), want4.data(), 2 * px) == 0) return 12;      // the diagonals change something on this pair
    for (int i = 0; i < rows; ++i)
        for (size_t k = cols; k < step; ++k)
            if (padded[step * i + k] != 0xEE) return 13;      // the padding is not the image's

    // path counts other than 4 and 8, p2 beyond the eight-path limit (fine with four), images the shim refuses: thrown
    int thrown = 0;
    cv::Mat sink;
    for (int paths : {0, 5, 16, -8})
        try { dcmt_shim::stereo_sgm_paths(l, r, sink, paths); } catch (const std::runtime_error&) { ++thrown; }
    p.p2 = 1801;
    try { dcmt_shim::stereo_sgm_paths(l, r, sink, 8, &p); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat c(rows, cols, CV_8UC3); dcmt_shim::stereo_sgm_paths(c, r, sink, 8); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat s(rows, cols + 1, CV_8UC1); dcmt_shim::stereo_sgm_paths(l, s, sink, 8); } catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 7) return 14;
    dcmt_shim::stereo_sgm_paths(l, r, sink, 4, &p);           // p2 = 1801 with four paths: taken
    if (sink.type() != CV_16SC1 || sink.rows != rows) return 15;

    std::vector<int16_t> got(px);
    for (int i = 0; i < rows; ++i) std::memcpy(got.data() + (size_t)cols * i, eight.ptr<int16_t>(i), 2 * (size_t)cols);
    if (!write_all(argv[6], got.data(), 2 * px)) return 16;
    std::printf("ok\n");
    return 0;
}
