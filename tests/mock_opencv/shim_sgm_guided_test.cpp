// Exercises the guided stereo matcher through include/img_completion.h: dcmt_shim::stereo_sgm_guided on cv::Mats (the guide with padded
// rows) against dcmt_sgm_guided on the same planes, byte for byte, with eight paths and with four; with weight 0 against
// dcmt_shim::stereo_sgm_paths.  Guides and integers the call refuses must throw.  Writes the eight-path map the shim returned.
// Returns 0 when everything agreed.
//   shim_sgm_guided_test <rows> <cols> <num_disparities> <left.u8> <right.u8> <guide.f32> <disp16.i16>
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
    if (argc < 8) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), disparities = std::atoi(argv[3]);
    const size_t px = (size_t)rows * cols;
    std::vector<unsigned char> left(px), right(px);
    std::vector<float> guide(px);
    if (!read_all(argv[4], left.data(), px) || !read_all(argv[5], right.data(), px) || !read_all(argv[6], guide.data(), 4 * px)) return 3;

    cv::Mat l(rows, cols, CV_8UC1), r(rows, cols, CV_8UC1);
    std::memcpy(l.ptr<unsigned char>(), left.data(), px);
    std::memcpy(r.ptr<unsigned char>(), right.data(), px);
    const size_t step = 4 * ((size_t)cols + 3);              // the guide's rows are 12 bytes further apart than they need to be
    std::vector<unsigned char> padded(step * rows, 0xEE);
    cv::Mat g(rows, cols, CV_32FC1, padded.data(), step);
    for (int i = 0; i < rows; ++i) std::memcpy(g.ptr<float>(i), guide.data() + (size_t)cols * i, 4 * (size_t)cols);

    dcmt_sgm_params p;
    dcmt_default_sgm_params(&p);
    p.num_disparities = disparities;
    cv::Mat eight, four, weightless, plain;
    dcmt_shim::stereo_sgm_guided(l, r, g, eight, 8, 100, 1000, &p);
    dcmt_shim::stereo_sgm_guided(l, r, g, four, 4, 100, 1000, &p);
    dcmt_shim::stereo_sgm_guided(l, r, g, weightless, 8, 0, 1000, &p);
    dcmt_shim::stereo_sgm_paths(l, r, plain, 8, &p);
    for (const cv::Mat* m : {&eight, &four, &weightless, &plain})
        if (m->type() != CV_16SC1 || m->rows != rows || m->cols != cols) return 5;

    // the C ABI on the same planes
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 6;
    std::vector<int16_t> want8(px, 9), want4(px, 9), want_plain(px, 9);
    if (dcmt_sgm_guided(ctx, left.data(), cols, right.data(), cols, guide.data(), 4 * (size_t)cols, rows, cols, &p, want8.data(), 2 * (size_t)cols, nullptr, 0,
                        8, 100, 1000) != DCMT_OK) return 7;
    if (dcmt_sgm_guided(ctx, left.data(), cols, right.data(), cols, guide.data(), 4 * (size_t)cols, rows, cols, &p, want4.data(), 2 * (size_t)cols, nullptr, 0,
                        4, 100, 1000) != DCMT_OK) return 7;
    if (dcmt_sgm_paths(ctx, left.data(), cols, right.data(), cols, rows, cols, &p, want_plain.data(), 2 * (size_t)cols, nullptr, 0, 8) != DCMT_OK) return 7;
    // refused by the C call: nothing written
    std::vector<int16_t> untouched(px, 9);
    if (dcmt_sgm_guided(ctx, left.data(), cols, right.data(), cols, guide.data(), 4 * (size_t)cols, rows, cols, &p, untouched.data(), 2 * (size_t)cols, nullptr,
                        0, 8, 100, 1001) != DCMT_E_INVALID) return 8;
    for (size_t i = 0; i < px; ++i)
        if (untouched[i] != 9) return 8;
    dcmt_destroy(ctx);
    if (!same_rows(eight, want8.data(), rows, cols)) return 9;
    if (!same_rows(four, want4.data(), rows, cols)) return 10;
    if (!same_rows(weightless, want_plain.data(), rows, cols) || !same_rows(plain, want_plain.data(), rows, cols)) return 11;
    if (std::memcmp(want8.data(), want_plain.data(), 2 * px) == 0) return 12;       // the guide changes something on this pair
    for (int i = 0; i < rows; ++i)
        for (size_t k = 4 * (size_t)cols; k < step; ++k)
            if (padded[step * i + k] != 0xEE) return 13;      // the padding is not the guide's

    // integers and sums beyond their limits, guides and images the shim refuses: thrown
    int thrown = 0;
    cv::Mat sink;
    try { dcmt_shim::stereo_sgm_guided(l, r, g, sink, 8, -1, 1000); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::stereo_sgm_guided(l, r, g, sink, 8, 10001, 1000); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::stereo_sgm_guided(l, r, g, sink, 8, 100, -1); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::stereo_sgm_guided(l, r, g, sink, 8, 100, 1001); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::stereo_sgm_guided(l, r, g, sink, 4, 100, 9201); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::stereo_sgm_guided(l, r, g, sink, 5, 100, 1000); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat c(rows, cols, CV_8UC1); dcmt_shim::stereo_sgm_guided(l, r, c, sink, 8, 100, 1000); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat s(rows, cols + 1, CV_32FC1); dcmt_shim::stereo_sgm_guided(l, r, s, sink, 8, 100, 1000); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat c(rows, cols, CV_8UC3); dcmt_shim::stereo_sgm_guided(c, r, g, sink, 8, 100, 1000); } catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 9) return 14;
    dcmt_shim::stereo_sgm_guided(l, r, g, sink, 4, 100, 9200);       // the default parameters, the four-path limit: taken
    if (sink.type() != CV_16SC1 || sink.rows != rows) return 15;

    std::vector<int16_t> got(px);
    for (int i = 0; i < rows; ++i) std::memcpy(got.data() + (size_t)cols * i, eight.ptr<int16_t>(i), 2 * (size_t)cols);
    if (!write_all(argv[7], got.data(), 2 * px)) return 16;
    std::printf("ok\n");
    return 0;
}
