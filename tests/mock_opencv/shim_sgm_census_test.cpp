// Exercises the census matching cost through include/img_completion.h: dcmt_shim::stereo_sgm_cost on cv::Mats (the guide with padded
// rows, and an empty guide) against dcmt_sgm_cost on the same planes, byte for byte, with eight paths and a guide and with four paths
// and none; with DCMT_SGM_COST_ABSDIFF against dcmt_shim::stereo_sgm_guided and dcmt_shim::stereo_sgm_paths.  A cost that does not
// exist must throw.  Writes the guided eight-path census map and the unguided four-path one the shim returned.  Returns 0 when
// everything agreed.
//   shim_sgm_census_test <rows> <cols> <num_disparities> <left.u8> <right.u8> <guide.f32> <guided8.i16> <plain4.i16>
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

static bool write_rows(const char* path, const cv::Mat& m, int rows, int cols)
{
    FILE* f = std::fopen(path, "wb");
    bool ok = f != nullptr;
    for (int i = 0; ok && i < rows; ++i) ok = std::fwrite(m.ptr<int16_t>(i), 2, (size_t)cols, f) == (size_t)cols;
    if (f) std::fclose(f);
    return ok;
}

static bool same_rows(const cv::Mat& m, const int16_t* want, int rows, int cols)
{
    for (int i = 0; i < rows; ++i)
        if (std::memcmp(m.ptr<int16_t>(i), want + (size_t)cols * i, 2 * (size_t)cols) != 0) return false;
    return true;
}

static bool same_mats(const cv::Mat& a, const cv::Mat& b, int rows, int cols)
{
    for (int i = 0; i < rows; ++i)
        if (std::memcmp(a.ptr<int16_t>(i), b.ptr<int16_t>(i), 2 * (size_t)cols) != 0) return false;
    return true;
}

int main(int argc, char** argv)
{
    if (argc < 9) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), disparities = std::atoi(argv[3]);
    const size_t px = (size_t)rows * cols;
    std::vector<unsigned char> left(px), right(px);
    std::vector<float> guide(px);
    if (!read_all(argv[4], left.data(), px) || !read_all(argv[5], right.data(), px) || !read_all(argv[6], guide.data(), 4 * px)) return 3;

    cv::Mat l(rows, cols, CV_8UC1), r(rows, cols, CV_8UC1), none;
    std::memcpy(l.ptr<unsigned char>(), left.data(), px);
    std::memcpy(r.ptr<unsigned char>(), right.data(), px);
    const size_t step = 4 * ((size_t)cols + 3);              // the guide's rows are 12 bytes further apart than they need to be
    std::vector<unsigned char> padded(step * rows, 0xEE);
    cv::Mat g(rows, cols, CV_32FC1, padded.data(), step);
    for (int i = 0; i < rows; ++i) std::memcpy(g.ptr<float>(i), guide.data() + (size_t)cols * i, 4 * (size_t)cols);

    dcmt_sgm_params p;
    dcmt_default_sgm_params(&p);
    p.num_disparities = disparities;
    cv::Mat guided8, plain4, absdiff_guided, absdiff_plain, old_guided, old_plain;
    dcmt_shim::stereo_sgm_cost(l, r, g, guided8, 8, 100, 1000, DCMT_SGM_COST_CENSUS, &p);
    dcmt_shim::stereo_sgm_cost(l, r, none, plain4, 4, -5, -5, DCMT_SGM_COST_CENSUS, &p);        // without a guide the integers are not looked at
    dcmt_shim::stereo_sgm_cost(l, r, g, absdiff_guided, 8, 100, 1000, DCMT_SGM_COST_ABSDIFF, &p);
    dcmt_shim::stereo_sgm_cost(l, r, none, absdiff_plain, 8, 0, 0, DCMT_SGM_COST_ABSDIFF, &p);
    dcmt_shim::stereo_sgm_guided(l, r, g, old_guided, 8, 100, 1000, &p);
    dcmt_shim::stereo_sgm_paths(l, r, old_plain, 8, &p);
    for (const cv::Mat* m : {&guided8, &plain4, &absdiff_guided, &absdiff_plain, &old_guided, &old_plain})
        if (m->type() != CV_16SC1 || m->rows != rows || m->cols != cols) return 5;

    // the C ABI on the same planes
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 6;
    std::vector<int16_t> want8(px, 9), want4(px, 9);
    if (dcmt_sgm_cost(ctx, left.data(), cols, right.data(), cols, guide.data(), 4 * (size_t)cols, rows, cols, &p, want8.data(), 2 * (size_t)cols, nullptr, 0, 8,
                      100, 1000, DCMT_SGM_COST_CENSUS) != DCMT_OK) return 7;
    if (dcmt_sgm_cost(ctx, left.data(), cols, right.data(), cols, nullptr, 0, rows, cols, &p, want4.data(), 2 * (size_t)cols, nullptr, 0, 4, 0, 0,
                      DCMT_SGM_COST_CENSUS) != DCMT_OK) return 7;
    // refused by the C call: nothing written
    std::vector<int16_t> untouched(px, 9);
    for (int cost : {2, -1})
        if (dcmt_sgm_cost(ctx, left.data(), cols, right.data(), cols, guide.data(), 4 * (size_t)cols, rows, cols, &p, untouched.data(), 2 * (size_t)cols,
                          nullptr, 0, 8, 100, 1000, cost) != DCMT_E_INVALID) return 8;
    if (dcmt_sgm_cost(ctx, left.data(), cols, right.data(), cols, guide.data(), 4 * (size_t)cols, rows, cols, &p, untouched.data(), 2 * (size_t)cols, nullptr,
                      0, 8, 100, 1001, DCMT_SGM_COST_CENSUS) != DCMT_E_INVALID) return 8;
    for (size_t i = 0; i < px; ++i)
        if (untouched[i] != 9) return 8;
    dcmt_destroy(ctx);
    if (!same_rows(guided8, want8.data(), rows, cols)) return 9;
    if (!same_rows(plain4, want4.data(), rows, cols)) return 10;
    if (!same_mats(absdiff_guided, old_guided, rows, cols) || !same_mats(absdiff_plain, old_plain, rows, cols)) return 11;
    if (same_mats(guided8, old_guided, rows, cols)) return 12;                      // the cost changes something on this pair
    for (int i = 0; i < rows; ++i)
        for (size_t k = 4 * (size_t)cols; k < step; ++k)
            if (padded[step * i + k] != 0xEE) return 13;      // the padding is not the guide's

    // a cost that does not exist, and what stereo_sgm_guided refuses: thrown
    int thrown = 0;
    cv::Mat sink;
    try { dcmt_shim::stereo_sgm_cost(l, r, g, sink, 8, 100, 1000, 2); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::stereo_sgm_cost(l, r, none, sink, 4, 0, 0, -1); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::stereo_sgm_cost(l, r, g, sink, 8, 100, 1001, DCMT_SGM_COST_CENSUS); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::stereo_sgm_cost(l, r, none, sink, 5, 0, 0, DCMT_SGM_COST_CENSUS); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat c(rows, cols, CV_8UC1); dcmt_shim::stereo_sgm_cost(l, r, c, sink, 8, 100, 1000, DCMT_SGM_COST_CENSUS); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat s(rows, cols + 1, CV_32FC1); dcmt_shim::stereo_sgm_cost(l, r, s, sink, 8, 100, 1000, DCMT_SGM_COST_CENSUS); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat c(rows, cols, CV_8UC3); dcmt_shim::stereo_sgm_cost(c, r, none, sink, 4, 0, 0, DCMT_SGM_COST_CENSUS); } catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 7) return 14;

    if (!write_rows(argv[7], guided8, rows, cols) || !write_rows(argv[8], plain4, rows, cols)) return 16;
    std::printf("ok\n");
    return 0;
}
