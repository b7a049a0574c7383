// Exercises the joint bilateral filter through include/img_completion.h: dcmt_shim::joint_bilateral_fill on cv::Mat (packed, and with
// padded rows; a grey and a three-channel guide) against dcmt_joint_bilateral on the same planes, bit for bit, on raw planes written
// by the pytest driver.  Arguments the call refuses must throw.  Writes what the shim produced.  Returns 0 when everything agreed.
//   shim_joint_test <rows> <cols> <depth.f32> <grey.u8> <bgr.u8> <filled_grey.f32> <filled_bgr.f32>
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
    if (argc < 8) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]);
    const size_t px = (size_t)rows * cols, row = 4 * (size_t)cols;
    std::vector<float> depth(px);
    std::vector<unsigned char> grey(px), bgr(3 * px);
    if (!read_all(argv[3], depth.data(), 4 * px) || !read_all(argv[4], grey.data(), px) || !read_all(argv[5], bgr.data(), 3 * px)) return 3;

    // the shim: packed images with every default; then a depth image whose rows are 3 floats apart more than they need, a padded
    // three-channel guide, another radius with smoothing and tables of the caller's
    cv::Mat d(rows, cols, CV_32FC1), g1(rows, cols, CV_8UC1);
    std::memcpy(d.ptr<float>(), depth.data(), 4 * px);
    std::memcpy(g1.ptr<unsigned char>(), grey.data(), px);
    cv::Mat filled_a, filled_b;
    unsigned left_a = 77, left_b = 77;
    const unsigned n_a = dcmt_shim::joint_bilateral_fill(d, g1, filled_a, nullptr, nullptr, 3.0, 10.0, &left_a);
    const size_t step = 4 * ((size_t)cols + 3), gstep = 3 * (size_t)cols + 5;
    std::vector<unsigned char> padded(step * rows, 0xEE), gpadded(gstep * rows, 0xEE);
    cv::Mat dp(rows, cols, CV_32FC1, padded.data(), step), g3(rows, cols, CV_8UC3, gpadded.data(), gstep);
    for (int i = 0; i < rows; ++i) {
        std::memcpy(dp.ptr<float>(i), depth.data() + (size_t)cols * i, row);
        std::memcpy(g3.ptr<unsigned char>(i), bgr.data() + 3 * (size_t)cols * i, 3 * (size_t)cols);
    }
    dcmt_joint_params wide;
    dcmt_default_joint_params(&wide);
    wide.radius = 3;
    wide.flags = DCMT_JOINT_FILL | DCMT_JOINT_SMOOTH;
    dcmt_joint_tables tab;
    if (dcmt_make_joint_tables(3, 1.5, 25.0, &tab) != DCMT_OK) return 4;
    const unsigned n_b = dcmt_shim::joint_bilateral_fill(dp, g3, filled_b, &wide, &tab, 0.0, 0.0, &left_b);
    if (filled_a.rows != rows || filled_a.cols != cols || filled_a.type() != CV_32FC1 || filled_b.rows != rows || filled_b.cols != cols) return 4;

    // the C ABI on the same data
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 5;
    dcmt_joint_params def;
    dcmt_default_joint_params(&def);
    dcmt_joint_tables dtab;
    if (dcmt_make_joint_tables(def.radius, 3.0, 10.0, &dtab) != DCMT_OK) return 5;
    std::vector<float> want_a(px), want_b(px);
    uint32_t c_a[2] = {0, 0}, c_b[2] = {0, 0};
    if (dcmt_joint_bilateral(ctx, depth.data(), row, grey.data(), (size_t)cols, 1, &dtab, want_a.data(), row, rows, cols, &def, c_a) != DCMT_OK) return 6;
    if (dcmt_joint_bilateral(ctx, depth.data(), row, bgr.data(), 3 * (size_t)cols, 3, &tab, want_b.data(), row, rows, cols, &wide, c_b) != DCMT_OK) return 6;
    dcmt_destroy(ctx);
    std::vector<float> got_a(px), got_b(px);
    for (int i = 0; i < rows; ++i) {
        std::memcpy(got_a.data() + (size_t)cols * i, filled_a.ptr<float>(i), row);
        std::memcpy(got_b.data() + (size_t)cols * i, filled_b.ptr<float>(i), row);
        for (size_t k = row; k < step; ++k)
            if (padded[step * i + k] != 0xEE) return 7;      // the input's padding is not the image's
        for (size_t k = 3 * (size_t)cols; k < gstep; ++k)
            if (gpadded[gstep * i + k] != 0xEE) return 7;
    }
    if (std::memcmp(got_a.data(), want_a.data(), 4 * px) != 0 || std::memcmp(got_b.data(), want_b.data(), 4 * px) != 0) return 8;
    if (n_a != c_a[0] || left_a != c_a[1] || n_b != c_b[0] || left_b != c_b[1] || n_a == 0 || n_b == 0) return 9;
    if (std::memcmp(d.ptr<float>(), depth.data(), 4 * px) != 0 || std::memcmp(g1.ptr<unsigned char>(), grey.data(), px) != 0) return 10;   // the inputs are not modified

    // an image of another type or size, parameters the call refuses: thrown
    int thrown = 0;
    cv::Mat o;
    try { cv::Mat z(rows, cols, CV_8UC1); dcmt_shim::joint_bilateral_fill(z, g1, o); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat g(rows, cols, CV_32FC1); dcmt_shim::joint_bilateral_fill(d, g, o); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat g(rows, cols + 1, CV_8UC1); dcmt_shim::joint_bilateral_fill(d, g, o); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_joint_params p = def; p.radius = 10; dcmt_shim::joint_bilateral_fill(d, g1, o, &p); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_joint_params p = def; p.flags = 0; dcmt_shim::joint_bilateral_fill(d, g1, o, &p); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::joint_bilateral_fill(d, g1, o, nullptr, nullptr, 0.0, 10.0); } catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 6) return 11;

    if (!write_all(argv[6], got_a.data(), 4 * px) || !write_all(argv[7], got_b.data(), 4 * px)) return 12;
    std::printf("ok\n");
    return 0;
}
