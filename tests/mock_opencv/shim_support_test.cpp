// Exercises the support map and the trust mask through include/img_completion.h: dcmt_shim::distance_to_returns and
// dcmt_shim::trust_mask on cv::Mat (packed, and with padded rows) against dcmt_support_distance on the same planes, bit for bit, on raw
// f32 planes written by the pytest driver.  Arguments the calls refuse must throw.  Writes what the shim produced.  Returns 0 when
// everything agreed.
//   shim_support_test <rows> <cols> <sparse.f32> <dense.f32> <fallback.f32> <dist2.f32> <trusted.f32>
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
    std::vector<float> sparse(px), dense(px), fallback(px);
    if (!read_all(argv[3], sparse.data(), 4 * px) || !read_all(argv[4], dense.data(), 4 * px) || !read_all(argv[5], fallback.data(), 4 * px)) return 3;

    // the shim: packed images with the defaults; then a sparse image whose rows are 3 floats apart more than they need, a fallback and
    // another radius
    cv::Mat s(rows, cols, CV_32FC1), d(rows, cols, CV_32FC1), f(rows, cols, CV_32FC1);
    std::memcpy(s.ptr<float>(), sparse.data(), 4 * px);
    std::memcpy(d.ptr<float>(), dense.data(), 4 * px);
    std::memcpy(f.ptr<float>(), fallback.data(), 4 * px);
    cv::Mat dist2_a, trusted_a, trusted_b;
    const unsigned beyond_a = dcmt_shim::distance_to_returns(s, dist2_a);
    const unsigned beyond_t = dcmt_shim::trust_mask(s, d, trusted_a);
    const size_t step = 4 * ((size_t)cols + 3);
    std::vector<unsigned char> padded(step * rows, 0xEE);
    cv::Mat sp(rows, cols, CV_32FC1, padded.data(), step);
    for (int i = 0; i < rows; ++i) std::memcpy(sp.ptr<float>(i), sparse.data() + (size_t)cols * i, row);
    dcmt_support_params wide;
    dcmt_default_support_params(&wide);
    wide.max_radius = 3;
    const unsigned beyond_b = dcmt_shim::trust_mask(sp, d, trusted_b, &f, &wide);
    if (dist2_a.rows != rows || dist2_a.cols != cols || dist2_a.type() != CV_32FC1 || trusted_a.rows != rows || trusted_a.cols != cols ||
        trusted_a.type() != CV_32FC1 || trusted_b.rows != rows || trusted_b.cols != cols) return 4;

    // the C ABI on the same data
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 5;
    dcmt_support_params def;
    dcmt_default_support_params(&def);
    std::vector<uint16_t> want_d2(px);
    std::vector<float> want_a(px), want_b(px);
    uint32_t n_a = 0, n_b = 0;
    if (dcmt_support_distance(ctx, sparse.data(), row, dense.data(), row, nullptr, 0, want_a.data(), row, want_d2.data(), 2 * (size_t)cols, rows, cols, &def, &n_a) != DCMT_OK) return 6;
    if (dcmt_support_distance(ctx, sparse.data(), row, dense.data(), row, fallback.data(), row, want_b.data(), row, nullptr, 0, rows, cols, &wide, &n_b) != DCMT_OK) return 6;
    dcmt_destroy(ctx);
    std::vector<float> got_d2(px), got_a(px), got_b(px);
    for (int i = 0; i < rows; ++i) {
        std::memcpy(got_d2.data() + (size_t)cols * i, dist2_a.ptr<float>(i), row);
        std::memcpy(got_a.data() + (size_t)cols * i, trusted_a.ptr<float>(i), row);
        std::memcpy(got_b.data() + (size_t)cols * i, trusted_b.ptr<float>(i), row);
        for (size_t k = row; k < step; ++k)
            if (padded[step * i + k] != 0xEE) return 7;      // the input's padding is not the image's
    }
    for (size_t i = 0; i < px; ++i)
        if (got_d2[i] != (float)want_d2[i]) return 8;
    if (std::memcmp(got_a.data(), want_a.data(), 4 * px) != 0 || std::memcmp(got_b.data(), want_b.data(), 4 * px) != 0) return 8;
    if (beyond_a != n_a || beyond_t != n_a || beyond_b != n_b || n_a == 0 || n_b <= n_a || n_b >= px) return 9;
    if (std::memcmp(s.ptr<float>(), sparse.data(), 4 * px) != 0 || std::memcmp(d.ptr<float>(), dense.data(), 4 * px) != 0 ||
        std::memcmp(f.ptr<float>(), fallback.data(), 4 * px) != 0) return 10;                       // the inputs are not modified

    // an image of another type or size, parameters the call refuses: thrown
    int thrown = 0;
    cv::Mat o;
    try { cv::Mat g(rows, cols, CV_8UC1); dcmt_shim::distance_to_returns(g, o); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat g(rows, cols, CV_8UC1); dcmt_shim::trust_mask(s, g, o); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat g(rows, cols + 1, CV_32FC1); dcmt_shim::trust_mask(s, d, o, &g); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_support_params p = def; p.max_radius = 256; dcmt_shim::distance_to_returns(s, o, &p); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_support_params p = def; p.valid_thresh = 0.01f; dcmt_shim::trust_mask(s, d, o, nullptr, &p); } catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 5) return 11;

    if (!write_all(argv[6], got_d2.data(), 4 * px) || !write_all(argv[7], got_b.data(), 4 * px)) return 12;
    std::printf("ok\n");
    return 0;
}
