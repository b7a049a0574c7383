// Exercises the speckle filter through include/img_completion.h: dcmt_shim::filter_speckles on a cv::Mat with padded rows, in place,
// against dcmt_filter_speckles on the same plane, byte for byte, on a raw plane written by the pytest driver.  Arguments the call
// refuses must throw.  Writes the plane the shim left.  Returns 0 when everything agreed.
//   shim_speckle_test <rows> <cols> <new_val> <max_size> <max_diff> <disp16.i16> <out.i16>
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
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), new_val = std::atoi(argv[3]), max_size = std::atoi(argv[4]),
              max_diff = std::atoi(argv[5]);
    const size_t px = (size_t)rows * cols;
    std::vector<int16_t> plane(px);
    if (!read_all(argv[6], plane.data(), 2 * px)) return 3;

    const size_t step = 2 * (size_t)cols + 6;                // the rows are 6 bytes further apart than they need to be
    std::vector<unsigned char> padded(step * rows, 0xEE);
    cv::Mat m(rows, cols, CV_16SC1, padded.data(), step);
    for (int i = 0; i < rows; ++i) std::memcpy(m.ptr<int16_t>(i), plane.data() + (size_t)cols * i, 2 * (size_t)cols);

    dcmt_speckle_params p;
    dcmt_default_speckle_params(&p);
    if (p.max_size != 200 || p.max_diff != 32 || p.new_val != -16) return 4;
    dcmt_shim::filter_speckles(m, new_val, max_size, max_diff);
    if (m.type() != CV_16SC1 || m.rows != rows || m.cols != cols || m.ptr<unsigned char>() != padded.data()) return 5;    // in place

    // the C ABI on the same plane, out of place, with the count
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 6;
    p.max_size = max_size; p.max_diff = max_diff; p.new_val = new_val;
    std::vector<int16_t> want(px, 9);
    uint32_t removed = 0xffffffffu;
    if (dcmt_filter_speckles(ctx, plane.data(), 2 * (size_t)cols, want.data(), 2 * (size_t)cols, nullptr, 0, rows, cols, &p, &removed) != DCMT_OK) return 7;
    dcmt_destroy(ctx);
    size_t differ = 0;
    for (size_t i = 0; i < px; ++i) differ += want[i] != plane[i];
    if (differ != removed || removed == 0) return 8;
    for (int i = 0; i < rows; ++i)
        if (std::memcmp(m.ptr<int16_t>(i), want.data() + (size_t)cols * i, 2 * (size_t)cols) != 0) return 9;
    for (int i = 0; i < rows; ++i)
        for (size_t k = 2 * (size_t)cols; k < step; ++k)
            if (padded[step * i + k] != 0xEE) return 10;      // the padding is not the plane's

    // an f32 plane, an 8-bit plane, an empty Mat, parameters the library refuses: thrown, and nothing written
    int thrown = 0;
    try { cv::Mat f(rows, cols, CV_32FC1); dcmt_shim::filter_speckles(f, -16, 200, 32); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat u(rows, cols, CV_8UC1); dcmt_shim::filter_speckles(u, -16, 200, 32); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat e; dcmt_shim::filter_speckles(e, -16, 200, 32); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::filter_speckles(m, -16, -1, 32); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::filter_speckles(m, -16, 200, 65536); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::filter_speckles(m, 32768, 200, 32); } catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 6) return 11;
    for (int i = 0; i < rows; ++i)
        if (std::memcmp(m.ptr<int16_t>(i), want.data() + (size_t)cols * i, 2 * (size_t)cols) != 0) return 12;

    std::vector<int16_t> got(px);
    for (int i = 0; i < rows; ++i) std::memcpy(got.data() + (size_t)cols * i, m.ptr<int16_t>(i), 2 * (size_t)cols);
    if (!write_all(argv[7], got.data(), 2 * px)) return 13;
    std::printf("ok\n");
    return 0;
}
