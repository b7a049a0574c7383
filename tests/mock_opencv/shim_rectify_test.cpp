// Exercises dcmt_shim::undistort_rectify (include/img_completion.h) against dcmt_rectify, byte for byte, on a raw 8-bit frame the
// pytest driver wrote, held in a cv::Mat with padded rows; 1 or 3 channels.  The record is read as 22 raw doubles.  Writes the
// shim's result packed.  Returns 0 when everything agreed.
//   shim_rectify_test <src_rows> <src_cols> <channels> <rows> <cols> <in.u8> <calib.f64> <out.u8>
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

int main(int argc, char** argv)
{
    if (argc < 9) return 2;
    const int src_rows = std::atoi(argv[1]), src_cols = std::atoi(argv[2]), ch = std::atoi(argv[3]), rows = std::atoi(argv[4]), cols = std::atoi(argv[5]);
    if (ch != 1 && ch != 3) return 2;
    const size_t row = (size_t)src_cols * ch, pad = 7, step = row + pad, out_row = (size_t)cols * ch;
    std::vector<unsigned char> packed(row * src_rows), storage(step * src_rows, 0xEE);
    dcmt_rectify_calib calib;
    if (sizeof calib != 22 * sizeof(double)) return 3;
    if (!read_all(argv[6], packed.data(), packed.size()) || !read_all(argv[7], &calib, sizeof calib)) return 3;
    for (int r = 0; r < src_rows; ++r) std::memcpy(&storage[r * step], &packed[r * row], row);
    const int type = ch == 3 ? CV_8UC3 : CV_8UC1;
    const cv::Mat src(src_rows, src_cols, type, storage.data(), step);

    cv::Mat dst;
    dcmt_shim::undistort_rectify(src, dst, calib, rows, cols);
    if (dst.rows != rows || dst.cols != cols || dst.type() != type) return 4;

    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 5;
    std::vector<unsigned char> want(out_row * rows, 0x77);
    if (dcmt_rectify(ctx, packed.data(), row, src_rows, src_cols, ch, &calib, want.data(), out_row, rows, cols) != DCMT_OK) return 6;
    for (int r = 0; r < rows; ++r)
        if (std::memcmp(dst.ptr<unsigned char>(r), &want[r * out_row], out_row) != 0) return 7;
    if (std::strstr(dcmt_last_path(ctx), "k_rectify<") == nullptr) return 8;

    // what the C call refuses
    if (dcmt_rectify(ctx, packed.data(), row, src_rows, src_cols, 2, &calib, want.data(), out_row, rows, cols) != DCMT_E_INVALID) return 9;
    if (dcmt_rectify(ctx, packed.data(), row - 1, src_rows, src_cols, ch, &calib, want.data(), out_row, rows, cols) != DCMT_E_INVALID) return 9;
    if (dcmt_rectify(ctx, packed.data(), row, src_rows, src_cols, ch, nullptr, want.data(), out_row, rows, cols) != DCMT_E_INVALID) return 9;
    if (dcmt_rectify(ctx, packed.data(), row, src_rows, src_cols, ch, &calib, want.data(), out_row, rows + 1, cols) != DCMT_E_INVALID) return 9;
    // ... and the shim: a type that is not 8-bit
    bool thrown = false;
    try { cv::Mat f(4, 4, CV_32FC1), t; dcmt_shim::undistort_rectify(f, t, calib, rows, cols); } catch (const std::runtime_error&) { thrown = true; }
    if (!thrown) return 10;
    dcmt_destroy(ctx);

    FILE* o = std::fopen(argv[8], "wb");
    if (!o) return 11;
    bool ok = true;
    for (int r = 0; r < rows; ++r) ok = ok && std::fwrite(dst.ptr<unsigned char>(r), 1, out_row, o) == out_row;
    std::fclose(o);
    return ok ? 0 : 11;
}
