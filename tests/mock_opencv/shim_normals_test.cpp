// Exercises the normals and the flying-pixel filter through include/img_completion.h: dcmt_shim::depth_normals and
// dcmt_shim::filter_flying_pixels on a cv::Mat (one packed, one with padded rows) against dcmt_depth_normals on the same plane, bit for
// bit, on a raw f32 plane written by the pytest driver.  Arguments the call refuses must throw.  Writes the plane and the records the
// shim produced.  Returns 0 when everything agreed.
//   shim_normals_test <rows> <cols> <depth.f32> <filtered.f32> <normals.f32>
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
    if (argc < 6) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]);
    const size_t px = (size_t)rows * cols;
    std::vector<float> depth(px);
    if (!read_all(argv[3], depth.data(), 4 * px)) return 3;
    static_assert(sizeof(dcmt_normal) == 16 && sizeof(dcmt_normals_params) == 12, "layouts");

    // the shim: a packed cv::Mat with the defaults, one whose rows are 3 floats apart more than they need with other parameters
    cv::Mat a(rows, cols, CV_32FC1);
    std::memcpy(a.ptr<float>(), depth.data(), 4 * px);
    cv::Mat filtered_a;
    std::vector<dcmt_normal> normals_a, with_filter;
    const unsigned none_a = dcmt_shim::depth_normals(a, normals_a);
    const unsigned removed_a = dcmt_shim::filter_flying_pixels(a, filtered_a, nullptr, nullptr, &with_filter);
    const size_t step = 4 * ((size_t)cols + 3);
    std::vector<unsigned char> padded(step * rows, 0xEE);
    cv::Mat b(rows, cols, CV_32FC1, padded.data(), step);
    for (int i = 0; i < rows; ++i) std::memcpy(b.ptr<float>(i), depth.data() + (size_t)cols * i, 4 * (size_t)cols);
    dcmt_cloud_params kitti = {721.5, 721.5, 608.0, 176.0};
    dcmt_normals_params wide;
    dcmt_default_normals_params(&wide);
    wide.min_plane_dist = 30.0f;
    cv::Mat filtered_b;
    const unsigned removed_b = dcmt_shim::filter_flying_pixels(b, filtered_b, &kitti, &wide);
    if (filtered_a.rows != rows || filtered_a.cols != cols || filtered_a.type() != CV_32FC1 || filtered_b.rows != rows || filtered_b.cols != cols) return 4;
    if (normals_a.size() != px || with_filter.size() != px || std::memcmp(normals_a.data(), with_filter.data(), 16 * px) != 0) return 4;

    // the C ABI on the same data
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 5;
    dcmt_cloud_params cdef;
    dcmt_default_cloud_params(&cdef);
    dcmt_normals_params def;
    dcmt_default_normals_params(&def);
    std::vector<float> want_a(px), want_b(px);
    std::vector<dcmt_normal> want_n(px);
    uint32_t n_a[2] = {0, 0}, n_b[2] = {0, 0};
    const size_t row = 4 * (size_t)cols;
    if (dcmt_depth_normals(ctx, depth.data(), row, rows, cols, &cdef, &def, want_n.data(), 4 * row, want_a.data(), row, n_a) != DCMT_OK) return 6;
    if (dcmt_depth_normals(ctx, depth.data(), row, rows, cols, &kitti, &wide, nullptr, 0, want_b.data(), row, n_b) != DCMT_OK) return 6;
    dcmt_destroy(ctx);
    std::vector<float> got_a(px), got_b(px);
    for (int i = 0; i < rows; ++i) {
        std::memcpy(got_a.data() + (size_t)cols * i, filtered_a.ptr<float>(i), row);
        std::memcpy(got_b.data() + (size_t)cols * i, filtered_b.ptr<float>(i), row);
        for (size_t k = row; k < step; ++k)
            if (padded[step * i + k] != 0xEE) return 7;      // the input's padding is not the image's
    }
    if (std::memcmp(got_a.data(), want_a.data(), 4 * px) != 0) return 8;
    if (std::memcmp(got_b.data(), want_b.data(), 4 * px) != 0) return 8;
    if (std::memcmp(normals_a.data(), want_n.data(), 16 * px) != 0) return 8;
    if (removed_a != n_a[0] || none_a != n_a[1] || removed_b != n_b[0] || n_b[0] == 0 || n_b[0] <= n_a[0]) return 9;
    for (int i = 0; i < rows; ++i)                           // the inputs are not modified
        if (std::memcmp(b.ptr<float>(i), depth.data() + (size_t)cols * i, row) != 0 || std::memcmp(a.ptr<float>(i), depth.data() + (size_t)cols * i, row) != 0) return 10;

    // an image of another type, parameters and intrinsics the call refuses: thrown
    int thrown = 0;
    cv::Mat o;
    std::vector<dcmt_normal> q;
    try { cv::Mat g(rows, cols, CV_8UC1); dcmt_shim::filter_flying_pixels(g, o); } catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat g(rows, cols, CV_8UC1); dcmt_shim::depth_normals(g, q); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_normals_params p = def; p.min_plane_dist = -1.0f; dcmt_shim::filter_flying_pixels(a, o, nullptr, &p); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_normals_params p = def; p.valid_thresh = 0.01f; dcmt_shim::depth_normals(a, q, nullptr, &p); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_cloud_params k = kitti; k.fx = 0.0; dcmt_shim::depth_normals(a, q, &k); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_cloud_params k = kitti; k.cy = 3e6; dcmt_shim::filter_flying_pixels(a, o, &k); } catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 6) return 11;

    if (!write_all(argv[4], got_b.data(), 4 * px) || !write_all(argv[5], normals_a.data(), 16 * px)) return 12;
    std::printf("ok\n");
    return 0;
}
