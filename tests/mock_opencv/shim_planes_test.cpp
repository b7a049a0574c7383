// Exercises the per-superpixel plane fit through include/img_completion.h: dcmt_shim::fit_superpixel_planes on clusters[col][row] and
// a cv::Mat (one packed, one with padded rows) against dcmt_superpixel_planes on the same labels row-major, bit for bit, on a raw
// f32 plane and a raw int32 plane written by the pytest driver.  Arguments the call refuses must throw.  Writes the plane and the
// fits the shim produced.  Returns 0 when everything agreed.
//   shim_planes_test <rows> <cols> <n_labels> <depth.f32> <labels.i32> <planes.f32> <fits.bin>
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
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), n_labels = std::atoi(argv[3]);
    const size_t px = (size_t)rows * cols;
    std::vector<float> depth(px);
    std::vector<int32_t> packed(px);
    if (!read_all(argv[4], depth.data(), 4 * px) || !read_all(argv[5], packed.data(), 4 * px)) return 3;
    std::vector<std::vector<int> > clusters(cols, std::vector<int>(rows));
    for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) clusters[j][i] = packed[(size_t)i * cols + j];

    // the shim: a packed cv::Mat with the defaults and the fits, one whose rows are 3 floats apart more than they need with a refit
    cv::Mat a(rows, cols, CV_32FC1);
    std::memcpy(a.ptr<float>(), depth.data(), 4 * px);
    cv::Mat planes_a;
    std::vector<dcmt_plane_fit> fits_a;
    dcmt_shim::fit_superpixel_planes(clusters, n_labels, a, planes_a, nullptr, &fits_a);
    const size_t step = 4 * ((size_t)cols + 3);
    std::vector<unsigned char> padded(step * rows, 0xEE);
    cv::Mat b(rows, cols, CV_32FC1, padded.data(), step);
    for (int i = 0; i < rows; ++i) std::memcpy(b.ptr<float>(i), depth.data() + (size_t)cols * i, 4 * (size_t)cols);
    dcmt_planes_params refit;
    dcmt_default_planes_params(&refit);
    refit.refit_tol = 0.1f;
    refit.keep_returns = 0;
    cv::Mat planes_b;
    dcmt_shim::fit_superpixel_planes(clusters, n_labels, b, planes_b, &refit);
    if (planes_a.rows != rows || planes_a.cols != cols || planes_a.type() != CV_32FC1 || planes_b.rows != rows || planes_b.cols != cols) return 4;
    if ((int)fits_a.size() != n_labels) return 4;

    // the C ABI on the same data
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 5;
    dcmt_planes_params def;
    dcmt_default_planes_params(&def);
    std::vector<float> want_a(px), want_b(px);
    std::vector<dcmt_plane_fit> want_f(n_labels);
    const size_t row = 4 * (size_t)cols;
    if (dcmt_superpixel_planes(ctx, depth.data(), row, packed.data(), row, rows, cols, n_labels, &def, want_a.data(), row, want_f.data()) != DCMT_OK) return 6;
    if (dcmt_superpixel_planes(ctx, depth.data(), row, packed.data(), row, rows, cols, n_labels, &refit, want_b.data(), row, nullptr) != DCMT_OK) return 6;
    dcmt_destroy(ctx);
    std::vector<float> got_a(px), got_b(px);
    for (int i = 0; i < rows; ++i) {
        std::memcpy(got_a.data() + (size_t)cols * i, planes_a.ptr<float>(i), row);
        std::memcpy(got_b.data() + (size_t)cols * i, planes_b.ptr<float>(i), row);
        for (size_t k = row; k < step; ++k)
            if (padded[step * i + k] != 0xEE) return 7;      // the input's padding is not the image's
    }
    if (std::memcmp(got_a.data(), want_a.data(), 4 * px) != 0) return 8;
    if (std::memcmp(got_b.data(), want_b.data(), 4 * px) != 0) return 8;
    if (std::memcmp(fits_a.data(), want_f.data(), sizeof(dcmt_plane_fit) * (size_t)n_labels) != 0) return 9;
    for (int i = 0; i < rows; ++i)                           // the inputs are not modified
        if (std::memcmp(b.ptr<float>(i), depth.data() + (size_t)cols * i, row) != 0 || std::memcmp(a.ptr<float>(i), depth.data() + (size_t)cols * i, row) != 0) return 10;

    // an image of another type, clusters of another size, no labels, parameters the call refuses: thrown
    int thrown = 0;
    cv::Mat o;
    try { cv::Mat g(rows, cols, CV_8UC1); dcmt_shim::fit_superpixel_planes(clusters, n_labels, g, o); } catch (const std::runtime_error&) { ++thrown; }
    try { std::vector<std::vector<int> > c = clusters; c[cols - 1].push_back(0); dcmt_shim::fit_superpixel_planes(c, n_labels, a, o); } catch (const std::runtime_error&) { ++thrown; }
    try { std::vector<std::vector<int> > c = clusters; c.push_back(c[0]); dcmt_shim::fit_superpixel_planes(c, n_labels, a, o); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_shim::fit_superpixel_planes(clusters, 0, a, o); } catch (const std::runtime_error&) { ++thrown; }
    try { dcmt_planes_params p = def; p.min_points = 2; dcmt_shim::fit_superpixel_planes(clusters, n_labels, a, o, &p); } catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 5) return 11;

    if (!write_all(argv[6], got_a.data(), 4 * px) || !write_all(argv[7], fits_a.data(), sizeof(dcmt_plane_fit) * (size_t)n_labels)) return 12;
    std::printf("ok\n");
    return 0;
}
