// Exercises SLIC's two pixel renderings through include/img_completion.h: dcmt_shim::slic_display_contours and
// dcmt_shim::slic_colour_with_cluster_means on clusters[col][row] and a cv::Mat (one packed, one with padded rows) against
// dcmt_slic_contours / dcmt_slic_cluster_means on the same labels row-major, byte for byte, on a raw int32 plane and a raw
// BGR image written by the pytest driver.  Arguments the calls refuse must throw.  Writes the two images the shim painted.
// Returns 0 when everything agreed.
//   shim_contours_test <rows> <cols> <n_labels> <labels.i32> <image.u8> <contours.u8> <means.u8>
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
    std::vector<int32_t> packed(px);
    std::vector<unsigned char> image(3 * px);
    if (!read_all(argv[4], packed.data(), 4 * px) || !read_all(argv[5], image.data(), 3 * px)) return 3;
    std::vector<std::vector<int> > clusters(cols, std::vector<int>(rows));
    for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) clusters[j][i] = packed[(size_t)i * cols + j];
    const double colour[4] = {0, 0, 200, 0};                 // CV_RGB(200,0,0) as a cv::Scalar holds it

    // the shim: contours into a packed cv::Mat, means into one whose rows are 5 bytes apart more than they need
    cv::Mat a(rows, cols, CV_8UC3);
    std::memcpy(a.ptr<unsigned char>(), image.data(), 3 * px);
    dcmt_shim::slic_display_contours(clusters, a, colour);
    const size_t step = 3 * (size_t)cols + 5;
    std::vector<unsigned char> padded(step * rows, 0xEE);
    cv::Mat b(rows, cols, CV_8UC3, padded.data(), step);
    for (int i = 0; i < rows; ++i) std::memcpy(b.ptr<unsigned char>(i), image.data() + 3 * (size_t)cols * i, 3 * (size_t)cols);
    dcmt_shim::slic_colour_with_cluster_means(clusters, b, n_labels);

    // the C ABI on the same data
    dcmt_ctx* ctx = nullptr;
    if (dcmt_create(0, rows, cols, 1, &ctx) != DCMT_OK) return 4;
    std::vector<unsigned char> want_c = image, want_m = image, mask(px, 7);
    const uint8_t red[3] = {0, 0, 200};
    const size_t lrow = sizeof(int32_t) * (size_t)cols, irow = 3 * (size_t)cols;
    if (dcmt_slic_contours(ctx, packed.data(), lrow, rows, cols, want_c.data(), irow, red, mask.data(), cols) != DCMT_OK) return 5;
    if (dcmt_slic_cluster_means(ctx, packed.data(), lrow, rows, cols, n_labels, want_m.data(), irow, nullptr) != DCMT_OK) return 5;
    dcmt_destroy(ctx);
    if (std::memcmp(a.ptr<unsigned char>(), want_c.data(), 3 * px) != 0) return 6;
    std::vector<unsigned char> got_m(3 * px);
    for (int i = 0; i < rows; ++i) {
        std::memcpy(got_m.data() + irow * i, b.ptr<unsigned char>(i), irow);
        for (size_t k = irow; k < step; ++k)
            if (padded[step * i + k] != 0xEE) return 7;      // the padding is not the image's
    }
    if (got_m != want_m) return 8;
    for (size_t p = 0; p < px; ++p) {                        // the mask and the painted image say the same
        const bool painted = want_c[3 * p] == 0 && want_c[3 * p + 1] == 0 && want_c[3 * p + 2] == 200;
        if (mask[p] != 0 && mask[p] != 255) return 9;
        if (mask[p] == 255 && !painted) return 9;
        if (mask[p] == 0 && std::memcmp(&want_c[3 * p], &image[3 * p], 3) != 0) return 9;
    }

    // a grey image, clusters of another size, no labels at all: refused
    int thrown = 0;
    try { cv::Mat g(rows, cols, CV_8UC1); dcmt_shim::slic_display_contours(clusters, g, colour); } catch (const std::runtime_error&) { ++thrown; }
    try { std::vector<std::vector<int> > c = clusters; c[cols - 1].push_back(0); cv::Mat m(rows, cols, CV_8UC3); dcmt_shim::slic_colour_with_cluster_means(c, m, n_labels); }
    catch (const std::runtime_error&) { ++thrown; }
    try { std::vector<std::vector<int> > c = clusters; c.push_back(c[0]); cv::Mat m(rows, cols, CV_8UC3); dcmt_shim::slic_display_contours(c, m, colour); }
    catch (const std::runtime_error&) { ++thrown; }
    try { cv::Mat m(rows, cols, CV_8UC3); std::memset(m.ptr<unsigned char>(), 0, 3 * px); dcmt_shim::slic_colour_with_cluster_means(clusters, m, 0); }
    catch (const std::runtime_error&) { ++thrown; }
    if (thrown != 4) return 10;

    if (!write_all(argv[6], a.ptr<unsigned char>(), 3 * px) || !write_all(argv[7], got_m.data(), 3 * px)) return 11;
    std::printf("ok\n");
    return 0;
}
