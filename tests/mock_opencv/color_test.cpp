// Exercises dcmt_shim::to_color_image (include/img_completion.h) the way a reference main's toColorImage would call it
// (src/DC_lidar_only/main.cpp:6-14, :97).  Reads a raw f32 frame written by the pytest driver into a cv::Mat with padded rows,
// writes the CV_8UC3 result as raw B, G, R bytes.
//   color_test <rows> <cols> <in.f32> <out.u8>
#include "img_completion.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]);
    const size_t pad = 8, row_step = (size_t)(cols + pad) * sizeof(float);    // a ROI-like strided input
    std::vector<float> storage((size_t)rows * (cols + pad), -7.0f), packed((size_t)rows * cols);
    FILE* f = std::fopen(argv[3], "rb");
    if (!f) return 3;
    const size_t got = std::fread(packed.data(), sizeof(float), packed.size(), f);
    std::fclose(f);
    if (got != packed.size()) return 3;
    for (int r = 0; r < rows; ++r) std::memcpy(&storage[(size_t)r * (cols + pad)], &packed[(size_t)r * cols], (size_t)cols * 4);
    const cv::Mat r_img(rows, cols, CV_32FC1, storage.data(), row_step);
    cv::Mat color_img;
    dcmt_shim::quiet() = true;
    dcmt_shim::to_color_image(r_img, color_img);
    if (color_img.rows != rows || color_img.cols != cols || color_img.type() != CV_8UC3) return 4;
    FILE* o = std::fopen(argv[4], "wb");
    if (!o) return 5;
    for (int r = 0; r < rows; ++r)
        if (std::fwrite(color_img.ptr<unsigned char>(r), 1, 3 * (size_t)cols, o) != 3 * (size_t)cols) { std::fclose(o); return 5; }
    std::fclose(o);
    return 0;
}
