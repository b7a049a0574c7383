// Exercises dcmt_shim::gaussian_blur5 and dcmt_shim::depth_to_cloud (include/img_completion.h) the way the stereo-lidar main uses
// its GaussianBlur and reproject_pc_colors on the refined depth (src/DC_stereo_lidar/main_sl.cpp:1253, :1270).  Reads a raw f32
// frame (and raw B, G, R bytes, or "-" for none) written by the pytest driver into cv::Mats with padded rows; writes the blurred
// frame as raw f32 and the cloud of the UNBLURRED frame as raw 16-byte records.
//   cloud_test <rows> <cols> <in.f32> <in.bgr | -> <out_blur.f32> <out_cloud.bin>
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
    if (argc < 7) return 2;
    static_assert(sizeof(dcmt_cloud_point) == 16 && sizeof(dcmt_cloud_params) == 32, "record layout");
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]);
    const bool colour = std::strcmp(argv[4], "-") != 0;
    const size_t pad = 8, px = (size_t)rows * cols;                           // ROI-like strided inputs
    const size_t dstep = (size_t)(cols + pad) * sizeof(float), cstep = 3 * (size_t)cols + 5;
    std::vector<float> packed(px), storage((size_t)rows * (cols + pad), -7.0f);
    std::vector<unsigned char> cpacked(3 * px), cstorage(cstep * rows, 0x5a);
    if (!read_all(argv[3], packed.data(), px * sizeof(float))) return 3;
    if (colour && !read_all(argv[4], cpacked.data(), 3 * px)) return 3;
    for (int r = 0; r < rows; ++r) {
        std::memcpy(&storage[(size_t)r * (cols + pad)], &packed[(size_t)r * cols], (size_t)cols * 4);
        std::memcpy(&cstorage[cstep * r], &cpacked[3 * (size_t)r * cols], 3 * (size_t)cols);
    }
    const cv::Mat depth(rows, cols, CV_32FC1, storage.data(), dstep);
    const cv::Mat bgr = colour ? cv::Mat(rows, cols, CV_8UC3, cstorage.data(), cstep) : cv::Mat();
    dcmt_shim::quiet() = true;

    cv::Mat blurred;
    dcmt_shim::gaussian_blur5(depth, blurred);
    if (blurred.rows != rows || blurred.cols != cols || blurred.type() != CV_32FC1) return 4;
    FILE* o = std::fopen(argv[5], "wb");
    if (!o) return 5;
    for (int r = 0; r < rows; ++r)
        if (std::fwrite(blurred.ptr<float>(r), sizeof(float), (size_t)cols, o) != (size_t)cols) { std::fclose(o); return 5; }
    std::fclose(o);

    std::vector<dcmt_cloud_point> cloud;
    dcmt_shim::depth_to_cloud(depth, bgr, cloud);
    o = std::fopen(argv[6], "wb");
    if (!o) return 5;
    if (!cloud.empty() && std::fwrite(cloud.data(), sizeof(dcmt_cloud_point), cloud.size(), o) != cloud.size()) { std::fclose(o); return 5; }
    std::fclose(o);
    return 0;
}
