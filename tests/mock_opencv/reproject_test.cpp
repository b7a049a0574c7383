// Exercises dcmt_shim::unrectify_sol (include/img_completion.h) the way the stereo-lidar main uses its unrectify_sol on the
// pre-refinement depth (src/DC_stereo_lidar/main_sl.cpp:1227-1228): a pre-sized destination, no image argument.  Reads a raw f32
// frame and the 16 floats of the row-major matrix that is applied, written by the pytest driver, into cv::Mats with padded rows (the
// destination starts full of junk: the call must overwrite all of it); writes the warped frame as raw f32.
//   reproject_test <rows> <cols> <in.f32> <minv.f32> <out_rows> <out_cols> <out.f32>
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
    if (argc < 8) return 2;
    static_assert(sizeof(dcmt_reproject_params) == 4 * 8 + 16 * 4 + 9 * 4 + 4, "parameter layout");
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), orows = std::atoi(argv[5]), ocols = std::atoi(argv[6]);
    if (rows < 1 || cols < 1 || orows < 1 || ocols < 1) return 2;
    const size_t pad = 8, opad = 5, px = (size_t)rows * cols;                    // ROI-like strided source and destination
    std::vector<float> packed(px), storage((size_t)rows * (cols + pad), -7.0f), ostorage((size_t)orows * (ocols + opad), -11.0f);
    float minv[16];
    if (!read_all(argv[3], packed.data(), px * sizeof(float)) || !read_all(argv[4], minv, sizeof minv)) return 3;
    for (int r = 0; r < rows; ++r) std::memcpy(&storage[(size_t)r * (cols + pad)], &packed[(size_t)r * cols], (size_t)cols * 4);
    const cv::Mat depth(rows, cols, CV_32FC1, storage.data(), (cols + pad) * sizeof(float));
    cv::Mat unrect(orows, ocols, CV_32FC1, ostorage.data(), (ocols + opad) * sizeof(float));
    dcmt_shim::quiet() = true;

    dcmt_shim::unrectify_sol(depth, unrect, minv);
    if (unrect.rows != orows || unrect.cols != ocols || unrect.ptr<float>() != ostorage.data()) return 4;
    for (int r = 0; r < orows; ++r)                                              // the padding is not the call's to touch
        for (size_t c = ocols; c < ocols + opad; ++c)
            if (ostorage[(size_t)r * (ocols + opad) + c] != -11.0f) return 6;
    FILE* o = std::fopen(argv[7], "wb");
    if (!o) return 5;
    for (int r = 0; r < orows; ++r)
        if (std::fwrite(unrect.ptr<float>(r), sizeof(float), (size_t)ocols, o) != (size_t)ocols) { std::fclose(o); return 5; }
    std::fclose(o);
    return 0;
}
