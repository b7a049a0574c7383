// Exercises dcmt_shim::unrectify_sol_nearest (include/img_completion.h) the way reproject_test.cpp exercises unrectify_sol: a
// strided source, a pre-sized strided destination that starts full of junk and whose padding is not the call's to touch.  Reads a
// raw f32 frame and the 16 floats of the row-major matrix that is applied; writes the warped frame as raw f32.
//   reproject_nearest_test <rows> <cols> <in.f32> <minv.f32> <out_rows> <out_cols> <out.f32>
#include "img_completion.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv)
{
    if (argc < 8) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), orows = std::atoi(argv[5]), ocols = std::atoi(argv[6]);
    if (rows < 1 || cols < 1 || orows < 1 || ocols < 1) return 2;
    const size_t pad = 3, opad = 5;
    std::vector<float> storage((size_t)rows * (cols + pad), -7.0f), ostorage((size_t)orows * (ocols + opad), -11.0f);
    float minv[16];
    FILE* f = std::fopen(argv[3], "rb");
    if (!f) return 3;
    for (int r = 0; r < rows; ++r)
        if (std::fread(&storage[(size_t)r * (cols + pad)], sizeof(float), (size_t)cols, f) != (size_t)cols) return 3;
    std::fclose(f);
    f = std::fopen(argv[4], "rb");
    if (!f || std::fread(minv, sizeof(float), 16, f) != 16) return 3;
    std::fclose(f);
    const cv::Mat depth(rows, cols, CV_32FC1, storage.data(), (cols + pad) * sizeof(float));
    cv::Mat unrect(orows, ocols, CV_32FC1, ostorage.data(), (ocols + opad) * sizeof(float));
    dcmt_shim::quiet() = true;

    dcmt_shim::unrectify_sol_nearest(depth, unrect, minv);
    if (unrect.rows != orows || unrect.cols != ocols || unrect.ptr<float>() != ostorage.data()) return 4;
    for (int r = 0; r < orows; ++r)
        for (size_t c = ocols; c < ocols + opad; ++c)
            if (ostorage[(size_t)r * (ocols + opad) + c] != -11.0f) return 6;
    FILE* o = std::fopen(argv[7], "wb");
    if (!o) return 5;
    for (int r = 0; r < orows; ++r)
        if (std::fwrite(unrect.ptr<float>(r), sizeof(float), (size_t)ocols, o) != (size_t)ocols) { std::fclose(o); return 5; }
    std::fclose(o);
    return 0;
}
