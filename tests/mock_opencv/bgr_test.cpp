// Exercises dcmt_shim::bgr_to_lab and dcmt_shim::bgr_to_gray (include/img_completion.h) the way the camera mains use cv::cvtColor
// on a frame they have just read (src/DC_lidar_camera/main_lc.cpp:183, src/DC_stereo_lidar/main_sl.cpp:439, :1167): reads a raw
// B, G, R frame written by the pytest driver into a cv::Mat with padded rows (an ROI-like view), writes the Lab and the grey frame
// as raw bytes.
//   bgr_test <rows> <cols> <in.bgr> <out.lab> <out.gray>
#include "img_completion.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static bool write_rows(const char* path, const cv::Mat& m, size_t row_bytes)
{
    FILE* o = std::fopen(path, "wb");
    if (!o) return false;
    bool ok = true;
    for (int r = 0; r < m.rows && ok; ++r) ok = std::fwrite(m.ptr<unsigned char>(r), 1, row_bytes, o) == row_bytes;
    std::fclose(o);
    return ok;
}

int main(int argc, char** argv)
{
    if (argc < 6) return 2;
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]);
    if (rows < 1 || cols < 1) return 2;
    const size_t pad = 7, row = 3 * (size_t)cols, step = row + pad;              // an odd step: no row but the first is dword-aligned
    std::vector<unsigned char> storage(step * rows, 0xEE);
    FILE* f = std::fopen(argv[3], "rb");
    if (!f) return 3;
    for (int r = 0; r < rows; ++r)
        if (std::fread(&storage[step * r], 1, row, f) != row) { std::fclose(f); return 3; }
    std::fclose(f);
    const std::vector<unsigned char> before(storage);
    const cv::Mat image(rows, cols, CV_8UC3, storage.data(), step);
    dcmt_shim::quiet() = true;

    cv::Mat lab, gray;
    dcmt_shim::bgr_to_lab(image, lab);
    dcmt_shim::bgr_to_gray(image, gray);
    if (lab.rows != rows || lab.cols != cols || lab.type() != CV_8UC3 || gray.rows != rows || gray.cols != cols || gray.type() != CV_8UC1) return 4;
    if (storage != before) return 6;                                              // the source is not the call's to touch
    cv::Mat same = image;                                                         // cvtColor(img, img, ...): source and destination one Mat
    dcmt_shim::bgr_to_lab(same, same);
    if (same.rows != rows || same.cols != cols || same.type() != CV_8UC3) return 4;
    for (int r = 0; r < rows; ++r)
        if (std::memcmp(same.ptr<unsigned char>(r), lab.ptr<unsigned char>(r), row) != 0) return 7;
    return write_rows(argv[4], lab, row) && write_rows(argv[5], gray, (size_t)cols) ? 0 : 5;
}
