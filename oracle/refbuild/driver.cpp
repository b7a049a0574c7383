/* C ABI over the reference's whole-file translation units (img_completion.cpp, img_completion_lc.cpp, slic.cpp), which
 * build_ref.py compiles in place and unmodified next to this file.  Everything here is plumbing: wrap the caller's
 * buffers in cv::Mat headers, call the reference's function, copy the result out.  TEST INFRASTRUCTURE. */
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "img_completion.h"
#include "slic.h"          /* the reference's own header, found through the include path of the build */
#include "quiet.h"

void interpolate_with_superpixels(Slic &, const cv::Mat &, cv::Mat &, const std::string &, int);

namespace {
void copy_out(const cv::Mat &m, float *dst, int rows, int cols)
{
    for (int r = 0; r < rows; ++r) std::memcpy(dst + (size_t)r * cols, &m.at<float>(r, 0), sizeof(float) * (size_t)cols);
}
}  // namespace

extern "C" {

int ref_abi_version(void) { return 1; }

/* img_completion on one f32 frame; blur_type is handed through as the reference's string argument */
void ref_img_completion(const float *src, float *dst, int rows, int cols, const char *blur_type)
{
    refbuild::Quiet q;
    const cv::Mat in(rows, cols, CV_32F, (void *)src);
    cv::Mat out;
    img_completion(in, out, false, std::string(blur_type));
    copy_out(out, dst, rows, cols);
}

/* Slic::generate_superpixels on an 8-bit 3-channel image [rows][cols][3]: labels int32 [rows][cols] (from the
 * object's clusters[col][row]), up to max_centers rows of 5 doubles.  Returns centers.size(). */
int ref_slic(const uint8_t *img, int rows, int cols, int step, int nc, int32_t *labels, double *centers, int max_centers)
{
    refbuild::Quiet q;
    cv::Mat image(rows, cols, CV_8UC3, (void *)img);
    Slic slic;
    slic.generate_superpixels(image, step, nc);
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r) labels[(size_t)r * cols + c] = slic.clusters[c][r];
    const int n = (int)slic.centers.size();
    if (centers)
        for (int j = 0; j < n && j < max_centers; ++j)
            for (int k = 0; k < 5; ++k) centers[5 * (size_t)j + k] = slic.centers[j][k];
    return n;
}

/* interpolate_with_superpixels fed through a Slic object whose clusters[col][row] and centers.size() are filled
 * from a label plane: those two are all the function reads of it */
void ref_interpolate_with_superpixels(const float *src, const int32_t *labels, int n_labels, float *dst, int rows, int cols,
                                      int use_superpixel)
{
    refbuild::Quiet q;
    Slic slic;
    slic.clusters.assign((size_t)cols, std::vector<int>((size_t)rows, -1));
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r) slic.clusters[c][r] = labels[(size_t)r * cols + c];
    slic.centers.assign((size_t)n_labels, std::vector<double>(5, 0.0));
    slic.center_counts.assign((size_t)n_labels, 0);
    const cv::Mat in(rows, cols, CV_32F, (void *)src);
    cv::Mat out;
    interpolate_with_superpixels(slic, in, out, std::string("gaussian"), use_superpixel);
    copy_out(out, dst, rows, cols);
}

/* the stand-in's primitives on their own, so that a chain mismatch can be attributed (what = 0 dilate, 1 erode,
 * 2 medianBlur 5, 3 GaussianBlur 5x5 sigma 0; element: kr x kc bytes for 0 and 1) */
void ref_standin_primitive(int what, const float *src, float *dst, int rows, int cols, const uint8_t *element, int kr, int kc)
{
    const cv::Mat in(rows, cols, CV_32F, (void *)src);
    cv::Mat out;
    if (what == 0 || what == 1) {
        const cv::Mat el(kr, kc, CV_8UC1, (void *)element);
        if (what == 0) cv::dilate(in, out, el); else cv::erode(in, out, el);
    } else if (what == 2) {
        cv::medianBlur(in, out, 5);
    } else {
        cv::GaussianBlur(in, out, cv::Size(5, 5), 0);
    }
    copy_out(out, dst, rows, cols);
}

}  // extern "C"
