/* C ABI over the reference functions that live in files which cannot be compiled whole (they need PCL, Eigen, image
 * I/O): build_ref.py cuts each function out by signature and brace matching into the *.inc files included below,
 * at build time, next to the library.  Two of them share one name, so every cut sits in a namespace of its own.
 * ref_stereo sets up what the reference's stereo main sets up around its functions: two images of
 * CV_32FC(sizeof(EntryType)) whose entries carry the grey value and a zero derivative, a zero disparity plane, the two
 * derivative passes, the initial disparity, the depth before the sweeps, the sweeps, the depth after.
 * TEST INFRASTRUCTURE. */
#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include <opencv2/opencv.hpp>
#include <Eigen/Dense>
#include "quiet.h"

namespace ref_lo {
#include "eval_lo.inc"
}
namespace ref_lc {
#include "eval_lc.inc"
}
namespace ref_sl {
#include "stereo_sl.inc"
}

static_assert(sizeof(ref_sl::EntryType) == 12, "EntryType must be three floats, as with the real Eigen::Vector2f");

namespace {
cv::Mat entry_image(const uint8_t *grey, int rows, int cols)
{
    cv::Mat m(rows, cols, CV_32FC(sizeof(ref_sl::EntryType)));
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            ref_sl::EntryType &e = m.at<ref_sl::EntryType>(r, c);
            e.value = (float)grey[(size_t)r * cols + c];
            e.derivative.x() = 0.0f;
            e.derivative.y() = 0.0f;
        }
    return m;
}
void copy_out(const cv::Mat &m, float *dst, int rows, int cols)
{
    for (int r = 0; r < rows; ++r) std::memcpy(dst + (size_t)r * cols, &m.at<float>(r, 0), sizeof(float) * (size_t)cols);
}
}  // namespace

extern "C" {

/* depth f32, left / right grey uint8, all [rows][cols]; pre = depth from the initial disparity, post = after the sweeps */
void ref_stereo(const float *depth, const uint8_t *left, const uint8_t *right, float *pre, float *post, int rows, int cols)
{
    refbuild::Quiet q;
    cv::Mat el = entry_image(left, rows, cols), er = entry_image(right, rows, cols);
    cv::Mat dense(rows, cols, CV_32F, (void *)depth);
    cv::Mat disparity = cv::Mat::zeros(rows, cols, CV_32F);
    ref_sl::calculateMeasuementDerivatives(el);
    ref_sl::calculateMeasuementDerivatives(er);
    ref_sl::get_initial_disparity(dense, disparity);
    cv::Mat before = cv::Mat::zeros(rows, cols, CV_32F);
    ref_sl::retrieve_optimized_depth(disparity, before);
    copy_out(before, pre, rows, cols);
    ref_sl::optimize_IG(el, er, disparity);
    cv::Mat after = cv::Mat::zeros(rows, cols, CV_32F);
    ref_sl::retrieve_optimized_depth(disparity, after);
    copy_out(after, post, rows, cols);
}

void ref_evaluate_lo(const float *gt, const float *pred, int rows, int cols, float *out1)
{
    refbuild::Quiet q;
    const cv::Mat g(rows, cols, CV_32F, (void *)gt), p(rows, cols, CV_32F, (void *)pred);
    ref_lo::evaluate_performance(g, p, out1[0]);
}

void ref_evaluate_lc(const float *gt, const float *pred, int rows, int cols, float *out2)
{
    refbuild::Quiet q;
    const cv::Mat g(rows, cols, CV_32F, (void *)gt), p(rows, cols, CV_32F, (void *)pred);
    ref_lc::evaluate_performance(g, p, out2[0], out2[1]);
}

void ref_evaluate_sl(const float *gt, const float *pred, int rows, int cols, float *out2)
{
    refbuild::Quiet q;
    cv::Mat g(rows, cols, CV_32F, (void *)gt), p(rows, cols, CV_32F, (void *)pred);
    ref_sl::evaluate_performances(g, p, out2[0], out2[1]);
}

}  // extern "C"
