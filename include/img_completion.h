// img_completion.h -- the header the reference includes but does not ship
// (/root/reference/src/DC_lidar_only/img_completion.cpp:15, main.cpp:1, utils.cpp:3).
//
// Drop-in: with this file on the include path, and libdcmt_hip.so linked, the reference's
// mains (DC_lidar_only/main.cpp, DC_lidar_camera/main_lc.cpp, DC_stereo_lidar/main_sl*.cpp)
// compile unmodified apart from dropping their textual `#include ".../img_completion.cpp"` /
// `#include ".../img_completion_lc.cpp"` lines: the two functions below have the reference's
// exact signatures and semantics, and run on the GPU through the C ABI of dcmt.h.
//
//   void img_completion(const cv::Mat&, cv::Mat&, const bool&, const std::string&)
//        reference: src/DC_lidar_only/img_completion.cpp:17-20
//   void interpolate_with_superpixels(Slic&, const cv::Mat&, cv::Mat&, const std::string&, int)
//        reference: src/DC_lidar_camera/img_completion_lc.cpp:34-38   (define DCMT_WITH_SLIC
//        after including the reference's slic.h, or use the generic overload below)
//
// Header-only C++11.  Needs only cv::Mat from OpenCV (rows, cols, type(), step[0], ptr<float>(),
// create(), CV_32FC1): the tests compile it against a 60-line stand-in (tests/mock_opencv).
#ifndef IMG_COMPLETION_H
#define IMG_COMPLETION_H

#include <opencv2/opencv.hpp>

#include <cstdint>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "dcmt.h"

namespace dcmt_shim {

// One context per thread, grown on demand: the reference function is re-entrant and has no
// state, a dcmt_ctx must not be shared between threads.
struct ThreadCtx {
    dcmt_ctx* ctx = nullptr;
    int rows = 0, cols = 0;
    ~ThreadCtx() { dcmt_destroy(ctx); }
    dcmt_ctx* get(int r, int c)
    {
        if (!ctx || r > rows || c > cols) {
            dcmt_destroy(ctx);
            ctx = nullptr;
            rows = r > rows ? r : rows;
            cols = c > cols ? c : cols;
            const int st = dcmt_create(device(), rows, cols, 1, &ctx);
            if (st != DCMT_OK) throw std::runtime_error(std::string("dcmt_create: ") + dcmt_strerror(st));
        }
        return ctx;
    }
    static int& device() { static int d = 0; return d; }     // dcmt_shim::ThreadCtx::device() = k selects the GPU
};

// The reference prints while it works (img_completion.cpp:29 the dimensions, :50 "max range is", :161 one hole count per loop
// iteration; img_completion_lc.cpp:173 the hole counts only) and so does the drop-in; dcmt_shim::quiet() = true silences it.
inline bool& quiet() { static bool q = false; return q; }

inline ThreadCtx& thread_ctx()
{
    static thread_local ThreadCtx t;
    return t;
}

inline void check_input(const cv::Mat& m)
{
    // The reference reads at<float>(i,j) without checking: any other type is undefined behaviour
    // there; here it is an error.
    if (m.type() != CV_32FC1) throw std::runtime_error("img_completion: sparse image must be CV_32FC1");
    if (m.rows < 1 || m.cols < 1) throw std::runtime_error("img_completion: empty image");
}

inline int blur_from_string(const std::string& blur_type)
{
    if (blur_type == "gaussian") return DCMT_BLUR_GAUSSIAN;   // img_completion.cpp:176
    if (blur_type == "bilateral") return DCMT_BLUR_BILATERAL; // :172 -- cv::bilateralFilter in place throws; so do we
    if (blur_type == "bilateral_clone") return DCMT_BLUR_BILATERAL_CLONE;   // this project's opt-in: :174 given a copy (dcmt.h)
    if (blur_type == "gaussian_valid") return DCMT_BLUR_GAUSSIAN_VALID;     // this project's opt-in: the Gaussian that ignores holes (dcmt.h)
    return DCMT_BLUR_NONE;                                    // any other string: no blur
}

inline void raise(int st, const char* what)
{
    // The reference's failure mode is a cv::Exception out of an OpenCV call; the closest here.
    if (st != DCMT_OK) throw std::runtime_error(std::string(what) + ": " + dcmt_strerror(st));
}

// Generic form of interpolate_with_superpixels: labels[col][row] exactly as Slic::clusters
// (reference slic.cpp:21-30 builds it column-major), n_labels = slic.centers.size().
inline void interpolate_with_labels(const std::vector<std::vector<int> >& clusters, int n_labels,
                                    const cv::Mat& sparse_r_img, cv::Mat& dense_r_img,
                                    const std::string& /*blur_type: unused by the reference, img_completion_lc.cpp:183*/,
                                    int use_superpixel, const double* normalize_range = nullptr /* {alpha, beta}: see below */,
                                    int flags = 0 /* more DCMT_FLAG_* bits */)
{
    check_input(sparse_r_img);
    const int rows = sparse_r_img.rows, cols = sparse_r_img.cols;
    std::vector<int32_t> lab((size_t)rows * cols, -1);
    if (use_superpixel) {
        if ((int)clusters.size() < cols) throw std::runtime_error("interpolate_with_superpixels: clusters smaller than the image");
        for (int j = 0; j < cols; ++j) {
            if ((int)clusters[j].size() < rows) throw std::runtime_error("interpolate_with_superpixels: clusters smaller than the image");
            for (int i = 0; i < rows; ++i) lab[(size_t)i * cols + j] = clusters[j][i];   // [col][row] -> row-major
        }
    }
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    dcmt_params p;
    dcmt_default_params(&p);
    p.flags |= flags;
    if (normalize_range) { p.flags |= DCMT_FLAG_NORMALIZE; p.norm_lo = (float)normalize_range[0]; p.norm_hi = (float)normalize_range[1]; }
    p.verbose = quiet() ? 0 : 2;                             // img_completion_lc.cpp:173
    const int st = dcmt_complete_labeled_f32(thread_ctx().get(rows, cols), sparse_r_img.ptr<float>(), sparse_r_img.step[0], 0,
                                             lab.data(), sizeof(int32_t) * (size_t)cols, 0, n_labels, out.ptr<float>(),
                                             out.step[0], 0, rows, cols, 1, &p, use_superpixel);
    raise(st, "interpolate_with_superpixels");
    dense_r_img = out;
}

// The stereo-lidar callers' two lines in one call (DC_stereo_lidar/main_sl.cpp:370 + :386):
//     cv::normalize(projected, normalized, alpha, beta, cv::NORM_MINMAX);  img_completion(normalized, dense, extr, blur);
// the min-max pass runs on the GPU in front of the cascade (DCMT_FLAG_NORMALIZE) and the normalised image is never
// materialised.  For the labeled variant (:523 + :540) pass normalize_range to interpolate_with_labels.
inline void img_completion_normalized(const cv::Mat& projected, cv::Mat& dense_r_img, double alpha, double beta,
                                      const bool& /*extr*/, const std::string& blur_type)
{
    check_input(projected);
    const int rows = projected.rows, cols = projected.cols;
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    dcmt_params p;
    dcmt_default_params(&p);
    p.blur = blur_from_string(blur_type);
    p.flags |= DCMT_FLAG_NORMALIZE;
    p.norm_lo = (float)alpha;
    p.norm_hi = (float)beta;
    p.verbose = quiet() ? 0 : 2;                             // (the reference's "max range is" would be that of the normalised image: beta)
    if (!quiet()) std::cout << "NUMERO ROWS, COLS: " << rows << " " << cols << std::endl << "max range is" << (float)(alpha > beta ? alpha : beta) << std::endl;
    const int st = dcmt_complete_f32(thread_ctx().get(rows, cols), projected.ptr<float>(), projected.step[0], 0,
                                     out.ptr<float>(), out.step[0], 0, rows, cols, 1, &p);
    raise(st, "img_completion_normalized");
    dense_r_img = out;
}

// The cascade without its extrapolation (DCMT_FLAG_NO_EXTRAPOLATE, dcmt.h: no column extension, no large fills -- the median, the
// blur and the final invert run on the plane the 7x7 fill left, and nothing is invented far from a measurement).  An opt-in of
// this project under a name of its own: the reference's `extr` argument is never read there, so img_completion() below keeps
// ignoring it.  Prints the reference's two header lines and no hole counts.
inline void img_completion_no_extrapolate(const cv::Mat& sparse_r_img, cv::Mat& dense_r_img, const std::string& blur_type)
{
    check_input(sparse_r_img);
    const int rows = sparse_r_img.rows, cols = sparse_r_img.cols;
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    dcmt_params p;
    dcmt_default_params(&p);
    p.blur = blur_from_string(blur_type);
    p.flags |= DCMT_FLAG_NO_EXTRAPOLATE;
    p.verbose = quiet() ? 0 : 1;
    const int st = dcmt_complete_f32(thread_ctx().get(rows, cols), sparse_r_img.ptr<float>(), sparse_r_img.step[0], 0,
                                     out.ptr<float>(), out.step[0], 0, rows, cols, 1, &p);
    raise(st, "img_completion_no_extrapolate");
    dense_r_img = out;
}

// ... and its labeled twin: interpolate_with_labels without the extrapolation (prints nothing)
inline void interpolate_with_labels_no_extrapolate(const std::vector<std::vector<int> >& clusters, int n_labels,
                                                   const cv::Mat& sparse_r_img, cv::Mat& dense_r_img, const std::string& blur_type,
                                                   int use_superpixel, const double* normalize_range = nullptr)
{
    interpolate_with_labels(clusters, n_labels, sparse_r_img, dense_r_img, blur_type, use_superpixel, normalize_range, DCMT_FLAG_NO_EXTRAPOLATE);
}

// ---- the steps either side of the path, on cv::Mat / std::vector like the reference's own code -----------------------

// DC_stereo_lidar/main_sl.cpp:478-520: velodyne points ([n][4] floats: x, y, z, reflectance, the .bin payload) through
// T (4x4) and P (3x4), both ROW-major, into a fresh CV_32FC1 image of rows x cols (0 = no point), like projected_depths.
inline void project_points(const float* xyzi, int n_points, const float T[16], const float P[12], int rows, int cols,
                           cv::Mat& projected_depths)
{
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    raise(dcmt_project_points(thread_ctx().get(rows, cols), xyzi, n_points, T, P, out.ptr<float>(), out.step[0], rows, cols),
          "project_points");
    projected_depths = out;
}

// Slic::generate_superpixels (DC_lidar_camera/slic.cpp:101-182) on the CV_8UC3 image the reference passes; fills `clusters`
// as Slic::clusters ([col][row]) and returns slic.centers.size().
inline int slic_labels(const cv::Mat& lab_image, int step, int nc, std::vector<std::vector<int> >& clusters)
{
    if (lab_image.type() != CV_8UC3 || lab_image.rows < 1 || lab_image.cols < 1) throw std::runtime_error("slic_labels: image must be CV_8UC3");
    const int rows = lab_image.rows, cols = lab_image.cols;
    std::vector<int32_t> lab((size_t)rows * cols);
    raise(dcmt_slic_labels(thread_ctx().get(rows, cols), lab_image.ptr<unsigned char>(), lab_image.step[0], rows, cols, step, nc,
                           lab.data(), nullptr), "slic_labels");
    clusters.assign(cols, std::vector<int>(rows));
    for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) clusters[j][i] = lab[(size_t)i * cols + j];
    return dcmt_slic_num_centers(rows, cols, step);
}

// slic.create_connectivity(lab_image) (DC_lidar_camera/main_lc.cpp:202, slic.cpp:186-254) with its result KEPT, as dcmt.h states it
// (dcmt_slic_connectivity): `clusters` ([col][row], as Slic::clusters) is relabelled in place so that every label is one 4-connected
// region, fragments below a quarter of a superpixel merged into a neighbour.  n_centers = slic.centers.size() (what slic_labels
// returns).  Returns the number of labels; every label is below max(1, that).  An opt-in: the reference drops this relabelling.
inline int slic_enforce_connectivity(std::vector<std::vector<int> >& clusters, int n_centers)
{
    const int cols = (int)clusters.size(), rows = cols > 0 ? (int)clusters[0].size() : 0;
    if (rows < 1) throw std::runtime_error("slic_enforce_connectivity: empty clusters");
    std::vector<int32_t> lab((size_t)rows * cols);
    for (int j = 0; j < cols; ++j) {
        if ((int)clusters[j].size() != rows) throw std::runtime_error("slic_enforce_connectivity: clusters is not rectangular");
        for (int i = 0; i < rows; ++i) lab[(size_t)i * cols + j] = clusters[j][i];   // [col][row] -> row-major
    }
    int32_t count = 0;
    const size_t row = sizeof(int32_t) * (size_t)cols;
    raise(dcmt_slic_connectivity(thread_ctx().get(rows, cols), lab.data(), row, rows, cols, n_centers, lab.data(), row, &count),
          "slic_enforce_connectivity");
    for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) clusters[j][i] = lab[(size_t)i * cols + j];
    return (int)count;
}

// `clusters` ([col][row], as Slic::clusters) as the row-major int32 plane the C ABI takes, checked against the image it belongs to
inline std::vector<int32_t> clusters_row_major(const std::vector<std::vector<int> >& clusters, const cv::Mat& image, const char* what)
{
    const int rows = image.rows, cols = image.cols;
    if (image.type() != CV_8UC3 || rows < 1 || cols < 1) throw std::runtime_error(std::string(what) + ": image must be CV_8UC3");
    if ((int)clusters.size() != cols) throw std::runtime_error(std::string(what) + ": clusters does not have the image's size");
    std::vector<int32_t> lab((size_t)rows * cols);
    for (int j = 0; j < cols; ++j) {
        if ((int)clusters[j].size() != rows) throw std::runtime_error(std::string(what) + ": clusters does not have the image's size");
        for (int i = 0; i < rows; ++i) lab[(size_t)i * cols + j] = clusters[j][i];
    }
    return lab;
}

// slic.display_contours(image, CV_RGB(200,0,0)) (DC_lidar_camera/main_lc.cpp:214, slic.cpp:337-384) as dcmt.h states it
// (dcmt_slic_contours): the contour pixels of `clusters` painted into `image` (CV_8UC3, in place) with (uchar)colour[0..2] = B, G, R.
// `colour` is anything indexable: cv::Scalar, cv::Vec3b, an array.
template <typename Colour>
inline void slic_display_contours(const std::vector<std::vector<int> >& clusters, cv::Mat& image, const Colour& colour)
{
    const std::vector<int32_t> lab = clusters_row_major(clusters, image, "slic_display_contours");
    const uint8_t bgr[3] = {(uint8_t)colour[0], (uint8_t)colour[1], (uint8_t)colour[2]};
    raise(dcmt_slic_contours(thread_ctx().get(image.rows, image.cols), lab.data(), sizeof(int32_t) * (size_t)image.cols, image.rows, image.cols,
                             image.ptr<unsigned char>(), image.step[0], bgr, nullptr, 0), "slic_display_contours");
}

// slic.colour_with_cluster_means(image) (slic.cpp:392-433) as dcmt.h states it (dcmt_slic_cluster_means): every pixel of `image`
// (CV_8UC3, in place) becomes the mean colour of its superpixel.  n_labels = slic.centers.size() (what slic_labels returns), or the
// count slic_enforce_connectivity returns for clusters that went through it; a label outside [0, n_labels) keeps its pixels.
inline void slic_colour_with_cluster_means(const std::vector<std::vector<int> >& clusters, cv::Mat& image, int n_labels)
{
    const std::vector<int32_t> lab = clusters_row_major(clusters, image, "slic_colour_with_cluster_means");
    raise(dcmt_slic_cluster_means(thread_ctx().get(image.rows, image.cols), lab.data(), sizeof(int32_t) * (size_t)image.cols, image.rows, image.cols,
                                  n_labels, image.ptr<unsigned char>(), image.step[0], nullptr), "slic_colour_with_cluster_means");
}

// DC_stereo_lidar/main_sl.cpp:1165-1246: get_initial_disparity + calculateMeasuementDerivatives + optimize_IG +
// retrieve_optimized_depth on the dense depth (CV_32FC1) and the two grey images (CV_8UC1).
inline void stereo_refine(const cv::Mat& dense_depth, const cv::Mat& left_gray, const cv::Mat& right_gray, cv::Mat& optimized_depth)
{
    check_input(dense_depth);
    const int rows = dense_depth.rows, cols = dense_depth.cols;
    if (left_gray.type() != CV_8UC1 || right_gray.type() != CV_8UC1 || left_gray.rows != rows || right_gray.rows != rows ||
        left_gray.cols != cols || right_gray.cols != cols) throw std::runtime_error("stereo_refine: grey images must be CV_8UC1 of the depth's size");
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    dcmt_stereo_params sp;
    dcmt_default_stereo_params(&sp);
    raise(dcmt_stereo_refine(thread_ctx().get(rows, cols), dense_depth.ptr<float>(), dense_depth.step[0], left_gray.ptr<unsigned char>(),
                             left_gray.step[0], right_gray.ptr<unsigned char>(), right_gray.step[0], out.ptr<float>(), out.step[0], rows, cols, &sp),
          "stereo_refine");
    optimized_depth = out;
}

// The mains' toColorImage (DC_lidar_only/main.cpp:6-14): normalize to [0, 1], convertTo CV_8UC1 * 255, applyColorMap JET.
// CV_32FC1 in, a fresh CV_8UC3 (B, G, R) out.  Not named toColorImage: the reference mains define that function themselves.
inline void to_color_image(const cv::Mat& r_img, cv::Mat& color_img)
{
    if (r_img.type() != CV_32FC1 || r_img.rows < 1 || r_img.cols < 1) throw std::runtime_error("to_color_image: image must be CV_32FC1");
    const int rows = r_img.rows, cols = r_img.cols;
    cv::Mat out;
    out.create(rows, cols, CV_8UC3);
    raise(dcmt_colorize(thread_ctx().get(rows, cols), r_img.ptr<float>(), r_img.step[0], rows, cols, out.ptr<unsigned char>(), out.step[0]),
          "to_color_image");
    color_img = out;
}

// cv::cvtColor(image, lab_image, cv::COLOR_BGR2Lab) on a camera frame (DC_lidar_camera/main_lc.cpp:183, DC_stereo_lidar/
// main_sl.cpp:439): CV_8UC3 (B, G, R) in, a fresh CV_8UC3 (L, a, b) out -- the image slic_labels takes.  The arithmetic is the
// library's statement of OpenCV's 8-bit fixed-point scheme (dcmt.h), not a call into OpenCV.
inline void bgr_to_lab(const cv::Mat& image, cv::Mat& lab_image)
{
    if (image.type() != CV_8UC3 || image.rows < 1 || image.cols < 1) throw std::runtime_error("bgr_to_lab: image must be CV_8UC3");
    const int rows = image.rows, cols = image.cols;
    cv::Mat out;
    out.create(rows, cols, CV_8UC3);
    raise(dcmt_bgr_convert(thread_ctx().get(rows, cols), image.ptr<unsigned char>(), image.step[0], rows, cols, out.ptr<unsigned char>(),
                           out.step[0], nullptr, 0), "bgr_to_lab");
    lab_image = out;
}

// cv::cvtColor(image, gray, cv::COLOR_BGR2GRAY) (main_sl.cpp:1167, :1171): CV_8UC3 in, a fresh CV_8UC1 out -- the images
// stereo_refine takes.
inline void bgr_to_gray(const cv::Mat& image, cv::Mat& gray)
{
    if (image.type() != CV_8UC3 || image.rows < 1 || image.cols < 1) throw std::runtime_error("bgr_to_gray: image must be CV_8UC3");
    const int rows = image.rows, cols = image.cols;
    cv::Mat out;
    out.create(rows, cols, CV_8UC1);
    raise(dcmt_bgr_convert(thread_ctx().get(rows, cols), image.ptr<unsigned char>(), image.step[0], rows, cols, nullptr, 0,
                           out.ptr<unsigned char>(), out.step[0]), "bgr_to_gray");
    gray = out;
}

// cv::GaussianBlur(src, dst, cv::Size(5, 5), 0) as DC_stereo_lidar/main_sl.cpp:1253 calls it on the refined depth (in place there:
// src and dst may be the same Mat).  CV_32FC1 in, a fresh CV_32FC1 out.
inline void gaussian_blur5(const cv::Mat& src, cv::Mat& dst)
{
    check_input(src);
    const int rows = src.rows, cols = src.cols;
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    raise(dcmt_gaussian5(thread_ctx().get(rows, cols), src.ptr<float>(), src.step[0], out.ptr<float>(), out.step[0], rows, cols),
          "gaussian_blur5");
    dst = out;
}

// The 5x5 Gaussian that ignores holes (dcmt_gaussian5_valid, dcmt.h's GV): a pixel >= valid_thresh becomes the average of its taps
// >= valid_thresh under the Gaussian's weights, every other pixel comes back as it is.  For planes with holes: the cascade without its
// extrapolation, a trust-masked plane, stereo depth.  src and dst may be the same Mat.  CV_32FC1 in, a fresh CV_32FC1 out.
inline void gaussian_blur5_valid(const cv::Mat& src, cv::Mat& dst, float valid_thresh = 0.1f)
{
    check_input(src);
    const int rows = src.rows, cols = src.cols;
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    raise(dcmt_gaussian5_valid(thread_ctx().get(rows, cols), src.ptr<float>(), src.step[0], out.ptr<float>(), out.step[0], rows, cols, valid_thresh),
          "gaussian_blur5_valid");
    dst = out;
}

// cv::bilateralFilter(src, dst, 5, sigma_color, sigma_space) as dcmt.h states it (dcmt_bilateral5): the edge-preserving alternative to
// gaussian_blur5; the defaults are the cascade's literals (img_completion.cpp:174).  src and dst may be the same Mat.  CV_32FC1 in,
// a fresh CV_32FC1 out.
inline void bilateral_filter5(const cv::Mat& src, cv::Mat& dst, float sigma_color = 1.5f, float sigma_space = 2.0f)
{
    check_input(src);
    const int rows = src.rows, cols = src.cols;
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    raise(dcmt_bilateral5(thread_ctx().get(rows, cols), src.ptr<float>(), src.step[0], out.ptr<float>(), out.step[0], rows, cols, sigma_color,
                          sigma_space),
          "bilateral_filter5");
    dst = out;
}

// get_initial_error (DC_stereo_lidar/main_sl.cpp:618-712, called at :1273 on the refined depth), its data: the CV_8UC1 error map the
// reference fills (:641-682) -- per pixel min(255, floor(sqrt(ssd))) of a (2 window)^2 window of the left image against the right image at
// the disparity the depth implies, as dcmt.h states it (dcmt_photo_error) -- returned instead of shown: error_map_show's cv::circle
// drawing, the imshow and the prints are not reproduced.  depth: CV_32FC1; left_gray, right_gray: CV_8UC1 of its size (the reference
// converts its BGR images itself, :625, :630: bgr_to_gray above).  params == nullptr: the reference's constants (:632-638).  stats, where
// given: valid pixels (the reference's row_cols), matches, pixels with error > 0 (its counts), the sum of the errors.
inline cv::Mat get_initial_error(const cv::Mat& depth, const cv::Mat& left_gray, const cv::Mat& right_gray,
                                 const dcmt_photo_error_params* params = nullptr, uint64_t* stats = nullptr)
{
    check_input(depth);
    const int rows = depth.rows, cols = depth.cols;
    if (left_gray.type() != CV_8UC1 || right_gray.type() != CV_8UC1 || left_gray.rows != rows || left_gray.cols != cols ||
        right_gray.rows != rows || right_gray.cols != cols)
        throw std::runtime_error("get_initial_error: the images must be CV_8UC1 of the depth's size");
    dcmt_photo_error_params def;
    dcmt_default_photo_error_params(&def);
    cv::Mat out;
    out.create(rows, cols, CV_8UC1);
    raise(dcmt_photo_error(thread_ctx().get(rows, cols), depth.ptr<float>(), depth.step[0], left_gray.ptr<unsigned char>(), left_gray.step[0],
                           right_gray.ptr<unsigned char>(), right_gray.step[0], rows, cols, params ? params : &def, out.ptr<unsigned char>(),
                           out.step[0], stats),
          "get_initial_error");
    return out;
}

// The "PERFORM STEREO MATCHING" block (DC_stereo_lidar/main_sl.cpp:1293-1339: cv::StereoSGBM::compute on the rectified grey pair), as the
// matcher dcmt.h states (dcmt_sgm): disp16 is CV_16SC1, the disparity in sixteenths of a pixel, -16 where there is none -- the convention
// of StereoSGBM's CV_16S output -- not OpenCV's own numerics.  left_gray, right_gray: CV_8UC1 of one size (bgr_to_gray above).
// params == nullptr: dcmt_default_sgm_params (64 disparities, :1306).
// OpenCV defines CV_16SC1 as a macro; against a cv::Mat stand-in without 16-bit elements the function is left out.
#ifdef CV_16SC1
inline void stereo_sgm(const cv::Mat& left_gray, const cv::Mat& right_gray, cv::Mat& disp16, const dcmt_sgm_params* params = nullptr)
{
    const int rows = left_gray.rows, cols = left_gray.cols;
    if (left_gray.empty() || left_gray.type() != CV_8UC1 || right_gray.type() != CV_8UC1 || right_gray.rows != rows || right_gray.cols != cols)
        throw std::runtime_error("stereo_sgm: the images must be CV_8UC1 of one size");
    dcmt_sgm_params def;
    dcmt_default_sgm_params(&def);
    cv::Mat out;
    out.create(rows, cols, CV_16SC1);
    raise(dcmt_sgm(thread_ctx().get(rows, cols), left_gray.ptr<unsigned char>(), left_gray.step[0], right_gray.ptr<unsigned char>(),
                   right_gray.step[0], rows, cols, params ? params : &def, out.ptr<int16_t>(), out.step[0], nullptr, 0),
          "stereo_sgm");
    disp16 = out;
}

// stereo_sgm with the number of aggregation paths (dcmt_sgm_paths): 4 is stereo_sgm itself, 8 adds the four diagonals, as the full
// mode of cv::StereoSGBM does; with 8 the library refuses p2 > 1800.  Anything else throws.
inline void stereo_sgm_paths(const cv::Mat& left_gray, const cv::Mat& right_gray, cv::Mat& disp16, int paths, const dcmt_sgm_params* params = nullptr)
{
    const int rows = left_gray.rows, cols = left_gray.cols;
    if (left_gray.empty() || left_gray.type() != CV_8UC1 || right_gray.type() != CV_8UC1 || right_gray.rows != rows || right_gray.cols != cols)
        throw std::runtime_error("stereo_sgm_paths: the images must be CV_8UC1 of one size");
    dcmt_sgm_params def;
    dcmt_default_sgm_params(&def);
    cv::Mat out;
    out.create(rows, cols, CV_16SC1);
    raise(dcmt_sgm_paths(thread_ctx().get(rows, cols), left_gray.ptr<unsigned char>(), left_gray.step[0], right_gray.ptr<unsigned char>(),
                         right_gray.step[0], rows, cols, params ? params : &def, out.ptr<int16_t>(), out.step[0], nullptr, 0, paths),
          "stereo_sgm_paths");
    disp16 = out;
}

// stereo_sgm_paths with a LiDAR guide (dcmt_sgm_guided): guide is CV_32FC1 of the images' size, the depth in the left camera in metres,
// 0 where there is none (project_points_nearest's plane, or a completed one).  A pixel whose depth gives a disparity h inside the
// range has min(guide_weight * |d - h|, guide_cap) added to its matching cost; the library refuses guide_weight outside 0..10000,
// guide_cap < 0 and p2 + guide_cap > 10000 (1800 with 8 paths).  Its Python defaults are 100 and 1000.  Anything refused throws.
inline void stereo_sgm_guided(const cv::Mat& left_gray, const cv::Mat& right_gray, const cv::Mat& guide, cv::Mat& disp16, int paths,
                              int guide_weight, int guide_cap, const dcmt_sgm_params* params = nullptr)
{
    const int rows = left_gray.rows, cols = left_gray.cols;
    if (left_gray.empty() || left_gray.type() != CV_8UC1 || right_gray.type() != CV_8UC1 || right_gray.rows != rows || right_gray.cols != cols)
        throw std::runtime_error("stereo_sgm_guided: the images must be CV_8UC1 of one size");
    if (guide.type() != CV_32FC1 || guide.rows != rows || guide.cols != cols)
        throw std::runtime_error("stereo_sgm_guided: the guide must be CV_32FC1 of the images' size");
    dcmt_sgm_params def;
    dcmt_default_sgm_params(&def);
    cv::Mat out;
    out.create(rows, cols, CV_16SC1);
    raise(dcmt_sgm_guided(thread_ctx().get(rows, cols), left_gray.ptr<unsigned char>(), left_gray.step[0], right_gray.ptr<unsigned char>(),
                          right_gray.step[0], guide.ptr<float>(), guide.step[0], rows, cols, params ? params : &def, out.ptr<int16_t>(),
                          out.step[0], nullptr, 0, paths, guide_weight, guide_cap),
          "stereo_sgm_guided");
    disp16 = out;
}

// stereo_sgm_guided with the matching cost (dcmt_sgm_cost): DCMT_SGM_COST_ABSDIFF is stereo_sgm_guided itself, DCMT_SGM_COST_CENSUS
// matches on 24-bit census codes (10 * the Hamming distance over the 5 x 5 block), which a difference in exposure, gain or vignetting
// between the two cameras does not disturb.  guide: as above, or an empty cv::Mat for none (guide_weight and guide_cap are then not
// looked at).  A cost other than the two throws, as does everything stereo_sgm_guided refuses.
inline void stereo_sgm_cost(const cv::Mat& left_gray, const cv::Mat& right_gray, const cv::Mat& guide, cv::Mat& disp16, int paths,
                            int guide_weight, int guide_cap, int cost, const dcmt_sgm_params* params = nullptr)
{
    const int rows = left_gray.rows, cols = left_gray.cols;
    if (left_gray.empty() || left_gray.type() != CV_8UC1 || right_gray.type() != CV_8UC1 || right_gray.rows != rows || right_gray.cols != cols)
        throw std::runtime_error("stereo_sgm_cost: the images must be CV_8UC1 of one size");
    const bool guided = !guide.empty();
    if (guided && (guide.type() != CV_32FC1 || guide.rows != rows || guide.cols != cols))
        throw std::runtime_error("stereo_sgm_cost: the guide must be CV_32FC1 of the images' size, or empty");
    dcmt_sgm_params def;
    dcmt_default_sgm_params(&def);
    cv::Mat out;
    out.create(rows, cols, CV_16SC1);
    raise(dcmt_sgm_cost(thread_ctx().get(rows, cols), left_gray.ptr<unsigned char>(), left_gray.step[0], right_gray.ptr<unsigned char>(),
                        right_gray.step[0], guided ? guide.ptr<float>() : nullptr, guided ? guide.step[0] : 0, rows, cols, params ? params : &def,
                        out.ptr<int16_t>(), out.step[0], nullptr, 0, paths, guide_weight, guide_cap, cost),
          "stereo_sgm_cost");
    disp16 = out;
}

// cv::filterSpeckles(disp16, new_val, max_size, max_diff) for a CV_16SC1 disparity map, its argument order, in place, as dcmt.h
// states it (dcmt_filter_speckles): what StereoSGBM runs on its output with ((minDisparity - 1) * 16, speckleWindowSize,
// 16 * speckleRange) -- (-16, 200, 32) for the reference's matcher (main_sl.cpp:1301-1302).  Arguments the C call refuses throw.
inline void filter_speckles(cv::Mat& disp16, int new_val, int max_size, int max_diff)
{
    if (disp16.empty() || disp16.type() != CV_16SC1) throw std::runtime_error("filter_speckles: the map must be CV_16SC1");
    const dcmt_speckle_params p = {max_size, max_diff, new_val};
    raise(dcmt_filter_speckles(thread_ctx().get(disp16.rows, disp16.cols), disp16.ptr<int16_t>(), disp16.step[0], disp16.ptr<int16_t>(),
                               disp16.step[0], nullptr, 0, disp16.rows, disp16.cols, &p, nullptr),
          "filter_speckles");
}
#endif

// reproject_pc_colors / reproject_pc (DC_stereo_lidar/main_sl.cpp:924-965, :887-922): the records of the ordered point cloud of a
// CV_32FC1 depth plane, one per pixel with depth > 0, row-major.  bgr: CV_8UC3 of the depth's size, or an empty Mat (then the
// fourth dword of every record is 1.0f).  params == nullptr: the reference's intrinsics (:927-930).
inline void depth_to_cloud(const cv::Mat& depth, const cv::Mat& bgr, std::vector<dcmt_cloud_point>& out, const dcmt_cloud_params* params = nullptr)
{
    check_input(depth);
    const int rows = depth.rows, cols = depth.cols;
    const bool colour = !bgr.empty();
    if (colour && (bgr.type() != CV_8UC3 || bgr.rows != rows || bgr.cols != cols))
        throw std::runtime_error("depth_to_cloud: colour image must be CV_8UC3 of the depth's size");
    dcmt_cloud_params def;
    dcmt_default_cloud_params(&def);
    out.resize((size_t)rows * cols);
    int64_t n = 0;
    raise(dcmt_depth_to_cloud(thread_ctx().get(rows, cols), depth.ptr<float>(), depth.step[0], colour ? bgr.ptr<unsigned char>() : nullptr,
                              colour ? bgr.step[0] : 0, rows, cols, params ? params : &def, out.data(), (int64_t)out.size(), &n),
          "depth_to_cloud");
    out.resize((size_t)n);
}

// One least-squares plane of inverse depth per superpixel through the returns that fall in it, as dcmt.h states it
// (dcmt_superpixel_planes): `clusters` [col][row] as Slic::clusters, n_labels = slic.centers.size() or the count
// slic_enforce_connectivity returns, sparse_r_img CV_32FC1 in metres with 0 = no return.  planes_img is overwritten with a fresh
// CV_32FC1 image: the returns, the planes over their labels, 0 where a label holds no return -- what interpolate_with_labels then
// takes as its sparse image.  params == nullptr: dcmt_default_planes_params; fits, where given, receives the n_labels records.
inline void fit_superpixel_planes(const std::vector<std::vector<int> >& clusters, int n_labels, const cv::Mat& sparse_r_img, cv::Mat& planes_img,
                                  const dcmt_planes_params* params = nullptr, std::vector<dcmt_plane_fit>* fits = nullptr)
{
    check_input(sparse_r_img);
    const int rows = sparse_r_img.rows, cols = sparse_r_img.cols;
    if ((int)clusters.size() != cols) throw std::runtime_error("fit_superpixel_planes: clusters does not have the image's size");
    std::vector<int32_t> lab((size_t)rows * cols);
    for (int j = 0; j < cols; ++j) {
        if ((int)clusters[j].size() != rows) throw std::runtime_error("fit_superpixel_planes: clusters does not have the image's size");
        for (int i = 0; i < rows; ++i) lab[(size_t)i * cols + j] = clusters[j][i];
    }
    dcmt_planes_params def;
    dcmt_default_planes_params(&def);
    if (fits) fits->assign(n_labels > 0 ? (size_t)n_labels : 0, dcmt_plane_fit());
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    raise(dcmt_superpixel_planes(thread_ctx().get(rows, cols), sparse_r_img.ptr<float>(), sparse_r_img.step[0], lab.data(), sizeof(int32_t) * (size_t)cols,
                                 rows, cols, n_labels, params ? params : &def, out.ptr<float>(), out.step[0], fits && n_labels > 0 ? fits->data() : nullptr),
          "fit_superpixel_planes");
    planes_img = out;
}

// The occlusion filter of projected LiDAR returns, as dcmt.h states it (dcmt_sparse_occlusion): sparse_r_img CV_32FC1 in metres with
// 0 = no return, as project_points leaves it; filtered_img is overwritten with a fresh CV_32FC1 image in which every return that a
// nearer return in the window shows to be hidden from the camera is 0 -- what img_completion, fit_superpixel_planes and the guided
// matcher then take.  params == nullptr: dcmt_default_occlusion_params.  Returns the number of returns removed.
inline unsigned filter_occluded_returns(const cv::Mat& sparse_r_img, cv::Mat& filtered_img, const dcmt_occlusion_params* params = nullptr)
{
    check_input(sparse_r_img);
    const int rows = sparse_r_img.rows, cols = sparse_r_img.cols;
    dcmt_occlusion_params def;
    dcmt_default_occlusion_params(&def);
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    uint32_t removed = 0;
    raise(dcmt_sparse_occlusion(thread_ctx().get(rows, cols), sparse_r_img.ptr<float>(), sparse_r_img.step[0], out.ptr<float>(), out.step[0], rows, cols,
                                params ? params : &def, &removed),
          "filter_occluded_returns");
    filtered_img = out;
    return removed;
}

// The support map of a sparse plane, as dcmt.h states it (dcmt_support_distance): sparse_r_img CV_32FC1 in metres; dist2_img is
// overwritten with a fresh CV_32FC1 image holding, for every pixel, the squared Euclidean distance to the nearest return where that
// is at most max_radius^2 (an integer, exact as a float) and 65535 everywhere else.  params == nullptr: dcmt_default_support_params
// (max_radius 9).  Returns the number of pixels beyond max_radius.
inline unsigned distance_to_returns(const cv::Mat& sparse_r_img, cv::Mat& dist2_img, const dcmt_support_params* params = nullptr)
{
    check_input(sparse_r_img);
    const int rows = sparse_r_img.rows, cols = sparse_r_img.cols;
    dcmt_support_params def;
    dcmt_default_support_params(&def);
    std::vector<uint16_t> d2((size_t)rows * cols);
    uint32_t beyond = 0;
    raise(dcmt_support_distance(thread_ctx().get(rows, cols), sparse_r_img.ptr<float>(), sparse_r_img.step[0], nullptr, 0, nullptr, 0, nullptr, 0, d2.data(),
                                sizeof(uint16_t) * (size_t)cols, rows, cols, params ? params : &def, &beyond),
          "distance_to_returns");
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) out.ptr<float>(i)[j] = (float)d2[(size_t)i * cols + j];
    dist2_img = out;
    return beyond;
}

// The trust mask of a dense plane (dcmt_support_distance): trusted_img is overwritten with a fresh CV_32FC1 image that holds
// dense_img where a return of sparse_r_img lies within max_radius and, beyond it, fallback_img -- the stereo matcher's depth, say --
// or 0 where fallback_img is null.  The pixels are copied bit for bit.  All images CV_32FC1 of one size.  params == nullptr:
// dcmt_default_support_params.  Returns the number of pixels beyond max_radius.
inline unsigned trust_mask(const cv::Mat& sparse_r_img, const cv::Mat& dense_img, cv::Mat& trusted_img, const cv::Mat* fallback_img = nullptr,
                           const dcmt_support_params* params = nullptr)
{
    check_input(sparse_r_img);
    const int rows = sparse_r_img.rows, cols = sparse_r_img.cols;
    if (dense_img.type() != CV_32FC1 || dense_img.rows != rows || dense_img.cols != cols)
        throw std::runtime_error("trust_mask: the dense image must be CV_32FC1 of the sparse image's size");
    if (fallback_img && (fallback_img->type() != CV_32FC1 || fallback_img->rows != rows || fallback_img->cols != cols))
        throw std::runtime_error("trust_mask: the fallback image must be CV_32FC1 of the sparse image's size");
    dcmt_support_params def;
    dcmt_default_support_params(&def);
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    uint32_t beyond = 0;
    raise(dcmt_support_distance(thread_ctx().get(rows, cols), sparse_r_img.ptr<float>(), sparse_r_img.step[0], dense_img.ptr<float>(), dense_img.step[0],
                                fallback_img ? fallback_img->ptr<float>() : nullptr, fallback_img ? fallback_img->step[0] : 0, out.ptr<float>(), out.step[0],
                                nullptr, 0, rows, cols, params ? params : &def, &beyond),
          "trust_mask");
    trusted_img = out;
    return beyond;
}

// The joint bilateral filter, as dcmt.h states it (dcmt_joint_bilateral): filled_img is overwritten with a fresh CV_32FC1 image in
// which every hole of depth_img (CV_32FC1, metres) that has measured depths around it whose pixels of guide_img (CV_8UC1 or CV_8UC3, of
// depth_img's size) look like its own holds their weighted mean; with DCMT_JOINT_SMOOTH among params->flags the valid pixels are
// smoothed the same way, else they keep their bytes.  params == nullptr: dcmt_default_joint_params; tables == nullptr:
// dcmt_make_joint_tables(params->radius, sigma_space, sigma_guide).  Returns the number of holes filled; *left: the holes that stay.
inline unsigned joint_bilateral_fill(const cv::Mat& depth_img, const cv::Mat& guide_img, cv::Mat& filled_img, const dcmt_joint_params* params = nullptr,
                                     const dcmt_joint_tables* tables = nullptr, double sigma_space = 3.0, double sigma_guide = 10.0, unsigned* left = nullptr)
{
    check_input(depth_img);
    const int rows = depth_img.rows, cols = depth_img.cols;
    if ((guide_img.type() != CV_8UC1 && guide_img.type() != CV_8UC3) || guide_img.rows != rows || guide_img.cols != cols)
        throw std::runtime_error("joint_bilateral_fill: the guide must be CV_8UC1 or CV_8UC3 of the depth image's size");
    dcmt_joint_params def;
    dcmt_default_joint_params(&def);
    const dcmt_joint_params* p = params ? params : &def;
    dcmt_joint_tables own;
    if (!tables) raise(dcmt_make_joint_tables(p->radius, sigma_space, sigma_guide, &own), "joint_bilateral_fill");
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    uint32_t counts[2] = {0, 0};
    raise(dcmt_joint_bilateral(thread_ctx().get(rows, cols), depth_img.ptr<float>(), depth_img.step[0], guide_img.ptr<unsigned char>(), guide_img.step[0],
                               guide_img.type() == CV_8UC3 ? 3 : 1, tables ? tables : &own, out.ptr<float>(), out.step[0], rows, cols, p, counts),
          "joint_bilateral_fill");
    filled_img = out;
    if (left) *left = counts[1];
    return counts[0];
}

// The flying-pixel filter of a dense plane, as dcmt.h states it (dcmt_depth_normals): filtered_img is overwritten with a fresh CV_32FC1
// image in which every pixel of depth_img (CV_32FC1, metres) whose local plane passes closer to the camera centre than
// params->min_plane_dist is 0 -- the veil a blur strings between an object and what lies behind it -- and every other pixel keeps its
// bytes.  cloud == nullptr: dcmt_default_cloud_params, the intrinsics reproject_pc_colors uses; params == nullptr:
// dcmt_default_normals_params.  normals, where given, receives the rows * cols records of depth_normals below (of the INPUT plane).
// Returns the number of pixels removed.  It belongs between the blur and reproject_pc_colors.
inline unsigned filter_flying_pixels(const cv::Mat& depth_img, cv::Mat& filtered_img, const dcmt_cloud_params* cloud = nullptr,
                                     const dcmt_normals_params* params = nullptr, std::vector<dcmt_normal>* normals = nullptr)
{
    check_input(depth_img);
    const int rows = depth_img.rows, cols = depth_img.cols;
    dcmt_cloud_params cdef;
    dcmt_default_cloud_params(&cdef);
    dcmt_normals_params def;
    dcmt_default_normals_params(&def);
    if (normals) normals->assign((size_t)rows * cols, dcmt_normal());
    cv::Mat out;
    out.create(rows, cols, CV_32FC1);
    uint32_t counts[2] = {0, 0};
    raise(dcmt_depth_normals(thread_ctx().get(rows, cols), depth_img.ptr<float>(), depth_img.step[0], rows, cols, cloud ? cloud : &cdef, params ? params : &def,
                             normals ? normals->data() : nullptr, sizeof(dcmt_normal) * (size_t)cols, out.ptr<float>(), out.step[0], counts),
          "filter_flying_pixels");
    filtered_img = out;
    return counts[0];
}

// The surface normals of a dense plane (dcmt_depth_normals): normals is overwritten with rows * cols records, row-major -- the unit
// normal towards the camera and the distance of the pixel's local plane from the camera centre; four zeros on a hole and where no
// normal is defined.  The records of the pixels with depth > 0, in this order, are the normals of reproject_pc_colors' points.
// cloud, params: as above.  Returns the number of valid pixels without a normal.
inline unsigned depth_normals(const cv::Mat& depth_img, std::vector<dcmt_normal>& normals, const dcmt_cloud_params* cloud = nullptr,
                              const dcmt_normals_params* params = nullptr)
{
    check_input(depth_img);
    const int rows = depth_img.rows, cols = depth_img.cols;
    dcmt_cloud_params cdef;
    dcmt_default_cloud_params(&cdef);
    dcmt_normals_params def;
    dcmt_default_normals_params(&def);
    normals.assign((size_t)rows * cols, dcmt_normal());
    uint32_t counts[2] = {0, 0};
    raise(dcmt_depth_normals(thread_ctx().get(rows, cols), depth_img.ptr<float>(), depth_img.step[0], rows, cols, cloud ? cloud : &cdef, params ? params : &def,
                             normals.data(), sizeof(dcmt_normal) * (size_t)cols, nullptr, 0, counts),
          "depth_normals");
    return counts[1];
}

// unrectify_sol (DC_stereo_lidar/main_sl.cpp:967-1028, called at :1228) without its cv::circle / imshow / std::cout lines, so it
// takes no image: depth (CV_32FC1) forward-warped into depth_unrect, which the caller has sized (CV_32FC1, as at :1227) and which is
// overwritten completely -- 0 where nothing lands.  Minv: the 4x4 matrix that is applied, ROW-major: the inverse of the R_rect the
// reference passes (it calls Eigen's R_rect.inverse() inside its loop; that f32 inverse is not reproduced here, pass your own).
// Intrinsics and camera matrix: the reference's (:969-976).
inline void unrectify_sol_with(decltype(&dcmt_reproject_depth) call, const char* what, const cv::Mat& depth, cv::Mat& depth_unrect, const float Minv[16])
{
    check_input(depth);
    if (depth_unrect.type() != CV_32FC1 || depth_unrect.rows < 1 || depth_unrect.cols < 1)
        throw std::runtime_error(std::string(what) + ": the destination must be a pre-sized CV_32FC1 image");
    const int rows = depth.rows, cols = depth.cols, orows = depth_unrect.rows, ocols = depth_unrect.cols;
    dcmt_reproject_params p;
    dcmt_default_reproject_params(&p);
    for (int i = 0; i < 16; ++i) p.M[i] = Minv[i];
    raise(call(thread_ctx().get(rows > orows ? rows : orows, cols > ocols ? cols : ocols), depth.ptr<float>(), depth.step[0],
               rows, cols, &p, depth_unrect.ptr<float>(), depth_unrect.step[0], orows, ocols),
          what);
}

inline void unrectify_sol(const cv::Mat& depth, cv::Mat& depth_unrect, const float Minv[16])
{
    unrectify_sol_with(dcmt_reproject_depth, "unrectify_sol", depth, depth_unrect, Minv);
}

// The same warp as a z-buffer: a destination pixel several source pixels land on keeps the smallest new depth instead of the last in
// row-major order (dcmt_reproject_depth_nearest); the occupied pixels are the same.
inline void unrectify_sol_nearest(const cv::Mat& depth, cv::Mat& depth_unrect, const float Minv[16])
{
    unrectify_sol_with(dcmt_reproject_depth_nearest, "unrectify_sol_nearest", depth, depth_unrect, Minv);
}

// rectify() of DC_stereo_lidar/main_sl.cpp:1350-1381 for one camera, as dcmt.h states it (dcmt_rectify): cv::initUndistortRectifyMap
// on the record's K, D, R, P and cv::remap(..., cv::INTER_LINEAR) of `src` (CV_8UC1 or CV_8UC3) into a rows x cols `dst` of its type;
// samples outside the source are 0.
inline void undistort_rectify(const cv::Mat& src, cv::Mat& dst, const dcmt_rectify_calib& calib, int rows, int cols)
{
    if ((src.type() != CV_8UC1 && src.type() != CV_8UC3) || src.rows < 1 || src.cols < 1)
        throw std::runtime_error("undistort_rectify: image must be CV_8UC1 or CV_8UC3");
    if (rows < 1 || cols < 1) throw std::runtime_error("undistort_rectify: empty output");
    cv::Mat out;
    out.create(rows, cols, src.type());
    raise(dcmt_rectify(thread_ctx().get(rows, cols), src.ptr<unsigned char>(), src.step[0], src.rows, src.cols, src.type() == CV_8UC3 ? 3 : 1,
                       &calib, out.ptr<unsigned char>(), out.step[0], rows, cols),
          "undistort_rectify");
    dst = out;
}

}  // namespace dcmt_shim

// reference: src/DC_lidar_only/img_completion.cpp:17-20.  `extr` is accepted and ignored, as there (the cascade without its
// extrapolation is dcmt_shim::img_completion_no_extrapolate).
inline void img_completion(const cv::Mat& sparse_r_img, cv::Mat& dense_r_img, const bool& /*extr*/, const std::string& blur_type)
{
    dcmt_shim::check_input(sparse_r_img);
    const int rows = sparse_r_img.rows, cols = sparse_r_img.cols;
    cv::Mat out;                              // the reference overwrites dense_r_img with a fresh clone (:27)
    out.create(rows, cols, CV_32FC1);
    dcmt_params p;
    dcmt_default_params(&p);
    p.blur = dcmt_shim::blur_from_string(blur_type);
    p.verbose = dcmt_shim::quiet() ? 0 : 1;   // :29, :50, :161 -- printed by the library (stdout)
    const int st = dcmt_complete_f32(dcmt_shim::thread_ctx().get(rows, cols), sparse_r_img.ptr<float>(), sparse_r_img.step[0], 0,
                                     out.ptr<float>(), out.step[0], 0, rows, cols, 1, &p);
    dcmt_shim::raise(st, "img_completion");
    dense_r_img = out;
}

#ifdef DCMT_WITH_SLIC
// reference: src/DC_lidar_camera/img_completion_lc.cpp:34-38 (include the reference's slic.h first)
inline void interpolate_with_superpixels(Slic& slic, const cv::Mat& sparse_r_img, cv::Mat& dense_r_img,
                                         const std::string& blur_type, int use_superpixel)
{
    dcmt_shim::interpolate_with_labels(slic.clusters, (int)slic.centers.size(), sparse_r_img, dense_r_img, blur_type, use_superpixel);
}
#endif

#endif  // IMG_COMPLETION_H
