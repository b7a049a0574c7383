/*
 * Stand-in for <opencv2/opencv.hpp>, written from OpenCV's documented interface so that the
 * reference's own translation units compile unmodified on a machine without OpenCV
 * (oracle/refbuild/build_ref.py).  TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * It declares OpenCV's names and nothing of the reference's.  The five image primitives the reference
 * reaches (dilate, erode, morphologyEx(MORPH_CLOSE), medianBlur(5), GaussianBlur(5x5, 0)) are
 * written as their definitions -- a loop over the window per pixel -- and share no code, header or
 * algorithm with oracle/dcmt_oracle.c: they are a third implementation next to the oracle and the
 * numpy twin, checked against the oracle primitive by primitive in tests/test_reference_parity.py.
 * They are still a reading of OpenCV's documentation, never diffed against a running OpenCV.
 *
 * Two deliberate differences from a real cv::Mat, both only visible to code that reads memory it
 * never wrote: an allocation is zero-filled, and it carries one extra zero row behind the last one
 * (the reference's stereo refinement reads row `rows` with weight 0 on the last image row).
 */
#ifndef DCMT_REFBUILD_OPENCV_HPP
#define DCMT_REFBUILD_OPENCV_HPP

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

typedef unsigned char uchar;

#define CV_8U 0
#define CV_8S 1
#define CV_16U 2
#define CV_16S 3
#define CV_32S 4
#define CV_32F 5
#define CV_64F 6
#define CV_CN_SHIFT 3
#define CV_MAT_DEPTH(t) ((t) & ((1 << CV_CN_SHIFT) - 1))
#define CV_MAT_CN(t) ((((t) >> CV_CN_SHIFT) & 511) + 1)
#define CV_MAKETYPE(depth, cn) (CV_MAT_DEPTH(depth) + (((cn) - 1) << CV_CN_SHIFT))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_8UC3 CV_MAKETYPE(CV_8U, 3)
#define CV_8UC(n) CV_MAKETYPE(CV_8U, (n))
#define CV_32FC1 CV_MAKETYPE(CV_32F, 1)
#define CV_32FC(n) CV_MAKETYPE(CV_32F, (n))
#define CV_RGB(r, g, b) cv::Scalar((b), (g), (r), 0)

namespace cv {

typedef ::uchar uchar;

[[noreturn]] inline void standin_abort(const char *what)
{
    std::fprintf(stderr, "opencv stand-in: %s is not implemented (the reference was not expected to reach it)\n", what);
    std::abort();
}

template <typename T> struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T x_, T y_) : x(x_), y(y_) {}
};
typedef Point_<int> Point;

template <typename T> struct Size_ {
    T width, height;
    Size_() : width(0), height(0) {}
    Size_(T w, T h) : width(w), height(h) {}
};
typedef Size_<int> Size;

template <typename T, int N> struct Vec {
    T val[N];
    Vec() { for (int i = 0; i < N; ++i) val[i] = T(); }
    Vec(T a, T b, T c) { static_assert(N == 3, "three-element constructor"); val[0] = a; val[1] = b; val[2] = c; }
    T &operator[](int i) { return val[i]; }
    const T &operator[](int i) const { return val[i]; }
};
typedef Vec<uchar, 3> Vec3b;

struct Scalar {
    double val[4];
    Scalar() { val[0] = val[1] = val[2] = val[3] = 0; }
    Scalar(double a, double b = 0, double c = 0, double d = 0) { val[0] = a; val[1] = b; val[2] = c; val[3] = d; }
    static Scalar all(double v) { return Scalar(v, v, v, v); }
    double &operator[](int i) { return val[i]; }
    const double &operator[](int i) const { return val[i]; }
};

class Mat {
public:
    int rows, cols;
    uchar *data;
    size_t step;                     /* bytes per row = elemSize() * cols: rows are dense */

    Mat() : rows(0), cols(0), data(nullptr), step(0), type_(0) {}
    Mat(int r, int c, int type) : Mat() { create(r, c, type); }
    Mat(int r, int c, int type, void *ext) : rows(r), cols(c), data((uchar *)ext), step(0), type_(type) { step = elemSize() * (size_t)c; }

    int type() const { return type_; }
    int depth() const { return CV_MAT_DEPTH(type_); }
    int channels() const { return CV_MAT_CN(type_); }
    size_t elemSize1() const
    {
        switch (depth()) { case CV_8U: case CV_8S: return 1; case CV_16U: case CV_16S: return 2; case CV_64F: return 8; default: return 4; }
    }
    size_t elemSize() const { return elemSize1() * (size_t)channels(); }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    Size size() const { return Size(cols, rows); }

    /* (re)allocates unless the shape and type already match, as Mat::create does; returns whether it did */
    bool create(int r, int c, int type)
    {
        if (data && r == rows && c == cols && type == type_) return false;
        rows = r; cols = c; type_ = type;
        step = elemSize() * (size_t)c;
        const size_t bytes = step * ((size_t)r + 1);
        own_.reset(new uchar[bytes ? bytes : 1](), std::default_delete<uchar[]>());
        data = own_.get();
        return true;
    }

    /* the address is row * step + col * sizeof(T), whatever the matrix's own element type is */
    template <typename T> T &at(int r, int c) { return *(T *)(data + (size_t)r * step + (size_t)c * sizeof(T)); }
    template <typename T> const T &at(int r, int c) const { return *(const T *)(data + (size_t)r * step + (size_t)c * sizeof(T)); }

    Mat clone() const
    {
        Mat m;
        if (!data) return m;
        m.create(rows, cols, type_);
        std::memcpy(m.data, data, step * (size_t)rows);
        return m;
    }
    void copyTo(Mat &dst) const
    {
        if (dst.data == data && dst.rows == rows && dst.cols == cols) return;
        Mat m = clone();
        dst = m;
    }
    /* masked copy: a destination that has to be reallocated starts as zeros; elements whose mask byte is 0 stay */
    void copyTo(Mat &dst, const Mat &mask) const
    {
        if (mask.type() != CV_8UC1 || mask.rows != rows || mask.cols != cols) standin_abort("copyTo with a mask of another shape or type");
        dst.create(rows, cols, type_);            /* create() zero-fills what it allocates */
        const size_t es = elemSize();
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c)
                if (mask.at<uchar>(r, c)) std::memcpy(dst.data + (size_t)r * dst.step + (size_t)c * es, data + (size_t)r * step + (size_t)c * es, es);
    }
    void convertTo(Mat &, int, double = 1, double = 0) const { standin_abort("Mat::convertTo"); }

    static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }
    static Mat ones(int r, int c, int type)
    {
        Mat m(r, c, type);
        if (type != CV_8UC1) standin_abort("Mat::ones of a type other than CV_8UC1");
        std::memset(m.data, 1, m.step * (size_t)r);
        return m;
    }

private:
    int type_;
    std::shared_ptr<uchar> own_;
};

typedef const Mat &InputArray;
typedef Mat &OutputArray;
typedef Mat &InputOutputArray;

enum { MORPH_ERODE = 0, MORPH_DILATE = 1, MORPH_OPEN = 2, MORPH_CLOSE = 3 };
enum { NORM_MINMAX = 32 };
enum { COLORMAP_JET = 2 };
enum { COLOR_BGR2GRAY = 6, COLOR_BGR2Lab = 44 };
enum { IMREAD_ANYDEPTH = 2, IMREAD_COLOR = 1 };
enum { INTER_LINEAR = 1 };

/* ---- morphology: the definition.  dst(r, c) = max (min) of src(r + kr - ar, c + kc - ac) over the element's
 * non-zero positions (kr, kc), anchor at the element's centre, the element not mirrored.  Positions outside the
 * image do not take part: the default border value is the lowest (highest) finite float, which is also what the
 * running extreme starts from.  std::max / std::min semantics: the later operand wins only if strictly larger
 * (smaller). */
inline void morph_definition(const Mat &src, Mat &dst, const Mat &element, bool is_dilate)
{
    if (src.type() != CV_32FC1) standin_abort("morphology on a type other than CV_32FC1");
    if (element.type() != CV_8UC1 || element.empty()) standin_abort("morphology with an element that is not a non-empty CV_8UC1");
    const int ar = element.rows / 2, ac = element.cols / 2;
    const float start = is_dilate ? -FLT_MAX : FLT_MAX;
    Mat out(src.rows, src.cols, src.type());
    for (int r = 0; r < src.rows; ++r)
        for (int c = 0; c < src.cols; ++c) out.at<float>(r, c) = start;
    /* one element position at a time over the whole image (every pixel still meets the positions in row-major
     * element order); the loops only visit pixels whose source position lies inside the image */
    for (int kr = 0; kr < element.rows; ++kr)
        for (int kc = 0; kc < element.cols; ++kc) {
            if (!element.at<uchar>(kr, kc)) continue;
            const int dr = kr - ar, dc = kc - ac;
            const int r_lo = std::max(0, -dr), r_hi = std::min(src.rows, src.rows - dr);
            const int c_lo = std::max(0, -dc), c_hi = std::min(src.cols, src.cols - dc);
            for (int r = r_lo; r < r_hi; ++r) {
                float *o = &out.at<float>(r, 0);
                const float *s = &src.at<float>(r + dr, 0);
                if (is_dilate) for (int c = c_lo; c < c_hi; ++c) o[c] = std::max(o[c], s[c + dc]);
                else for (int c = c_lo; c < c_hi; ++c) o[c] = std::min(o[c], s[c + dc]);
            }
        }
    dst = out;
}

inline void dilate(InputArray src, OutputArray dst, InputArray kernel) { morph_definition(src, dst, kernel, true); }
inline void erode(InputArray src, OutputArray dst, InputArray kernel) { morph_definition(src, dst, kernel, false); }

inline void morphologyEx(InputArray src, OutputArray dst, int op, InputArray kernel)
{
    Mat tmp;
    switch (op) {
    case MORPH_ERODE: erode(src, dst, kernel); break;
    case MORPH_DILATE: dilate(src, dst, kernel); break;
    case MORPH_OPEN: erode(src, tmp, kernel); dilate(tmp, dst, kernel); break;
    case MORPH_CLOSE: dilate(src, tmp, kernel); erode(tmp, dst, kernel); break;
    default: standin_abort("morphologyEx with this operation");
    }
}

/* ---- medianBlur, ksize 5, CV_32F: the 13th smallest of the 25 window values, the window clamped to the image
 * (replicated border).  Gather, insertion sort, pick. */
inline void medianBlur(InputArray src, OutputArray dst, int ksize)
{
    if (ksize != 5 || src.type() != CV_32FC1) standin_abort("medianBlur other than ksize 5 on CV_32FC1");
    Mat out(src.rows, src.cols, src.type());
    for (int r = 0; r < src.rows; ++r)
        for (int c = 0; c < src.cols; ++c) {
            float w[25];
            int n = 0;
            for (int dr = -2; dr <= 2; ++dr)
                for (int dc = -2; dc <= 2; ++dc) {
                    const int rr = std::min(std::max(r + dr, 0), src.rows - 1), cc = std::min(std::max(c + dc, 0), src.cols - 1);
                    const float v = src.at<float>(rr, cc);
                    int p = n++;
                    while (p > 0 && v < w[p - 1]) { w[p] = w[p - 1]; --p; }
                    w[p] = v;
                }
            out.at<float>(r, c) = w[12];
        }
    dst = out;
}

/* ---- GaussianBlur(Size(5, 5), sigma 0), CV_32F: sigma <= 0 with ksize 5 selects the fixed kernel [1 4 6 4 1] / 16;
 * separable, rows first, then columns, f32 throughout, border reflected without repeating the edge pixel
 * (BORDER_REFLECT_101).  Each pass is the symmetric form centre * k0 + (pair at distance 1) * k1 + (pair at
 * distance 2) * k2, summed left to right, every operation rounded to f32 (the build forbids contraction). */
inline int reflect_101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

inline void GaussianBlur(InputArray src, OutputArray dst, Size ksize, double sigmaX, double sigmaY = 0)
{
    if (ksize.width != 5 || ksize.height != 5 || sigmaX != 0 || sigmaY != 0 || src.type() != CV_32FC1)
        standin_abort("GaussianBlur other than Size(5, 5), sigma 0 on CV_32FC1");
    const float k[3] = {6.0f / 16.0f, 4.0f / 16.0f, 1.0f / 16.0f};
    Mat hor(src.rows, src.cols, src.type()), out(src.rows, src.cols, src.type());
    for (int r = 0; r < src.rows; ++r)
        for (int c = 0; c < src.cols; ++c) {
            float acc = src.at<float>(r, c) * k[0];
            for (int d = 1; d <= 2; ++d) {
                const float pair = src.at<float>(r, reflect_101(c - d, src.cols)) + src.at<float>(r, reflect_101(c + d, src.cols));
                acc = acc + pair * k[d];
            }
            hor.at<float>(r, c) = acc;
        }
    for (int r = 0; r < src.rows; ++r)
        for (int c = 0; c < src.cols; ++c) {
            float acc = hor.at<float>(r, c) * k[0];
            for (int d = 1; d <= 2; ++d) {
                const float pair = hor.at<float>(reflect_101(r - d, src.rows), c) + hor.at<float>(reflect_101(r + d, src.rows), c);
                acc = acc + pair * k[d];
            }
            out.at<float>(r, c) = acc;
        }
    dst = out;
}

/* ---- named by the reference, never reached on the paths that are built: abort with a message ---- */
inline void bilateralFilter(InputArray, OutputArray, int, double, double) { standin_abort("bilateralFilter"); }
inline void normalize(InputArray, InputOutputArray, double = 1, double = 0, int = 4) { standin_abort("normalize"); }
inline void applyColorMap(InputArray, OutputArray, int) { standin_abort("applyColorMap"); }
inline void cvtColor(InputArray, OutputArray, int) { standin_abort("cvtColor"); }
inline Mat imread(const std::string &, int = 1) { standin_abort("imread"); }
inline bool imwrite(const std::string &, InputArray) { standin_abort("imwrite"); }
inline void imshow(const std::string &, InputArray) { standin_abort("imshow"); }
inline int waitKey(int = 0) { standin_abort("waitKey"); }
inline void vconcat(const std::vector<Mat> &, OutputArray) { standin_abort("vconcat"); }
inline void hconcat(const std::vector<Mat> &, OutputArray) { standin_abort("hconcat"); }
/* drawing is display only */
inline void circle(InputOutputArray, Point, int, const Scalar &, int = 1) {}

}  // namespace cv

#endif
