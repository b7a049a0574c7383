// The cv::Mat stand-in of tests/mock_opencv/opencv2/opencv.hpp with one more element type, CV_16SC1, which dcmt_shim::stereo_sgm
// returns.  A file of its own, found first by tests/test_shim_sgm.py's include path, so that the stand-in the other shim tests build
// against stays what it is.  Written from OpenCV's documented interface; used ONLY to build this repo's own shim + test.
#pragma once
#include <cstddef>
#include <cstring>
#include <memory>

#define CV_8UC1 0
#define CV_16SC1 3
#define CV_32FC1 5
#define CV_8UC3 16

namespace cv {
class Mat {
public:
    int rows = 0, cols = 0;
    size_t step[2] = {0, 0};
    Mat() {}
    Mat(int r, int c, int type) { create(r, c, type); }
    // a view over caller memory with an explicit row step (bytes), like cv::Mat(rows, cols, type, data, step)
    Mat(int r, int c, int type, void* data, size_t row_step) : rows(r), cols(c), type_(type), data_((unsigned char*)data)
    {
        step[0] = row_step; step[1] = elem_size(type);
    }
    void create(int r, int c, int type)
    {
        if (r == rows && c == cols && type == type_ && buf_) return;
        rows = r; cols = c; type_ = type;
        step[1] = elem_size(type); step[0] = step[1] * (size_t)c;
        buf_.reset(new unsigned char[step[0] * (size_t)r], std::default_delete<unsigned char[]>());
        data_ = buf_.get();
    }
    int type() const { return type_; }
    bool empty() const { return rows == 0 || cols == 0; }
    template <typename T> T* ptr(int r = 0) { return (T*)(data_ + step[0] * (size_t)r); }
    template <typename T> const T* ptr(int r = 0) const { return (const T*)(data_ + step[0] * (size_t)r); }
    template <typename T> T& at(int r, int c) { return ptr<T>(r)[c]; }
    template <typename T> const T& at(int r, int c) const { return ptr<T>(r)[c]; }
private:
    static size_t elem_size(int type)
    {
        switch (type) {
        case CV_32FC1: return 4;
        case CV_8UC3: return 3;
        case CV_16SC1: return 2;
        default: return 1;
        }
    }
    int type_ = CV_32FC1;
    std::shared_ptr<unsigned char> buf_;     // ref-counted like cv::Mat
    unsigned char* data_ = nullptr;
};
}  // namespace cv
