/* The header the reference's lidar-only sources include and do not ship: OpenCV, the streams, the entry point. */
#ifndef DCMT_REFBUILD_IMG_COMPLETION_H
#define DCMT_REFBUILD_IMG_COMPLETION_H
#include <opencv2/opencv.hpp>
#include <iostream>
#include <string>
void img_completion(const cv::Mat &, cv::Mat &, const bool &, const std::string &);
#endif
