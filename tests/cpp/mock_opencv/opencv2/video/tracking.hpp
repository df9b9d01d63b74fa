// tests/cpp/mock_opencv/opencv2/video/tracking.hpp -- the two flag values and the one function of OpenCV's video module that
// src/slam/src/opencv/CvLKStereo.cpp names.  MOCK, test infrastructure only, written from the names alone.
//
// cv::buildOpticalFlowPyramid is DECLARED here and computes nothing anywhere: oracle/lk_reference_driver.cpp defines it and
// hands back the padded levels and derivative planes it was given (see there).  The pyramid's arithmetic stays RECALLED.
#ifndef SBM_MOCK_OPENCV_VIDEO_TRACKING_HPP_
#define SBM_MOCK_OPENCV_VIDEO_TRACKING_HPP_

#include <vector>

#include "../core.hpp"

namespace cv {

enum { OPTFLOW_USE_INITIAL_FLOW = 4, OPTFLOW_LK_GET_MIN_EIGENVALS = 8 };

// Fills pyramid with the levels 0..k of img, each a rectangle inside a plane padded by winSize on every side, followed level by
// level by its two-channel int16 derivative plane when withDerivatives is set; returns k <= maxLevel.
int buildOpticalFlowPyramid(InputArray img, std::vector<Mat>& pyramid, Size winSize, int maxLevel, bool withDerivatives = true);

}  // namespace cv

#endif
