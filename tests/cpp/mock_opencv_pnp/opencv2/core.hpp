// tests/cpp/mock_opencv_pnp/opencv2/core.hpp -- the OpenCV mock of the motion-estimation call site (estimateMotion3DTo2D's
// std::map<int, cv::Point3f> and std::map<int, cv::KeyPoint>, Registration.cpp:337-397): the matching mock's cv::Point3f,
// cv::Point2f and cv::KeyPoint are all it uses. Test infrastructure only; it pins nothing about OpenCV's arithmetic.
#ifndef SBM_MOCK_OPENCV_PNP_CORE_HPP_
#define SBM_MOCK_OPENCV_PNP_CORE_HPP_

#include "../../mock_opencv_match/opencv2/core.hpp"

#endif  // SBM_MOCK_OPENCV_PNP_CORE_HPP_
