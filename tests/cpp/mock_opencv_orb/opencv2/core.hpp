// tests/cpp/mock_opencv_orb/opencv2/core.hpp -- the OpenCV mock of tests/cpp/mock_opencv_features plus cv::noArray(), the one
// name the descriptor call site (computeDescriptor(image, cv::noArray(), kpts2d, true, desc), main.cpp:246-248) adds. Test
// infrastructure only; it pins nothing about OpenCV's arithmetic.
#ifndef SBM_MOCK_OPENCV_ORB_CORE_HPP_
#define SBM_MOCK_OPENCV_ORB_CORE_HPP_

#include "../../mock_opencv_features/opencv2/core.hpp"

namespace cv {

inline InputArray noArray() {
  static Mat empty;
  static _InputArray a(empty);
  return a;
}

}  // namespace cv

#endif  // SBM_MOCK_OPENCV_ORB_CORE_HPP_
