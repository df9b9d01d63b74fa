// tests/cpp/mock_opencv_match/opencv2/core.hpp -- the OpenCV mock of tests/cpp/mock_opencv_orb plus cv::Point3f, the one name the
// matching call site (matchingGuess's kptsFrom3D, Registration.cpp:250-303) adds. Test infrastructure only; it pins nothing about
// OpenCV's arithmetic.
#ifndef SBM_MOCK_OPENCV_MATCH_CORE_HPP_
#define SBM_MOCK_OPENCV_MATCH_CORE_HPP_

#include "../../mock_opencv_orb/opencv2/core.hpp"

namespace cv {

struct Point3f {
  float x = 0.f, y = 0.f, z = 0.f;
  Point3f() {}
  Point3f(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};

}  // namespace cv

#endif  // SBM_MOCK_OPENCV_MATCH_CORE_HPP_
