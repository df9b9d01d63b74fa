// tests/cpp/mock_opencv_features/opencv2/core.hpp -- the OpenCV mock of tests/cpp/mock_opencv plus the two feature types
// include/sbm_gftt.hpp's reference-signature overload uses (cv::Point2f, cv::KeyPoint). Test infrastructure only; written from
// the constructor the reference calls (cv::KeyPoint(pt, size), GFTT.cpp:166), with OpenCV's documented defaults for the other
// fields. It pins nothing about OpenCV's arithmetic.
#ifndef SBM_MOCK_OPENCV_FEATURES_CORE_HPP_
#define SBM_MOCK_OPENCV_FEATURES_CORE_HPP_

#include "../../mock_opencv/opencv2/core.hpp"

namespace cv {

struct Point2f {
  float x = 0.f, y = 0.f;
  Point2f() {}
  Point2f(float x_, float y_) : x(x_), y(y_) {}
};

struct KeyPoint {
  Point2f pt;
  float size = 0.f, angle = -1.f, response = 0.f;
  int octave = 0, class_id = -1;
  KeyPoint() {}
  KeyPoint(Point2f p, float s, float a = -1.f, float r = 0.f, int o = 0, int c = -1)
      : pt(p), size(s), angle(a), response(r), octave(o), class_id(c) {}
};

}  // namespace cv

#endif  // SBM_MOCK_OPENCV_FEATURES_CORE_HPP_
