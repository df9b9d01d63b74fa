// sbm_lkstereo.hpp -- header-only C++ adaptor for the reference's sparse depth provider, DEPTH_METHOD_CV_LK (sbm.h,
// sbm_lk_*), so that the call
//
//     rightCorners = computeCorrespondences(data.imageLeft(), data.imageRight(), leftCorners, status);
//                                                                     // src/slam/src/core/Stereo.cpp:136 (Stereo.cpp:9-51)
//
// compiles against the MI355X engine unchanged once this header replaces Stereo.h's declaration. The
// reference-signature overload exists when OpenCV headers are present (SBM_HAVE_OPENCV, as in sbm_stereobm.hpp). The plain form
// takes raw strided frames and (x, y) pairs. Failures throw sbm::Error.
#ifndef SBM_LKSTEREO_HPP_
#define SBM_LKSTEREO_HPP_

#include <cstddef>
#include <cstdint>
#include <vector>

#include "sbm_stereobm.hpp"   // sbm::Error and the OpenCV detection

namespace sbm {

class LkStereo {
 public:
  // the reference's constants (15 x 3, 5 levels, 30 iterations, 0.01, min-eig 1e-4, 0.5 < d <= 128) unless p is given
  explicit LkStereo(int device = 0, const sbm_lk_params* p = nullptr) {
    if (p) p_ = *p; else sbm_lk_params_default(&p_);
    sbm_params bm;
    sbm_params_default(&bm, 0, 0);   // the handle's block-matcher parameters are not used by the tracker
    check(sbm_create(&h_, &bm, device));
  }
  ~LkStereo() { sbm_destroy(h_); }
  LkStereo(const LkStereo&) = delete;
  LkStereo& operator=(const LkStereo&) = delete;

  const sbm_lk_params& params() const { return p_; }
  void setParams(const sbm_lk_params& p) { p_ = p; }
  sbm_handle* handle() { return h_; }

  // One strided 8-bit pair (strides in bytes) and left = x0, y0, x1, y1, ... -> the right points in the same layout; status
  // gets one byte per point, err (may be null) the level-0 minimum eigenvalue per point.
  std::vector<float> correspondences(const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride, int width,
                                     int height, const std::vector<float>& left_xy, std::vector<unsigned char>& status,
                                     std::vector<float>* err = nullptr) {
    const int n = (int)(left_xy.size() / 2);
    std::vector<float> right_xy(2 * (size_t)n);
    status.assign((size_t)n, 0);
    if (err) err->assign((size_t)n, 0.f);
    check(sbm_lk_stereo(h_, left, left_stride, right, right_stride, width, height, left_xy.data(), n, &p_, right_xy.data(),
                        status.data(), err ? err->data() : nullptr));
    return right_xy;
  }

#ifdef SBM_HAVE_OPENCV
  // computeCorrespondences(leftImage, rightImage, leftCorners, status): CV_8UC1 frames of one size (any row step)
  std::vector<cv::Point2f> correspondences(const cv::Mat& leftImage, const cv::Mat& rightImage,
                                           const std::vector<cv::Point2f>& leftCorners, std::vector<unsigned char>& status) {
    if (leftImage.type() != CV_8UC1 || rightImage.type() != CV_8UC1) throw Error(SBM_ERR_SIZE, "the images must be CV_8UC1");
    if (leftImage.rows != rightImage.rows || leftImage.cols != rightImage.cols)
      throw Error(SBM_ERR_SIZE, "the images must have the same size");
    std::vector<float> xy(2 * leftCorners.size());
    for (size_t i = 0; i < leftCorners.size(); i++) { xy[2 * i] = leftCorners[i].x; xy[2 * i + 1] = leftCorners[i].y; }
    const std::vector<float> r = correspondences(leftImage.ptr<uint8_t>(0), (size_t)leftImage.step, rightImage.ptr<uint8_t>(0),
                                                 (size_t)rightImage.step, leftImage.cols, leftImage.rows, xy, status);
    std::vector<cv::Point2f> rightCorners(leftCorners.size());
    for (size_t i = 0; i < rightCorners.size(); i++) rightCorners[i] = cv::Point2f(r[2 * i], r[2 * i + 1]);
    return rightCorners;
  }
#endif

 private:
  static void check(int st) {
    if (st != SBM_OK) throw Error(st, sbm_strerror(st));
  }
  sbm_handle* h_ = nullptr;
  sbm_lk_params p_;
};

// One tracker per process on device 0, created at the first call (what the reference's free function needs).
inline LkStereo& default_lk_stereo() {
  static LkStereo s;
  return s;
}

inline std::vector<float> computeCorrespondences(const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride,
                                                 int width, int height, const std::vector<float>& left_xy,
                                                 std::vector<unsigned char>& status) {
  return default_lk_stereo().correspondences(left, left_stride, right, right_stride, width, height, left_xy, status);
}

#ifdef SBM_HAVE_OPENCV
inline std::vector<cv::Point2f> computeCorrespondences(const cv::Mat& leftImage, const cv::Mat& rightImage,
                                                       const std::vector<cv::Point2f>& leftCorners,
                                                       std::vector<unsigned char>& status) {
  return default_lk_stereo().correspondences(leftImage, rightImage, leftCorners, status);
}
#endif

}  // namespace sbm

#endif  // SBM_LKSTEREO_HPP_
