// sbm_gftt.hpp -- header-only C++ adaptor for the keypoint selection of the reference's FPGA feature path (sbm.h,
// sbm_gftt_select*) and for the OpenCV detector of its CV_GFTT modes (sbm_gftt_cv*), so that the calls
//
//     generateKeypoints2(eig, maxEigen, kpts2d);          // src/slam/src/core/main.cpp:241-243 (GFTT.cpp:41-170)
//     generateKeypoints(imageLeft, kpts2d);               // src/slam/src/core/main.cpp:239     (GFTT.cpp:11-25)
//
// compile against the MI355X engine unchanged once this header replaces GFTT.h's declaration. The
// reference-signature overload exists when OpenCV headers are present (SBM_HAVE_OPENCV, as in sbm_stereobm.hpp); it fills
// cv::KeyPoint(pt, block_size) in acceptance order. The plain form takes a raw strided uint16 map and returns (x, y) pairs.
// Failures throw sbm::Error.
#ifndef SBM_GFTT_HPP_
#define SBM_GFTT_HPP_

#include <cstddef>
#include <cstdint>
#include <vector>

#include "sbm_stereobm.hpp"   // sbm::Error and the OpenCV detection

namespace sbm {

class GfttSelect {
 public:
  // the reference's constants (1500, 0.01, 7.0, 3) unless p is given; `device` selects the HIP device
  explicit GfttSelect(int device = 0, const sbm_gftt_select_params* p = nullptr) {
    if (p) p_ = *p; else sbm_gftt_select_params_default(&p_);
    sbm_params bm;
    sbm_params_default(&bm, 0, 0);   // the handle's block-matcher parameters are not used by the selection
    check(sbm_create(&h_, &bm, device));
  }
  ~GfttSelect() { sbm_destroy(h_); }
  GfttSelect(const GfttSelect&) = delete;
  GfttSelect& operator=(const GfttSelect&) = delete;

  const sbm_gftt_select_params& params() const { return p_; }
  void setParams(const sbm_gftt_select_params& p) { p_ = p; }
  sbm_handle* handle() { return h_; }

  // One strided uint16 map (stride in bytes) and its Max register -> xy = x0, y0, x1, y1, ... in acceptance order.
  void select(const uint16_t* eig, size_t eig_stride, int width, int height, unsigned short max_eig, std::vector<float>& xy) {
    const int vst = sbm_gftt_select_params_validate(&p_, width, height);
    if (vst != SBM_OK) check(vst);
    const size_t cap = p_.max_features > 0 ? (size_t)p_.max_features : (size_t)(width - 2) * (height - 2);
    xy.resize(2 * cap);
    int k = 0;
    check(sbm_gftt_select(h_, eig, eig_stride, width, height, max_eig, &p_, xy.data(), cap, &k));
    xy.resize(2 * (size_t)k);
  }

#ifdef SBM_HAVE_OPENCV
  // generateKeypoints2(eig, max, kpts2d): eig a CV_16UC1 map (any row step)
  void select(cv::Mat& eig, unsigned short max_eig, std::vector<cv::KeyPoint>& kpts2d) {
#ifndef SBM_MOCK_OPENCV
    if (eig.depth() != CV_16U || eig.channels() != 1) throw Error(SBM_ERR_SIZE, "eig must be CV_16UC1");
#endif
    std::vector<float> xy;
    select(eig.ptr<uint16_t>(0), (size_t)eig.step, eig.cols, eig.rows, max_eig, xy);
    kpts2d.resize(xy.size() / 2);
    for (size_t i = 0; i < kpts2d.size(); i++)
      kpts2d[i] = cv::KeyPoint(cv::Point2f(xy[2 * i], xy[2 * i + 1]), (float)p_.block_size);
  }
#endif

 private:
  static void check(int st) {
    if (st != SBM_OK) throw Error(st, sbm_strerror(st));
  }
  sbm_handle* h_ = nullptr;
  sbm_gftt_select_params p_;
};

// One selector per process on device 0, created at the first call (what the reference's free function needs).
inline GfttSelect& default_gftt_select() {
  static GfttSelect s;
  return s;
}

inline void generateKeypoints2(const uint16_t* eig, size_t eig_stride, int width, int height, unsigned short max_eig,
                               std::vector<float>& xy) {
  default_gftt_select().select(eig, eig_stride, width, height, max_eig, xy);
}

#ifdef SBM_HAVE_OPENCV
inline void generateKeypoints2(cv::Mat& eig, unsigned short max, std::vector<cv::KeyPoint>& kpts2d) {
  default_gftt_select().select(eig, max, kpts2d);
}
#endif

// ---- generateKeypoints(img, kpts2d): the OpenCV detector of the CV_GFTT modes (src/slam/src/core/main.cpp:239, GFTT.cpp:11-25;
// sbm.h, sbm_gftt_cv*) -- the frame goes in, cv::KeyPoint(pt, block_size) come out in acceptance order.
class GfttCv {
 public:
  // the reference's constants (1500, 0.01, 7.0, 3, false, 0.04) unless p is given; `device` selects the HIP device
  explicit GfttCv(int device = 0, const sbm_gftt_cv_params* p = nullptr) {
    if (p) p_ = *p; else sbm_gftt_cv_params_default(&p_);
    sbm_params bm;
    sbm_params_default(&bm, 0, 0);   // the handle's block-matcher parameters are not used by the detector
    check(sbm_create(&h_, &bm, device));
  }
  ~GfttCv() { sbm_destroy(h_); }
  GfttCv(const GfttCv&) = delete;
  GfttCv& operator=(const GfttCv&) = delete;

  const sbm_gftt_cv_params& params() const { return p_; }
  void setParams(const sbm_gftt_cv_params& p) { p_ = p; }
  sbm_handle* handle() { return h_; }

  // One strided 8-bit frame (stride in bytes) -> xy = x0, y0, x1, y1, ... in acceptance order.
  void detect(const uint8_t* img, size_t img_stride, int width, int height, std::vector<float>& xy) {
    const int vst = sbm_gftt_cv_params_validate(&p_, width, height);
    if (vst != SBM_OK) check(vst);
    const size_t cap = p_.max_features > 0 ? (size_t)p_.max_features : (size_t)(width - 2) * (height - 2);
    xy.resize(2 * cap);
    int k = 0;
    check(sbm_gftt_cv_detect(h_, img, img_stride, width, height, &p_, xy.data(), cap, &k));
    xy.resize(2 * (size_t)k);
  }

#ifdef SBM_HAVE_OPENCV
  // generateKeypoints(img, kpts2d): img a CV_8UC1 frame (any row step)
  void detect(cv::Mat& img, std::vector<cv::KeyPoint>& kpts2d) {
#ifndef SBM_MOCK_OPENCV
    if (img.depth() != CV_8U || img.channels() != 1) throw Error(SBM_ERR_SIZE, "img must be CV_8UC1");
#endif
    std::vector<float> xy;
    detect(img.ptr<uint8_t>(0), (size_t)img.step, img.cols, img.rows, xy);
    kpts2d.resize(xy.size() / 2);
    for (size_t i = 0; i < kpts2d.size(); i++)
      kpts2d[i] = cv::KeyPoint(cv::Point2f(xy[2 * i], xy[2 * i + 1]), (float)p_.block_size);
  }
#endif

 private:
  static void check(int st) {
    if (st != SBM_OK) throw Error(st, sbm_strerror(st));
  }
  sbm_handle* h_ = nullptr;
  sbm_gftt_cv_params p_;
};

// One detector per process on device 0, created at the first call (what the reference's free function needs).
inline GfttCv& default_gftt_cv() {
  static GfttCv s;
  return s;
}

inline void generateKeypoints(const uint8_t* img, size_t img_stride, int width, int height, std::vector<float>& xy) {
  default_gftt_cv().detect(img, img_stride, width, height, xy);
}

#ifdef SBM_HAVE_OPENCV
inline void generateKeypoints(cv::Mat& img, std::vector<cv::KeyPoint>& kpts2d) { default_gftt_cv().detect(img, kpts2d); }
#endif

}  // namespace sbm

#endif  // SBM_GFTT_HPP_
