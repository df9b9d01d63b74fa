// sbm_orb.hpp -- header-only C++ adaptor for the descriptor step of the reference's feature path (sbm.h, sbm_orb_*), so that
// the call
//
//     computeDescriptor(data.imageLeft(), cv::noArray(), kpts2d, true, desc);   // src/slam/src/core/main.cpp:246-248
//
// compiles against the MI355X engine once this header replaces CvORB.h's declaration and the sampling pattern has been handed
// over once with sbm::setOrbPattern(bit_pattern_31_2). The reference-signature overload exists when OpenCV
// headers are present (SBM_HAVE_OPENCV, as in sbm_stereobm.hpp); like the reference it erases the keypoints near the border
// from kpts2d (stable) and fills desc with one 32-byte row per remaining keypoint; the mask and useProvidedKeypoints are
// ignored, as the reference ignores them. Keypoints must share one angle and have octave 0 (SBM_ERR_UNSUPPORTED otherwise).
// The plain form takes a raw strided u8 frame and (x, y) pairs. Failures throw sbm::Error.
#ifndef SBM_ORB_HPP_
#define SBM_ORB_HPP_

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "sbm_stereobm.hpp"   // sbm::Error and the OpenCV detection

namespace sbm {

class OrbDescriptor {
 public:
  // pattern: 512 points (x, y) as 1024 ints (the reference's bit_pattern_31_2), copied; the reference's constants unless p
  // is given; `device` selects the HIP device
  OrbDescriptor(int device, const int* pattern, const sbm_orb_params* p = nullptr) {
    if (!pattern) throw Error(SBM_ERR_NULL, "OrbDescriptor needs a sampling pattern");
    pattern_.assign(pattern, pattern + 1024);
    if (p) p_ = *p; else sbm_orb_params_default(&p_);
    check(sbm_orb_params_validate(&p_));
    sbm_params bm;
    sbm_params_default(&bm, 0, 0);   // the handle's block-matcher parameters are not used by the descriptors
    check(sbm_create(&h_, &bm, device));
  }
  ~OrbDescriptor() { sbm_destroy(h_); }
  OrbDescriptor(const OrbDescriptor&) = delete;
  OrbDescriptor& operator=(const OrbDescriptor&) = delete;

  const sbm_orb_params& params() const { return p_; }
  void setParams(const sbm_orb_params& p) { p_ = p; }
  sbm_handle* handle() { return h_; }

  // One strided u8 frame (stride in bytes); xy = x0, y0, x1, y1, ... is shortened to the kept points, desc receives 32 bytes
  // per kept point.
  void compute(const uint8_t* img, size_t stride, int width, int height, std::vector<float>& xy, std::vector<uint8_t>& desc) {
    const int n = (int)(xy.size() / 2);
    desc.resize((size_t)n * 32);
    int k = 0;
    check(sbm_orb_describe(h_, img, stride, width, height, xy.data(), n, pattern_.data(), &p_, xy.data(), &k, desc.data()));
    xy.resize(2 * (size_t)k);
    desc.resize((size_t)k * 32);
  }

#ifdef SBM_HAVE_OPENCV
  // computeDescriptor(image, mask, keypoints, useProvidedKeypoints, desc): image CV_8UC1 (any row step)
  void compute(cv::InputArray image, std::vector<cv::KeyPoint>& keypoints, cv::Mat& desc) {
    cv::Mat img = image.getMat();
#ifndef SBM_MOCK_OPENCV
    if (img.depth() != CV_8U || img.channels() != 1) throw Error(SBM_ERR_SIZE, "image must be CV_8UC1");
#endif
    sbm_orb_params p = p_;
    if (!keypoints.empty()) p.angle = keypoints[0].angle;
    std::vector<float> xy;
    xy.reserve(2 * keypoints.size());
    for (const cv::KeyPoint& kp : keypoints) {
      if (kp.octave != 0) throw Error(SBM_ERR_UNSUPPORTED, "keypoints above pyramid level 0 are not supported");
      if (!(kp.angle == p.angle)) throw Error(SBM_ERR_UNSUPPORTED, "keypoints with different angles are not supported");
      xy.push_back(kp.pt.x);
      xy.push_back(kp.pt.y);
    }
    const int n = (int)keypoints.size();
    std::vector<uint8_t> d((size_t)n * 32);
    int k = 0;
    check(sbm_orb_describe(h_, img.ptr<uint8_t>(0), (size_t)img.step, img.cols, img.rows, xy.data(), n, pattern_.data(), &p,
                           xy.data(), &k, d.data()));
    // the kept points are a subsequence decided by (x, y) alone: match them in order
    size_t w = 0;
    for (size_t r = 0; r < keypoints.size() && (int)w < k; r++)
      if (keypoints[r].pt.x == xy[2 * w] && keypoints[r].pt.y == xy[2 * w + 1]) keypoints[w++] = keypoints[r];
    keypoints.resize(w);
    desc.create(k, 32, CV_8U);
    for (int j = 0; j < k; j++) std::memcpy(desc.ptr<uint8_t>(j), d.data() + (size_t)j * 32, 32);
  }
#endif

 private:
  static void check(int st) {
    if (st != SBM_OK) throw Error(st, sbm_strerror(st));
  }
  sbm_handle* h_ = nullptr;
  std::vector<int> pattern_;
  sbm_orb_params p_;
};

// The pattern of the free function, and its descriptor object on device 0 (created at the first call after setOrbPattern).
inline std::vector<int>& orb_pattern_store() {
  static std::vector<int> p;
  return p;
}
inline std::unique_ptr<OrbDescriptor>& orb_default_slot() {
  static std::unique_ptr<OrbDescriptor> d;
  return d;
}
inline void setOrbPattern(const int* pattern) {
  if (!pattern) throw Error(SBM_ERR_NULL, "setOrbPattern needs a pattern");
  orb_pattern_store().assign(pattern, pattern + 1024);
  orb_default_slot().reset();
}
inline OrbDescriptor& default_orb_descriptor() {
  if (orb_pattern_store().empty()) throw Error(SBM_ERR_NULL, "no ORB pattern: call sbm::setOrbPattern(bit_pattern_31_2) first");
  if (!orb_default_slot()) orb_default_slot().reset(new OrbDescriptor(0, orb_pattern_store().data()));
  return *orb_default_slot();
}

inline void computeDescriptor(const uint8_t* img, size_t stride, int width, int height, std::vector<float>& xy,
                              std::vector<uint8_t>& desc) {
  default_orb_descriptor().compute(img, stride, width, height, xy, desc);
}

#ifdef SBM_HAVE_OPENCV
inline void computeDescriptor(cv::InputArray image, cv::InputArray /*mask*/, std::vector<cv::KeyPoint>& keypoints,
                              bool /*useProvidedKeypoints*/, cv::Mat& desc) {
  default_orb_descriptor().compute(image, keypoints, desc);
}
#endif

}  // namespace sbm

#endif  // SBM_ORB_HPP_
