// sbm_match.hpp -- header-only C++ adaptor for the keypoint matching of the reference's computeTransform (sbm.h, sbm_match_*), so
// that the bodies of matchingNoGuess and matchingGuess in src/slam/src/core/Registration.cpp become one call each:
//
//     sbm::matchingNoGuess(sensorFrom.descriptors(), sensorTo.descriptors(), matchedIndex);
//     sbm::matchingGuess(sensorFrom.keypoints3D(), sensorTo.keypoints(), sensorFrom.descriptors(), sensorTo.descriptors(),
//                        guessCameraRef, K, sensorTo.stereoCameraModel().imageSize(), matchedIndex);
//
// guessCameraRef is (guess * cameraModel.localTransform()).inverse() as 12 floats r11 r12 r13 x / r21 .. y / r31 .. z, K the left
// camera's fx, fy, cx, cy. Pairs are appended to the multimap in increasing from-index, as the reference inserts them. The
// reference-signature overloads exist when OpenCV headers are present (SBM_HAVE_OPENCV, as in sbm_stereobm.hpp); descriptors must
// be CV_8U with 32 columns. The plain form takes raw strided rows. Failures throw sbm::Error.
#ifndef SBM_MATCH_HPP_
#define SBM_MATCH_HPP_

#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "sbm_stereobm.hpp"   // sbm::Error and the OpenCV detection

namespace sbm {

class Matcher {
 public:
  // the reference's constants unless p is given; `device` selects the HIP device
  explicit Matcher(int device = 0, const sbm_match_params* p = nullptr) {
    if (p) p_ = *p; else sbm_match_params_default(&p_);
    check(sbm_match_params_validate(&p_));
    sbm_params bm;
    sbm_params_default(&bm, 0, 0);   // the handle's block-matcher parameters are not used by the matcher
    check(sbm_create(&h_, &bm, device));
  }
  ~Matcher() { sbm_destroy(h_); }
  Matcher(const Matcher&) = delete;
  Matcher& operator=(const Matcher&) = delete;

  const sbm_match_params& params() const { return p_; }
  sbm_handle* handle() { return h_; }

  // matchingNoGuess on raw rows (32 bytes each, strides in bytes): (from, to) pairs in increasing from
  std::vector<std::pair<int, int>> noGuess(const uint8_t* from, size_t from_stride, int nf, const uint8_t* to, size_t to_stride,
                                           int nt) {
    std::vector<int> pr(2 * (size_t)std::max(nf, 1));
    int k = 0;
    check(sbm_match(h_, from, from_stride, nf, to, to_stride, nt, &p_, pr.data(), &k));
    return pairs(pr, k);
  }
  // matchingGuess on raw arrays: xyz nf float (x, y, z), kpts nt float (x, y), T 12 floats, K fx, fy, cx, cy
  std::vector<std::pair<int, int>> guess(const float* xyz, const float* kpts, const uint8_t* from, size_t from_stride, int nf,
                                         const uint8_t* to, size_t to_stride, int nt, const float* T, const double* K, int width,
                                         int height) {
    std::vector<int> pr(2 * (size_t)std::max(nf, 1));
    const float none[3] = {0.f, 0.f, 0.f};
    int k = 0;
    check(sbm_match_guess(h_, xyz ? xyz : none, kpts ? kpts : none, from, from_stride, nf, to, to_stride, nt, T, K, width, height,
                          &p_, pr.data(), &k));
    return pairs(pr, k);
  }

#ifdef SBM_HAVE_OPENCV
  void noGuess(const cv::Mat& descFrom, const cv::Mat& descTo, std::multimap<int, int>& matched) {
    check_desc(descFrom);
    check_desc(descTo);
    for (const auto& pq : noGuess(rows(descFrom), (size_t)descFrom.step, descFrom.rows, rows(descTo), (size_t)descTo.step,
                                  descTo.rows))
      matched.insert(matched.end(), pq);
  }
  void guess(const std::vector<cv::Point3f>& kptsFrom3D, const std::vector<cv::KeyPoint>& kptsTo, const cv::Mat& descFrom,
             const cv::Mat& descTo, const float guessCameraRef[12], const double K[4], cv::Size imageSize,
             std::multimap<int, int>& matched) {
    check_desc(descFrom);
    check_desc(descTo);
    if ((int)kptsFrom3D.size() != descFrom.rows || (int)kptsTo.size() != descTo.rows)
      throw Error(SBM_ERR_SIZE, "one keypoint per descriptor row");
    std::vector<float> xyz, xy;
    xyz.reserve(3 * kptsFrom3D.size());
    for (const cv::Point3f& p : kptsFrom3D) { xyz.push_back(p.x); xyz.push_back(p.y); xyz.push_back(p.z); }
    xy.reserve(2 * kptsTo.size());
    for (const cv::KeyPoint& kp : kptsTo) { xy.push_back(kp.pt.x); xy.push_back(kp.pt.y); }
    for (const auto& pq : guess(xyz.data(), xy.data(), rows(descFrom), (size_t)descFrom.step, descFrom.rows, rows(descTo),
                                (size_t)descTo.step, descTo.rows, guessCameraRef, K, imageSize.width, imageSize.height))
      matched.insert(matched.end(), pq);
  }
#endif

 private:
  static void check(int st) {
    if (st != SBM_OK) throw Error(st, sbm_strerror(st));
  }
  static std::vector<std::pair<int, int>> pairs(const std::vector<int>& pr, int k) {
    std::vector<std::pair<int, int>> out((size_t)k);
    for (int i = 0; i < k; i++) out[i] = std::make_pair(pr[2 * i], pr[2 * i + 1]);
    return out;
  }
#ifdef SBM_HAVE_OPENCV
  static void check_desc(const cv::Mat& d) {
    if (d.empty()) return;
    if (d.cols != 32 || d.type() != CV_8U) throw Error(SBM_ERR_SIZE, "descriptors must be CV_8U rows of 32 bytes");
  }
  static const uint8_t* rows(const cv::Mat& d) { return d.empty() ? nullptr : d.ptr<uint8_t>(0); }
#endif
  sbm_handle* h_ = nullptr;
  sbm_match_params p_;
};

// The matcher of the free functions: one per process, on device 0, created at the first call.
inline Matcher& default_matcher() {
  static std::unique_ptr<Matcher> m(new Matcher(0));
  return *m;
}

#ifdef SBM_HAVE_OPENCV
inline void matchingNoGuess(const cv::Mat& descFrom, const cv::Mat& descTo, std::multimap<int, int>& matchedIndex) {
  default_matcher().noGuess(descFrom, descTo, matchedIndex);
}
inline void matchingGuess(const std::vector<cv::Point3f>& kptsFrom3D, const std::vector<cv::KeyPoint>& kptsTo,
                          const cv::Mat& descFrom, const cv::Mat& descTo, const float guessCameraRef[12], const double K[4],
                          cv::Size imageSize, std::multimap<int, int>& matchedIndex) {
  default_matcher().guess(kptsFrom3D, kptsTo, descFrom, descTo, guessCameraRef, K, imageSize, matchedIndex);
}
#endif

}  // namespace sbm

#endif  // SBM_MATCH_HPP_
