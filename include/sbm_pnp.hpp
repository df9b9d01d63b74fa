// sbm_pnp.hpp -- header-only C++ adaptor for the motion estimation of the reference's computeTransform (sbm.h, sbm_pnp_* and
// sbm_estimate_motion), so that the body of estimateMotion in src/slam/src/core/Registration.cpp becomes one call:
//
//     sbm::Motion m = sbm::estimateMotion3DTo2D(words3A, wordsB, k, local, minInliers, refineIterations, words3B);
//
// with the reference's std::map inputs (words3A / words3B: VW id -> cv::Point3f, words2B: VW id -> cv::KeyPoint), k the left
// camera's fx, fy, cx, cy and local the camera model's localTransform as 12 floats r11 r12 r13 x / r21 .. y / r31 .. z (nullptr:
// none). The motion guess is not taken: it cannot change the output (sbm.h). Motion holds the transform as 12 floats (all zero
// and isNull() when the reference returns a null Transform), the 6 x 6 covariance (identity with the 3 x 3 blocks scaled), the
// matches and the inliers as VW ids, exactly as estimateMotion3DTo2D's matchesOut / inliersOut. The map-typed form exists when
// OpenCV headers are present (SBM_HAVE_OPENCV, as in sbm_stereobm.hpp); the plain form takes arrays. Failures throw sbm::Error.
#ifndef SBM_PNP_HPP_
#define SBM_PNP_HPP_

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <vector>

#include "sbm_stereobm.hpp"   // sbm::Error and the OpenCV detection

namespace sbm {

struct Motion {
  int status = SBM_PNP_FEW_MATCHES;   // SBM_PNP_*
  float transform[12] = {};           // (localTransform * pnp).inverse(), row-major 3 x 4; zeros unless status == SBM_PNP_OK
  double covariance[36] = {};         // row-major 6 x 6
  std::vector<int> matches;           // the ids of the gathered correspondences, increasing
  std::vector<int> inliers;           // the ids of the final inliers
  sbm_pnp_result record = {};         // the engine's full record (indices in it refer to positions in `matches`' gather)
  bool isNull() const { return status != SBM_PNP_OK; }
};

class MotionEstimator {
 public:
  // the reference's constants unless p is given; `device` selects the HIP device
  explicit MotionEstimator(int device = 0, const sbm_pnp_params* p = nullptr) {
    if (p) p_ = *p; else sbm_pnp_params_default(&p_);
    check(sbm_pnp_params_validate(&p_));
    sbm_params bm;
    sbm_params_default(&bm, 0, 0);   // the handle's block-matcher parameters are not used here
    check(sbm_create(&h_, &bm, device));
  }
  ~MotionEstimator() { sbm_destroy(h_); }
  MotionEstimator(const MotionEstimator&) = delete;
  MotionEstimator& operator=(const MotionEstimator&) = delete;

  const sbm_pnp_params& params() const { return p_; }
  sbm_handle* handle() { return h_; }

  // The plain form over n correspondences in increasing id: object points xyz_from (n float (x, y, z); NaN = no depth, dropped
  // as the reference drops them), image points kpts_to (n float (x, y)), the to-frame's points xyz_to (n; NaN = none), ids (n).
  Motion estimate(const float* xyz_from, const float* kpts_to, const float* xyz_to, const int* ids, int n, const double K[4],
                  const float* local, int minInliers, int refineIterations) {
    sbm_pnp_params p = p_;
    p.min_inliers = minInliers;
    p.refine_iterations = refineIterations;
    check(sbm_pnp_params_validate(&p));
    sbm_stereo_model model = {};
    if (local) {
      for (int i = 0; i < 12; i++) model.local[i] = local[i];
      model.has_local = 1;
    }
    std::vector<int> pairs(2 * (size_t)std::max(n, 1)), inl((size_t)std::max(n, 1));
    for (int i = 0; i < n; i++) pairs[2 * i] = pairs[2 * i + 1] = i;
    Motion m;
    check(sbm_estimate_motion(h_, xyz_from, n, kpts_to, xyz_to, n, pairs.data(), n, K, &model, &p, &m.record, inl.data()));
    m.status = m.record.status;
    for (int i = 0; i < n; i++)   // the gather, as the engine ran it: finite object points in increasing id
      if (std::isfinite(xyz_from[3 * i]) && std::isfinite(xyz_from[3 * i + 1]) && std::isfinite(xyz_from[3 * i + 2]))
        m.matches.push_back(ids[i]);
    for (int i = 0; i < m.record.num_inliers; i++) m.inliers.push_back(ids[inl[i]]);
    for (int i = 0; i < 36; i++) m.covariance[i] = (i % 7) == 0 ? 1.0 : 0.0;
    if (m.status == SBM_PNP_OK) {
      for (int i = 0; i < 12; i++) m.transform[i] = m.record.transform[i];
      for (int i = 0; i < 3; i++) {
        m.covariance[7 * i] = m.record.cov_dist;
        m.covariance[7 * (i + 3)] = m.record.cov_angle;
      }
    }
    return m;
  }

#ifdef SBM_HAVE_OPENCV
  Motion estimate(const std::map<int, cv::Point3f>& words3A, const std::map<int, cv::KeyPoint>& words2B, const double K[4],
                  const float* local, int minInliers, int refineIterations, const std::map<int, cv::Point3f>& words3B) {
    const float nan = std::nanf("");
    std::vector<float> xa, kb, xb;
    std::vector<int> ids;
    for (const auto& w : words2B) {   // estimateMotion3DTo2D's scan over words2B's ids
      auto a = words3A.find(w.first);
      auto b = words3B.find(w.first);
      ids.push_back(w.first);
      if (a != words3A.end()) { xa.push_back(a->second.x); xa.push_back(a->second.y); xa.push_back(a->second.z); }
      else { xa.push_back(nan); xa.push_back(nan); xa.push_back(nan); }
      kb.push_back(w.second.pt.x);
      kb.push_back(w.second.pt.y);
      if (b != words3B.end()) { xb.push_back(b->second.x); xb.push_back(b->second.y); xb.push_back(b->second.z); }
      else { xb.push_back(nan); xb.push_back(nan); xb.push_back(nan); }
    }
    return estimate(xa.data(), kb.data(), xb.data(), ids.data(), (int)ids.size(), K, local, minInliers, refineIterations);
  }
#endif

 private:
  static void check(int st) {
    if (st != SBM_OK) throw Error(st, sbm_strerror(st));
  }
  sbm_handle* h_ = nullptr;
  sbm_pnp_params p_;
};

// The estimator of the free function: one per process, on device 0, created at the first call.
inline MotionEstimator& default_motion_estimator() {
  static std::unique_ptr<MotionEstimator> m(new MotionEstimator(0));
  return *m;
}

#ifdef SBM_HAVE_OPENCV
inline Motion estimateMotion3DTo2D(const std::map<int, cv::Point3f>& words3A, const std::map<int, cv::KeyPoint>& words2B,
                                   const double K[4], const float* localTransform, int minInliers, int refineIterations,
                                   const std::map<int, cv::Point3f>& words3B) {
  return default_motion_estimator().estimate(words3A, words2B, K, localTransform, minInliers, refineIterations, words3B);
}
#endif

}  // namespace sbm

#endif  // SBM_PNP_HPP_
