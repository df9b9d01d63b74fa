// sbm_vwd.hpp -- header-only C++ adaptor for the reference's loop-closure thread (sbm.h, sbm_vwd_*), so that the calls of
// addWordIds and detectLoopClosure (src/slam/src/core/Mapper.cpp:413-484, 536-677) keep their shape:
//
//     sbm::VWDictionary vwd(1 << 20);                                     // capacity in words
//     sbm::limitKeypoints(keypoints, inliers, maxFeatures);               // SensorData::limitKeypoints
//     addedWordIds = vwd.addNewWords(descriptorsForVwd, node->id(), (int)keypoints.size());
//     likelihood = sbm::computeLikelihood(vwd, node->id(), (int)nodes.size(), nodesToCompare);
//
// The 2-NN search of addNewWords runs on the MI355X and is exhaustive (the reference's FLANN kd-trees are approximate); the
// dictionary keeps each word's references and each node's words and keypoint count, so computeLikelihood needs no Node. The
// third argument of addNewWords is the node's keypoint count including the ones limitKeypoints cut (the reference's
// getWords().size()); it defaults to the number of rows. The reference-signature overloads exist when OpenCV headers are present
// (SBM_HAVE_OPENCV, as in sbm_stereobm.hpp); descriptors must be CV_8U with 32 columns. Failures throw sbm::Error; a dictionary
// that is too small throws with code SBM_ERR_VWD_FULL and adds nothing.
#ifndef SBM_VWD_HPP_
#define SBM_VWD_HPP_

#include <cstddef>
#include <cstdint>
#include <list>
#include <map>
#include <utility>
#include <vector>

#include "sbm_stereobm.hpp"   // sbm::Error and the OpenCV detection

namespace sbm {

class VWDictionary {
 public:
  // the reference's constants unless p is given; `device` selects the HIP device
  explicit VWDictionary(size_t capacity, int device = 0, const sbm_vwd_params* p = nullptr) {
    if (p) p_ = *p; else sbm_vwd_params_default(&p_);
    sbm_params bm;
    sbm_params_default(&bm, 0, 0);   // the handle's block-matcher parameters are not used by the dictionary
    check(sbm_create(&h_, &bm, device));
    const int st = sbm_vwd_create(h_, capacity, &p_, &v_);
    if (st != SBM_OK) {
      sbm_destroy(h_);
      check(st);
    }
  }
  ~VWDictionary() {
    sbm_vwd_destroy(v_);
    sbm_destroy(h_);
  }
  VWDictionary(const VWDictionary&) = delete;
  VWDictionary& operator=(const VWDictionary&) = delete;

  const sbm_vwd_params& params() const { return p_; }
  sbm_handle* handle() { return h_; }
  sbm_vwd* dictionary() { return v_; }

  // addNewWords on raw rows (32 bytes each, stride in bytes): the word id of every row
  std::list<int> addNewWords(const uint8_t* rows, size_t stride, int n, int nodeId, int nKeypointsTotal = -1) {
    std::vector<int> ids((size_t)(n > 0 ? n : 1));
    check(sbm_vwd_add_words(v_, rows, stride, n, nodeId, nKeypointsTotal < 0 ? n : nKeypointsTotal, ids.data()));
    return std::list<int>(ids.begin(), ids.begin() + (n > 0 ? n : 0));
  }
  // the same on n dense rows in DEVICE memory, as sbm_orb_describe_device leaves a frame's descriptors
  std::list<int> addNewWordsDevice(const void* d_rows, int n, int nodeId, int nKeypointsTotal = -1) {
    std::vector<int> ids((size_t)(n > 0 ? n : 1));
    check(sbm_vwd_add_words_device(v_, d_rows, n, nodeId, nKeypointsTotal < 0 ? n : nKeypointsTotal, ids.data()));
    return std::list<int>(ids.begin(), ids.begin() + (n > 0 ? n : 0));
  }
#ifdef SBM_HAVE_OPENCV
  std::list<int> addNewWords(const cv::Mat& descriptorsIn, int nodeId, int nKeypointsTotal = -1) {
    if (descriptorsIn.empty()) return addNewWords(nullptr, 32, 0, nodeId, nKeypointsTotal);
    if (descriptorsIn.cols != 32 || descriptorsIn.type() != CV_8U) throw Error(SBM_ERR_SIZE, "descriptors must be CV_8U rows of 32 bytes");
    return addNewWords(descriptorsIn.ptr<uint8_t>(0), (size_t)descriptorsIn.step, descriptorsIn.rows, nodeId, nKeypointsTotal);
  }
#endif

  // computeLikelihood(node, nodes, vwd, ids): N = nodes.size(); the map holds every id of `ids`
  std::map<int, float> likelihood(int nodeId, int nNodes, const std::list<int>& ids, std::pair<int, float>* highest = nullptr) {
    const std::vector<int> c(ids.begin(), ids.end());
    std::vector<float> s(c.size() ? c.size() : 1);
    int best = 0;
    float score = 0.f;
    check(sbm_vwd_likelihood(v_, nodeId, c.data(), (int)c.size(), nNodes, s.data(), &best, &score));
    std::map<int, float> out;
    for (size_t i = 0; i < c.size(); i++) out.insert(std::make_pair(c[i], s[i]));
    if (highest) *highest = std::make_pair(best, score);
    return out;
  }

  size_t size() {
    size_t n = 0;
    check(sbm_vwd_size(v_, &n));
    return n;
  }
  uint64_t overflow() {
    uint64_t n = 0;
    check(sbm_vwd_overflow(v_, &n));
    return n;
  }
  void clear() { check(sbm_vwd_reset(v_)); }

 private:
  static void check(int st) {
    if (st != SBM_OK) throw Error(st, sbm_strerror(st));
  }
  sbm_vwd_params p_;
  sbm_handle* h_ = nullptr;
  sbm_vwd* v_ = nullptr;
};

// computeLikelihood in the reference's spelling; `highest` (may be null) receives detectLoopClosure's highest hypothesis
inline std::map<int, float> computeLikelihood(VWDictionary& vwd, int nodeId, int nNodes, const std::list<int>& ids,
                                              std::pair<int, float>* highest = nullptr) {
  return vwd.likelihood(nodeId, nNodes, ids, highest);
}

// SensorData::limitKeypoints on the responses alone
inline void limitKeypoints(const std::vector<float>& responses, std::vector<bool>& inliers, int maxKeypoints) {
  std::vector<uint8_t> keep(responses.size() ? responses.size() : 1);
  const int st = sbm_vwd_limit_keypoints(responses.data(), (int)responses.size(), maxKeypoints, keep.data());
  if (st != SBM_OK) throw Error(st, sbm_strerror(st));
  inliers.assign(responses.size(), false);
  for (size_t i = 0; i < responses.size(); i++) inliers[i] = keep[i] != 0;
}
#ifdef SBM_HAVE_OPENCV
inline void limitKeypoints(const std::vector<cv::KeyPoint>& keypoints, std::vector<bool>& inliers, int maxKeypoints) {
  std::vector<float> r;
  r.reserve(keypoints.size());
  for (const cv::KeyPoint& k : keypoints) r.push_back(k.response);
  limitKeypoints(r, inliers, maxKeypoints);
}
#endif

}  // namespace sbm

#endif  // SBM_VWD_HPP_
