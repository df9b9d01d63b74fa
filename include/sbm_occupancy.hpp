// sbm_occupancy.hpp -- header-only C++ adaptor for the reference's occupancy map (sbm.h, sbm_occ_*), so that the body of
//
//     void buildOccupancyGridMap(Mapper &mapper, std::map<int, Transform> &optimized_poses)
//                                                                     // src/slam/src/core/main.cpp:495-561
//
// becomes one insert() per node and one writeBinary(): the per-pixel reprojection, transforms, range gate and
// key run on the MI355X, only the distinct voxels come back, and the .bt stream is written from them. Failures throw sbm::Error;
// a map that is too small throws with code SBM_ERR_OCC_FULL (nothing is dropped silently: overflow() counts the points).
#ifndef SBM_OCCUPANCY_HPP_
#define SBM_OCCUPANCY_HPP_

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sbm_stereobm.hpp"   // sbm::Error

namespace sbm {

class OccupancyMap {
 public:
  // octomap::OcTree tree(resolution) and the reference's rangeMax_ (0.1, 5.0f); capacity in voxels
  explicit OccupancyMap(size_t capacity, double resolution = 0.1, float range_max = 5.0f, int device = 0) {
    sbm_occ_params_default(&p_);
    p_.resolution = resolution;
    p_.range_max = range_max;
    sbm_params bm;
    sbm_params_default(&bm, 0, 0);   // the handle's block-matcher parameters are not used by the map
    check(sbm_create(&h_, &bm, device));
    const int st = sbm_occ_create(h_, &p_, capacity, &m_);
    if (st != SBM_OK) {
      sbm_destroy(h_);
      check(st);
    }
  }
  ~OccupancyMap() {
    sbm_occ_destroy(m_);
    sbm_destroy(h_);
  }
  OccupancyMap(const OccupancyMap&) = delete;
  OccupancyMap& operator=(const OccupancyMap&) = delete;

  const sbm_occ_params& params() const { return p_; }
  sbm_handle* handle() { return h_; }
  sbm_occ_map* map() { return m_; }

  // One node: its (decimated) int16 disparity map, dense rows, the decimation scale, its camera model and the optimised pose
  // as 12 floats r11 r12 r13 o14 / r21 r22 r23 o24 / r31 r32 r33 o34.
  void insert(const int16_t* disp, int width, int height, int scale, const sbm_stereo_model& model, const float pose[12]) {
    check(sbm_occ_insert(m_, 1, disp, width, height, scale, &model, pose));
  }
  // n planes of one size in DEVICE memory (as sbm_decimate_device leaves them) with their n poses in host memory
  void insertDevice(int n, const void* d_disp, int width, int height, int scale, const sbm_stereo_model& model, const float* poses,
                    bool sync = true) {
    check(sbm_occ_insert_device(m_, n, d_disp, width, height, scale, &model, poses, sync ? 1 : 0));
  }
  void reset() { check(sbm_occ_reset(m_)); }

  size_t size() {
    size_t n = 0;
    check(sbm_occ_size(m_, &n));
    return n;
  }
  uint64_t overflow() {
    uint64_t n = 0;
    check(sbm_occ_overflow(m_, &n));
    return n;
  }
  // the distinct voxels ascending by packed key (k0 << 32 | k1 << 16 | k2); hits (may be null) receives the points per voxel
  std::vector<uint64_t> keys(std::vector<uint32_t>* hits = nullptr) {
    std::vector<uint64_t> k(size());
    if (hits) hits->assign(k.size(), 0);
    size_t n = 0;
    check(sbm_occ_fetch(m_, k.data(), hits ? hits->data() : nullptr, k.size(), &n));
    k.resize(n);
    if (hits) hits->resize(n);
    return k;
  }
  // tree.writeBinary(path)
  void writeBinary(const std::string& path) {
    const std::vector<uint64_t> k = keys();
    check(sbm_occ_write_binary(k.data(), k.size(), p_.resolution, path.c_str()));
  }

 private:
  static void check(int st) {
    if (st != SBM_OK) throw Error(st, sbm_strerror(st));
  }
  sbm_occ_params p_;
  sbm_handle* h_ = nullptr;
  sbm_occ_map* m_ = nullptr;
};

}  // namespace sbm

#endif  // SBM_OCCUPANCY_HPP_
