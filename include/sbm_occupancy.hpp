// sbm_occupancy.hpp -- header-only C++ adaptor for the reference's occupancy map (sbm.h, sbm_occ_*), so that the body of
//
//     void buildOccupancyGridMap(Mapper &mapper, std::map<int, Transform> &optimized_poses)
//                                                                     // src/slam/src/core/main.cpp:495-561
//
// becomes one insert() per node and one writeBinary(): the per-pixel reprojection, transforms, range gate and
// key run on the MI355X, only the distinct voxels come back, and the .bt stream is written from them. Failures throw sbm::Error;
// a map that is too small throws with code SBM_ERR_OCC_FULL (nothing is dropped silently: overflow() counts the points).
// insertRays() / insertPointCloud() / writeBinaryLogOdds() are the same loop with octomap's insertPointCloud in place of
// updateNode: free space is ray-cast from each node's sensor origin and the .bt holds free and occupied leaves.
// search() / castRay() / castRays() / castView() are octomap's search and castRay on the device: castRay has octomap's signature
// and result for a call-site swap, the batch forms take arrays.
// buildTree() gives an OccupancyTree: octomap's sixteen levels above the voxels as a snapshot on the device, with search(point,
// depth), leaves(maxDepth), size() / getNumLeafNodes() and writeBinary() in octomap's spelling.
// readBinary() loads a .bt back into the map: the host parses the pruned tree, the device expands its leaves to voxels.
// write() / read() are octomap's .ot file, which keeps every voxel's log-odds: scans, write, read, more scans equal the
// uninterrupted run.
// setBBXMin() / setBBXMax() / useBBXLimit(), enableChangeDetection() / changedKeys() and the discretize flag of insertPointCloud
// are octomap's three insert switches, in its spelling.
// reserve() / setGrowth() let the table grow on the device, so that a long-running mapper need not know its voxel count.
// updateNode() / setNodeValue() / deleteNode() / deleteBBX() edit and forget voxels by key or point, in octomap's spelling; the
// vector forms take a batch in item order.
// leafs_bbx() / getUnknownLeafCenters() / getMetricMin() / getMetricMax() / getMetricSize() / volume() on a tree and
// getRayIntersection() on the map are octomap's read side for planners, in its spelling.
#ifndef SBM_OCCUPANCY_HPP_
#define SBM_OCCUPANCY_HPP_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "sbm_stereobm.hpp"   // sbm::Error

namespace sbm {

// One entry of leaves(maxDepth): octomap's centre key packed as the map packs keys, the node's depth and its value
struct OccupancyLeaf {
  uint64_t key;
  int32_t depth;
  float value;
};

// The tree above the voxels of an OccupancyMap as it was when the tree was (re)built: updateInnerOccupancy() and prune() done.
// The map's handle must outlive it.
class OccupancyTree {
 public:
  OccupancyTree(sbm_occ_map* map, float occupancy_thres_log) : thres_(occupancy_thres_log) { check(sbm_occ_tree_create(map, &t_)); }
  ~OccupancyTree() { sbm_occ_tree_destroy(t_); }
  OccupancyTree(const OccupancyTree&) = delete;
  OccupancyTree& operator=(const OccupancyTree&) = delete;
  sbm_occ_tree* tree() { return t_; }

  // a new snapshot: SBM_OCC_TREE_LOGODDS (the stored log-odds) or SBM_OCC_TREE_MAXLIKELIHOOD (toMaxLikelihood(), what .bt holds)
  void rebuild(int reading, const sbm_occ_ray_params& params) { check(sbm_occ_tree_build(t_, reading, &params, 1)); }
  sbm_occ_tree_counts info() {
    sbm_occ_tree_counts c;
    check(sbm_occ_tree_info(t_, &c));
    return c;
  }
  size_t size() { return (size_t)info().nodes; }                  // tree.size() == calcNumNodes() after prune()
  size_t getNumLeafNodes() { return (size_t)info().leaves; }
  // tree.search(x, y, z, depth): SBM_OCC_CELL_*; *value (may be null) receives the node's float, NaN where there is no node;
  // *found_depth (may be null) the depth of the node octomap returns, -1 where there is none
  int search(float x, float y, float z, unsigned depth = 0, float* value = nullptr, int* found_depth = nullptr) {
    const float p[3] = {x, y, z};
    int32_t state = 0, fd = -1;
    check(sbm_occ_tree_search(t_, 1, p, (int)depth, thres_, &state, value, &fd));
    if (found_depth) *found_depth = fd;
    return state;
  }
  // n points (host memory) at once
  void search(const float* xyz, size_t n, unsigned depth, int32_t* states, void* values = nullptr, int32_t* found_depths = nullptr) {
    check(sbm_occ_tree_search(t_, n, xyz, (int)depth, thres_, states, values, found_depths));
  }
  // for (it = tree.begin_leafs(maxDepth); it != tree.end_leafs(); ++it), in that order
  std::vector<OccupancyLeaf> leaves(unsigned maxDepth = 0) {
    size_t n = 0;
    std::vector<uint64_t> k;
    std::vector<int32_t> d;
    std::vector<float> v;
    int st = sbm_occ_tree_leaves(t_, (int)maxDepth, nullptr, nullptr, nullptr, 0, &n);   // the count
    if (st != SBM_OK && st != SBM_ERR_SIZE) check(st);
    k.resize(n), d.resize(n), v.resize(n);
    check(sbm_occ_tree_leaves(t_, (int)maxDepth, k.data(), d.data(), v.data(), n, &n));
    std::vector<OccupancyLeaf> out(n);
    for (size_t i = 0; i < n; i++) out[i] = OccupancyLeaf{k[i], d[i], v[i]};
    return out;
  }
  // for (it = tree.begin_leafs_bbx(min, max, maxDepth); it != tree.end_leafs_bbx(); ++it), by keys (both ends inclusive) ...
  std::vector<OccupancyLeaf> leafs_bbx(const uint16_t min[3], const uint16_t max[3], unsigned maxDepth = 0) {
    return listed([&](uint64_t* k, int32_t* d, float* v, size_t cap, size_t* n) {
      return sbm_occ_bbx_leaves(t_, min, max, (int)maxDepth, k, d, v, cap, n);
    });
  }
  // ... and by points: a corner without a key visits nothing
  std::vector<OccupancyLeaf> leafs_bbx(const float min[3], const float max[3], unsigned maxDepth = 0) {
    return listed([&](uint64_t* k, int32_t* d, float* v, size_t cap, size_t* n) {
      return sbm_occ_bbx_leaves_points(t_, min, max, (int)maxDepth, k, d, v, cap, n);
    });
  }
  // tree.getUnknownLeafCenters(node_centers, pmin, pmax, depth): x y z triples appended in octomap's push order
  void getUnknownLeafCenters(std::vector<float>& node_centers, const float pmin[3], const float pmax[3], unsigned depth = 0) {
    size_t n = 0;
    int st = sbm_occ_unknown(t_, pmin, pmax, (int)depth, nullptr, 0, &n);   // the count
    if (st != SBM_OK && !(st == SBM_ERR_SIZE && n > 0)) check(st);
    const size_t at = node_centers.size();
    node_centers.resize(at + 3 * n);
    check(sbm_occ_unknown(t_, pmin, pmax, (int)depth, node_centers.data() + at, n, &n));
  }
  void getMetricMin(double& x, double& y, double& z) {
    double lo[3], hi[3];
    check(sbm_occ_metric(t_, lo, hi));
    x = lo[0], y = lo[1], z = lo[2];
  }
  void getMetricMax(double& x, double& y, double& z) {
    double lo[3], hi[3];
    check(sbm_occ_metric(t_, lo, hi));
    x = hi[0], y = hi[1], z = hi[2];
  }
  void getMetricSize(double& x, double& y, double& z) {
    double minX, minY, minZ, maxX, maxY, maxZ;
    getMetricMax(maxX, maxY, maxZ);
    getMetricMin(minX, minY, minZ);
    x = maxX - minX;
    y = maxY - minY;
    z = maxZ - minZ;
  }
  double volume() {
    double x, y, z;
    getMetricSize(x, y, z);
    return x * y * z;
  }
  // tree.writeBinary(path) of a SBM_OCC_TREE_MAXLIKELIHOOD tree
  void writeBinary(const std::string& path) { check(sbm_occ_tree_write_binary(t_, path.c_str())); }
  // tree.write(path) of a SBM_OCC_TREE_LOGODDS tree: the .ot file, every node's float
  void write(const std::string& path) { check(sbm_occ_ot_write(t_, path.c_str())); }
  // ColorOcTree: begin_leafs(maxDepth) with every entry's colour word (r | g << 8 | b << 16; white: none set), octomap's after
  // prune(); updateInnerOccupancy(), and tree.write(path) with `id ColorOcTree`
  std::vector<OccupancyLeaf> leavesColors(std::vector<uint32_t>& colors, unsigned max_depth = 0) {
    return listed([&](uint64_t* k, int32_t* d, float* v, size_t cap, size_t* n) {   // a count, then one listing with the colours
      if (cap) colors.assign(cap, SBM_OCC_COLOR_WHITE);
      else colors.clear();
      return sbm_occ_color_leaves(t_, (int)max_depth, k, d, v, cap ? colors.data() : nullptr, cap, n);
    });
  }
  void writeColor(const std::string& path) { check(sbm_occ_color_ot_write(t_, path.c_str())); }
  // of a snapshot over a map with stamps, octomap's STAMPED pruned tree: begin_leafs(maxDepth) with getTimestamp() of every entry,
  // getLastUpdateTime() (the root's stamp), and tree.write(path) with `id OcTreeStamped`
  std::vector<OccupancyLeaf> leavesStamped(std::vector<uint32_t>& stamps, unsigned max_depth = 0) {
    std::vector<OccupancyLeaf> out = leaves(max_depth);
    std::vector<uint64_t> keys(out.size());
    std::vector<int32_t> depth(out.size());
    stamps.assign(out.size(), 0u);
    size_t n = 0;
    check(sbm_occ_stamp_leaves(t_, (int)max_depth, keys.data(), depth.data(), nullptr, stamps.data(), out.size(), &n));
    return out;
  }
  unsigned int getLastUpdateTime() {
    uint32_t s = 0;
    check(sbm_occ_stamp_root(t_, &s));
    return s;
  }
  void writeStamped(const std::string& path) { check(sbm_occ_stamp_ot_write(t_, path.c_str())); }

 private:
  static void check(int st) {
    if (st != SBM_OK) throw Error(st, sbm_strerror(st));
  }
  // a listing call run twice: for its count, then into arrays of that size
  template <class Call> std::vector<OccupancyLeaf> listed(Call call) {
    size_t n = 0;
    int st = call(nullptr, nullptr, nullptr, 0, &n);
    if (st != SBM_OK && !(st == SBM_ERR_SIZE && n > 0)) check(st);
    std::vector<uint64_t> k(n);
    std::vector<int32_t> d(n);
    std::vector<float> v(n);
    check(call(k.data(), d.data(), v.data(), n, &n));
    std::vector<OccupancyLeaf> out(n);
    for (size_t i = 0; i < n; i++) out[i] = OccupancyLeaf{k[i], d[i], v[i]};
    return out;
  }
  float thres_;
  sbm_occ_tree* t_ = nullptr;
};

class OccupancyMap {
 public:
  // octomap::OcTree tree(resolution) and the reference's rangeMax_ (0.1, 5.0f); capacity in voxels
  explicit OccupancyMap(size_t capacity, double resolution = 0.1, float range_max = 5.0f, int device = 0) {
    sbm_occ_params_default(&p_);
    sbm_occ_ray_params_default(&rp_);
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

  // ---- log-odds mode: a map whose first insert is one of these holds a float log-odds per voxel, free space included ---------
  // octomap's probabilities; rayParams().max_range is insertPointCloud's maxrange for insertRays (negative: no limit)
  sbm_occ_ray_params& rayParams() { return rp_; }
  // tree.insertPointCloud(scan, sensor_origin, maxrange): n float triples in host memory
  // lazy_eval only defers octomap's inner nodes, which the map does not hold: accepted and ignored. discretize casts one ray
  // per end voxel instead of one per point (computeDiscreteUpdate).
  void insertPointCloud(const float* xyz, size_t n, const float origin[3], double maxrange = -1., bool lazy_eval = false,
                        bool discretize = false) {
    (void)lazy_eval;
    sbm_occ_ray_params rp = rp_;
    rp.max_range = maxrange;
    check(discretize ? sbm_occ_insert_cloud_discrete(m_, n, xyz, origin, &rp) : sbm_occ_insert_cloud(m_, n, xyz, origin, &rp));
  }
  // One node as insert() takes it, ray-cast from the sensorOrigin the reference computes (main.cpp:520) and never uses: the
  // pose's translation.
  void insertRays(const int16_t* disp, int width, int height, int scale, const sbm_stereo_model& model, const float pose[12],
                  bool lazy_eval = false, bool discretize = false) {
    (void)lazy_eval;
    check(discretize ? sbm_occ_insert_rays_discrete(m_, 1, disp, width, height, scale, &model, pose, &rp_)
                     : sbm_occ_insert_rays(m_, 1, disp, width, height, scale, &model, pose, &rp_));
  }
  void insertRaysDevice(int n, const void* d_disp, int width, int height, int scale, const sbm_stereo_model& model,
                        const float* poses, bool sync = true, bool lazy_eval = false, bool discretize = false) {
    (void)lazy_eval;
    check(discretize ? sbm_occ_insert_rays_discrete_device(m_, n, d_disp, width, height, scale, &model, poses, &rp_, sync ? 1 : 0)
                     : sbm_occ_insert_rays_device(m_, n, d_disp, width, height, scale, &model, poses, &rp_, sync ? 1 : 0));
  }

  // ---- insert options of the log-odds mode, in octomap's spelling (sbm.h, "occupancy map: insert options") -------------------
  // A point without a key throws (SBM_ERR_SIZE) and leaves the box as it was, where octomap logs an error.
  void setBBXMin(const float min[3]) {
    const Box b = box();
    check(sbm_occ_set_bbx(m_, min, b.max));
  }
  void setBBXMax(const float max[3]) {
    const Box b = box();
    check(sbm_occ_set_bbx(m_, b.min, max));
  }
  void useBBXLimit(bool enable) { check(sbm_occ_use_bbx_limit(m_, enable ? 1 : 0)); }
  bool bbxSet() { return box().enabled != 0; }
  void getBBXMin(float min[3]) {
    const Box b = box();
    min[0] = b.min[0], min[1] = b.min[1], min[2] = b.min[2];
  }
  void getBBXMax(float max[3]) {
    const Box b = box();
    max[0] = b.max[0], max[1] = b.max[1], max[2] = b.max[2];
  }
  // inBBX(point): in float, both bounds inclusive; inBBX(key): by key, both inclusive
  bool inBBX(const float p[3]) {
    const Box b = box();
    return p[0] >= b.min[0] && p[1] >= b.min[1] && p[2] >= b.min[2] && p[0] <= b.max[0] && p[1] <= b.max[1] && p[2] <= b.max[2];
  }
  bool inBBX(const uint16_t key[3]) {
    const Box b = box();
    return key[0] >= b.min_key[0] && key[1] >= b.min_key[1] && key[2] >= b.min_key[2] && key[0] <= b.max_key[0] &&
           key[1] <= b.max_key[1] && key[2] <= b.max_key[2];
  }
  void enableChangeDetection(bool enable) { check(sbm_occ_enable_change_detection(m_, enable ? 1 : 0)); }
  bool isChangeDetectionEnabled() {
    int on = 0;
    check(sbm_occ_change_detection_enabled(m_, &on));
    return on != 0;
  }
  void resetChangeDetection() { check(sbm_occ_reset_change_detection(m_)); }
  size_t numChangesDetected() {
    size_t n = 0;
    check(sbm_occ_num_changes(m_, &n));
    return n;
  }
  // changedKeysBegin() .. changedKeysEnd() as (packed key, created) pairs ascending by key: created is octomap's true, a voxel
  // whose occupancy flipped its false
  std::vector<std::pair<uint64_t, bool>> changedKeys() {
    std::vector<uint64_t> k(numChangesDetected());
    std::vector<uint8_t> c(k.size());
    size_t n = 0;
    check(sbm_occ_fetch_changes(m_, k.data(), c.data(), k.size(), &n));
    std::vector<std::pair<uint64_t, bool>> out(n);
    for (size_t i = 0; i < n; i++) out[i] = std::make_pair(k[i], c[i] != 0);
    return out;
  }
  // ---- growth (sbm.h, "occupancy map: growth"): octomap never reports a full map ------------------------------------------------
  // reserve() moves the map into a table for at least `capacity` voxels and keeps everything it holds; setGrowth(true) lets
  // every insert and load do so when it needs to, up to max_capacity voxels (0: the create limit), instead of SBM_ERR_OCC_FULL.
  void reserve(size_t capacity) { check(sbm_occ_reserve(m_, capacity)); }
  size_t capacity() {
    size_t n = 0;
    check(sbm_occ_capacity(m_, &n));
    return n;
  }
  void setGrowth(bool enable, size_t max_capacity = 0) { check(sbm_occ_set_growth(m_, enable ? 1 : 0, max_capacity)); }
  sbm_occ_growth_info growth() {
    sbm_occ_growth_info g;
    check(sbm_occ_get_growth(m_, &g));
    return g;
  }
  // ---- edits by key (sbm.h, "occupancy map: edit voxels by key"), in octomap's spelling ----------------------------------------------
  // Keys are packed k0 << 32 | k1 << 16 | k2 (packKey). lazy_eval only defers octomap's inner nodes: accepted and ignored. Where
  // octomap returns NULL or false for a point without a key, nothing happens here either. The clamps and the threshold are those
  // of rayParams().
  static uint64_t packKey(const uint16_t key[3]) { return (uint64_t)key[0] << 32 | (uint64_t)key[1] << 16 | key[2]; }
  // tree.updateNode(key, log_odds_update) / updateNode(point, log_odds_update)
  void updateNode(uint64_t key, float log_odds_update, bool lazy_eval = false) {
    (void)lazy_eval;
    check(sbm_occ_edit(m_, 1, &key, nullptr, &log_odds_update, &rp_));
  }
  void updateNode(const float point[3], float log_odds_update, bool lazy_eval = false) {
    (void)lazy_eval;
    check(sbm_occ_edit_points(m_, 1, point, nullptr, &log_odds_update, &rp_));
  }
  // tree.updateNode(key, occupied) / updateNode(point, occupied): the hit or the miss log-odds of rayParams(), formed here
  void updateNode(uint64_t key, bool occupied, bool lazy_eval = false) { updateNode(key, hitOrMiss(occupied), lazy_eval); }
  void updateNode(const float point[3], bool occupied, bool lazy_eval = false) { updateNode(point, hitOrMiss(occupied), lazy_eval); }
  // the same for a batch, in item order: one update each, or one for all
  void updateNode(const std::vector<uint64_t>& keys, const std::vector<float>& log_odds_updates, bool lazy_eval = false) {
    (void)lazy_eval;
    if (keys.size() != log_odds_updates.size()) throw Error(SBM_ERR_SIZE, "updateNode: keys and updates differ in number");
    check(sbm_occ_edit(m_, keys.size(), keys.data(), nullptr, log_odds_updates.data(), &rp_));
  }
  void updateNode(const std::vector<uint64_t>& keys, bool occupied, bool lazy_eval = false) {
    updateNode(keys, std::vector<float>(keys.size(), hitOrMiss(occupied)), lazy_eval);
  }
  // points: n float triples
  void updateNode(const float* xyz, size_t n, const float* log_odds_updates, bool lazy_eval = false) {
    (void)lazy_eval;
    check(sbm_occ_edit_points(m_, n, xyz, nullptr, log_odds_updates, &rp_));
  }
  void updateNode(const float* xyz, size_t n, bool occupied, bool lazy_eval = false) {
    const std::vector<float> u(n, hitOrMiss(occupied));
    updateNode(xyz, n, u.data(), lazy_eval);
  }
  // tree.setNodeValue(key, log_odds_value) / setNodeValue(point, log_odds_value), and for a batch
  void setNodeValue(uint64_t key, float log_odds_value, bool lazy_eval = false) {
    (void)lazy_eval;
    const uint8_t op = SBM_OCC_EDIT_SET;
    check(sbm_occ_edit(m_, 1, &key, &op, &log_odds_value, &rp_));
  }
  void setNodeValue(const float point[3], float log_odds_value, bool lazy_eval = false) {
    (void)lazy_eval;
    const uint8_t op = SBM_OCC_EDIT_SET;
    check(sbm_occ_edit_points(m_, 1, point, &op, &log_odds_value, &rp_));
  }
  void setNodeValue(const std::vector<uint64_t>& keys, const std::vector<float>& log_odds_values, bool lazy_eval = false) {
    (void)lazy_eval;
    if (keys.size() != log_odds_values.size()) throw Error(SBM_ERR_SIZE, "setNodeValue: keys and values differ in number");
    const std::vector<uint8_t> ops(keys.size(), (uint8_t)SBM_OCC_EDIT_SET);
    check(sbm_occ_edit(m_, keys.size(), keys.data(), ops.data(), log_odds_values.data(), &rp_));
  }
  // mixed items in item order: ops SBM_OCC_EDIT_UPDATE / SET / DELETE (empty: all updates)
  void edit(const std::vector<uint64_t>& keys, const std::vector<uint8_t>& ops, const std::vector<float>& values) {
    if (keys.size() != values.size() || (!ops.empty() && ops.size() != keys.size())) throw Error(SBM_ERR_SIZE, "edit: arrays differ in number");
    check(sbm_occ_edit(m_, keys.size(), keys.data(), ops.empty() ? nullptr : ops.data(), values.data(), &rp_));
  }
  // tree.deleteNode(key, depth) / deleteNode(point, depth): depth 0 means 16; always true where octomap says whether a node went
  bool deleteNode(uint64_t key, unsigned depth = 0) {
    check(sbm_occ_delete(m_, 1, &key, (int)depth));
    return true;
  }
  bool deleteNode(const float point[3], unsigned depth = 0) {
    uint64_t key;
    if (!coordToKeyChecked(point, &key)) return false;
    return deleteNode(key, depth);
  }
  bool deleteNode(const std::vector<uint64_t>& keys, unsigned depth = 0) {
    check(sbm_occ_delete(m_, keys.size(), keys.data(), (int)depth));
    return true;
  }
  // The loop octomap's users write over a box -- for every leaf with inBBX(key): deleteNode(key) -- with these bounds, both
  // inclusive; outside = true removes everything else instead: the sliding window around the robot. The insert's box stays.
  void deleteBBX(const uint16_t min[3], const uint16_t max[3], bool outside = false) { check(sbm_occ_delete_box(m_, min, max, outside ? 1 : 0)); }
  void deleteBBX(const float min[3], const float max[3], bool outside = false) {
    uint64_t lo, hi;
    if (!coordToKeyChecked(min, &lo) || !coordToKeyChecked(max, &hi)) throw Error(SBM_ERR_SIZE, "deleteBBX: a bound has no key");
    const uint16_t a[3] = {(uint16_t)(lo >> 32), (uint16_t)(lo >> 16), (uint16_t)lo}, b[3] = {(uint16_t)(hi >> 32), (uint16_t)(hi >> 16), (uint16_t)hi};
    deleteBBX(a, b, outside);
  }
  // coordToKeyChecked(point, key): the packed key of a point, false where it has none
  bool coordToKeyChecked(const float point[3], uint64_t* key) const {
    uint64_t k = 0;
    for (int i = 0; i < 3; i++) {
      const double f = std::floor((1. / p_.resolution) * (double)point[i]);
      if (!(f >= -32768.0 && f < 32768.0)) return false;
      k = k << 16 | (uint64_t)((int)f + 32768);
    }
    *key = k;
    return true;
  }
  // items, skipped, lost to a full table, voxels created and removed by the last edit or delete call
  sbm_occ_edit_info lastEdit() {
    sbm_occ_edit_info e;
    check(sbm_occ_last_edit(m_, &e));
    return e;
  }
  // the stored voxels ascending by packed key with their log-odds
  std::vector<uint64_t> leaves(std::vector<float>& logodds) {
    std::vector<uint64_t> k(size());
    logodds.assign(k.size(), 0.f);
    size_t n = 0;
    check(sbm_occ_fetch_logodds(m_, k.data(), logodds.data(), k.size(), &n));
    k.resize(n);
    logodds.resize(n);
    return k;
  }
  // tree.writeBinary(path) of a log-odds map: free and occupied leaves, thresholded at rayParams().occupancy_thres
  void writeBinaryLogOdds(const std::string& path) {
    std::vector<float> v;
    const std::vector<uint64_t> k = leaves(v);
    float c[5];
    check(sbm_occ_ray_logodds(&rp_, c));
    check(sbm_occ_write_binary_logodds(k.data(), v.data(), k.size(), p_.resolution, c[4], path.c_str()));
  }

  // tree.readBinary(filename) / tree.readBinary(stream): the map becomes what the .bt holds -- occupied leaves at the clamp max of
  // rayParams(), free leaves at its clamp min, expanded to voxels on the device -- whatever it held before; further
  // insertPointCloud / insertRays scans continue on it. octomap returns false where this throws (SBM_ERR_SIZE for a malformed
  // stream or another resolution, SBM_ERR_UNSUPPORTED for a file that cannot be read or is no OcTree .bt, SBM_ERR_OCC_FULL for a
  // map too small), and then the map is as it was.
  bool readBinary(const std::string& filename) {
    check(sbm_occ_read_binary(m_, filename.c_str(), &rp_, 1));
    return true;
  }
  bool readBinary(const void* bytes, size_t n) {
    check(sbm_occ_load_binary(m_, bytes, n, &rp_, 1));
    return true;
  }

  // tree.write(path): the .ot file of a log-odds map as it is now, which keeps every voxel's log-odds (a .bt keeps which clamp
  // it is nearer to)
  void write(const std::string& path) { buildTree(SBM_OCC_TREE_LOGODDS)->write(path); }
  // AbstractOcTree::read(filename) / read(stream) for an OcTree: the map becomes what the .ot holds, every voxel its leaf's float,
  // unclamped, whatever it held before; further insertPointCloud / insertRays scans continue on it. octomap returns NULL where
  // this throws (the codes of readBinary above, and SBM_ERR_UNSUPPORTED for a leaf value that is not finite), and then the map is
  // as it was.
  bool read(const std::string& filename) {
    check(sbm_occ_ot_read(m_, filename.c_str(), 1));
    return true;
  }
  bool read(const void* bytes, size_t n) {
    check(sbm_occ_ot_load(m_, bytes, n, 1));
    return true;
  }

  // ---- ColorOcTree: a colour per voxel of a log-odds map (include/sbm.h, "occupancy map: colour per voxel") ----------------------
  // tree.setNodeColor(key, r, g, b) / averageNodeColor(key, r, g, b): true where octomap returns the node, false where its search
  // finds none (nothing happens then). White (255, 255, 255) is "no colour set". integrateNodeColor is not provided.
  static uint32_t packColor(uint8_t r, uint8_t g, uint8_t b) { return (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16; }
  bool setNodeColor(uint64_t key, uint8_t r, uint8_t g, uint8_t b) { return colorOne(&key, nullptr, packColor(r, g, b), SBM_OCC_COLOR_SET); }
  bool setNodeColor(const float point[3], uint8_t r, uint8_t g, uint8_t b) { return colorOne(nullptr, point, packColor(r, g, b), SBM_OCC_COLOR_SET); }
  bool averageNodeColor(uint64_t key, uint8_t r, uint8_t g, uint8_t b) { return colorOne(&key, nullptr, packColor(r, g, b), SBM_OCC_COLOR_AVERAGE); }
  bool averageNodeColor(const float point[3], uint8_t r, uint8_t g, uint8_t b) {
    return colorOne(nullptr, point, packColor(r, g, b), SBM_OCC_COLOR_AVERAGE);
  }
  // batches in item order: the loop a user writes over a coloured cloud, in one call
  void setNodeColor(const std::vector<uint64_t>& keys, const std::vector<uint32_t>& colors) {
    if (keys.size() != colors.size()) throw Error(SBM_ERR_SIZE, "setNodeColor: keys and colors differ in length");
    check(sbm_occ_color_keys(m_, keys.size(), keys.data(), colors.data(), SBM_OCC_COLOR_SET));
  }
  void averageNodeColor(const std::vector<uint64_t>& keys, const std::vector<uint32_t>& colors) {
    if (keys.size() != colors.size()) throw Error(SBM_ERR_SIZE, "averageNodeColor: keys and colors differ in length");
    check(sbm_occ_color_keys(m_, keys.size(), keys.data(), colors.data(), SBM_OCC_COLOR_AVERAGE));
  }
  void setNodeColor(const float* xyz, size_t n, const uint32_t* colors) { check(sbm_occ_color_points(m_, n, xyz, colors, SBM_OCC_COLOR_SET)); }
  void averageNodeColor(const float* xyz, size_t n, const uint32_t* colors) { check(sbm_occ_color_points(m_, n, xyz, colors, SBM_OCC_COLOR_AVERAGE)); }
  sbm_occ_color_info lastColor() {
    sbm_occ_color_info i;
    check(sbm_occ_color_last(m_, &i));
    return i;
  }
  // tree.search(x, y, z) of a ColorOcTree: the state, and the node's log-odds and colour word (white where there is no node)
  int search(float x, float y, float z, float* logodds, uint32_t* color) {
    const float p[3] = {x, y, z};
    int32_t state = 0;
    check(sbm_occ_color_search(m_, 1, p, occupancyThresLog(), &state, logodds, color));
    return state;
  }
  void search(const float* xyz, size_t n, int32_t* states, void* values, uint32_t* colors) {
    check(sbm_occ_color_search(m_, n, xyz, occupancyThresLog(), states, values, colors));
  }
  // tree.write(path) of a ColorOcTree as the map is now, and AbstractOcTree::read of one: every voxel its leaf's float and colour.
  // octomap colours a whole pruned leaf after read() where this map colours one voxel, unless expand() is called there first.
  void writeColor(const std::string& path) { buildTree(SBM_OCC_TREE_LOGODDS)->writeColor(path); }
  bool readColor(const std::string& filename) {
    check(sbm_occ_color_ot_read(m_, filename.c_str(), 1));
    return true;
  }
  bool readColor(const void* bytes, size_t n) {
    check(sbm_occ_color_ot_load(m_, bytes, n, 1));
    return true;
  }

  // ---- time stamps per voxel, in octomap's spelling (OcTreeStamped; sbm.h, "occupancy map: time stamps per voxel") -----------
  // OcTreeStamped reads time(NULL); this map has a clock of its own, which the caller sets: every updateNode of an insert or an
  // edit stamps its voxel with time() unless octomap's early return applies. A map holds colours or stamps, not both. The
  // tree snapshot of such a map is octomap's stamped pruned tree (OccupancyTree::leavesStamped, getLastUpdateTime, writeStamped).
  void enableStamps() { check(sbm_occ_stamp_enable(m_)); }
  bool stampsEnabled() {
    int on = 0;
    check(sbm_occ_stamp_enabled(m_, &on));
    return on != 0;
  }
  void setTime(uint32_t clock) { check(sbm_occ_stamp_set_time(m_, clock)); }
  uint32_t time() {
    uint32_t c = 0;
    check(sbm_occ_stamp_time(m_, &c));
    return c;
  }
  // tree.degradeOutdatedNodes(time_thres) -> how many voxels got the miss update
  uint64_t degradeOutdatedNodes(unsigned int time_thres) {
    uint64_t n = 0;
    check(sbm_occ_stamp_degrade(m_, time_thres, &rp_, &n));
    return n;
  }
  // not octomap: deletes every voxel whose stamp is more than time_thres behind the clock -> how many
  uint64_t forgetOlderThan(unsigned int time_thres) {
    uint64_t n = 0;
    check(sbm_occ_stamp_forget(m_, time_thres, &n));
    return n;
  }
  // tree.search(x, y, z) of an OcTreeStamped: the state, and the node's log-odds and getTimestamp() (0 where there is no node)
  int searchStamped(float x, float y, float z, float* logodds, uint32_t* stamp) {
    const float p[3] = {x, y, z};
    int32_t state = 0;
    check(sbm_occ_stamp_search(m_, 1, p, occupancyThresLog(), &state, logodds, stamp));
    return state;
  }
  void searchStamped(const float* xyz, size_t n, int32_t* states, void* values, uint32_t* stamps) {
    check(sbm_occ_stamp_search(m_, n, xyz, occupancyThresLog(), states, values, stamps));
  }
  // the voxels in ascending order of their packed keys, with log-odds and stamps
  std::vector<uint64_t> leavesStamped(std::vector<float>& logodds, std::vector<uint32_t>& stamps) {
    std::vector<uint64_t> keys(size());
    logodds.resize(keys.size());
    stamps.resize(keys.size());
    size_t n = 0;
    check(sbm_occ_stamp_fetch(m_, keys.data(), logodds.data(), stamps.data(), keys.size(), &n));
    keys.resize(n), logodds.resize(n), stamps.resize(n);
    return keys;
  }

  // tree.write(path) of an OcTreeStamped as the map is now, and AbstractOcTree::read of one: stamps 0 everywhere afterwards
  void writeStamped(const std::string& path) { buildTree(SBM_OCC_TREE_LOGODDS)->writeStamped(path); }
  bool readStamped(const std::string& filename) {
    check(sbm_occ_stamp_ot_read(m_, filename.c_str(), 1));
    return true;
  }
  bool readStamped(const void* bytes, size_t n) {
    check(sbm_occ_stamp_ot_load(m_, bytes, n, 1));
    return true;
  }

  // ---- queries: the map is not changed ---------------------------------------------------------------------------------------
  // The threshold of isNodeOccupied for a log-odds map: logodds(rayParams().occupancy_thres)
  float occupancyThresLog() const {
    float c[5];
    check(sbm_occ_ray_logodds(&rp_, c));
    return c[4];
  }
  // tree.search(x, y, z): SBM_OCC_CELL_OUT / UNKNOWN / FREE / OCCUPIED; *logodds (may be null) receives the node's log-odds,
  // NaN where there is no node (a log-odds map; in hit mode the word is the hit count)
  int search(float x, float y, float z, float* logodds = nullptr) {
    const float p[3] = {x, y, z};
    int32_t state = 0;
    check(sbm_occ_search(m_, 1, p, occupancyThresLog(), &state, logodds));
    return state;
  }
  // n points (host memory) at once: states, and the 4-byte value words where values is not null
  void search(const float* xyz, size_t n, int32_t* states, void* values = nullptr) {
    check(sbm_occ_search(m_, n, xyz, occupancyThresLog(), states, values));
  }
  // tree.castRay(origin, direction, end, ignoreUnknownCells, maxRange): true iff the ray hit an occupied voxel, whose centre is
  // then in end. Where octomap leaves end untouched (no key for the origin, no direction) so does this.
  bool castRay(const float origin[3], const float direction[3], float end[3], bool ignoreUnknownCells = false, double maxRange = -1.0,
               int* status = nullptr) {
    const sbm_occ_query_params q = queryParams(ignoreUnknownCells, maxRange);
    int32_t st = 0;
    float e[3];
    check(sbm_occ_cast_rays(m_, 1, origin, 1, direction, &q, &st, e));
    if (st != SBM_OCC_RAY_NONE) end[0] = e[0], end[1] = e[1], end[2] = e[2];
    if (status) *status = st;
    return st == SBM_OCC_RAY_HIT;
  }
  // n rays in host memory: origins n triples, or one that every ray starts from (one_origin); ends may be null
  void castRays(const float* origins, bool one_origin, const float* directions, size_t n, int32_t* status, float* ends,
                bool ignoreUnknownCells = false, double maxRange = -1.0) {
    const sbm_occ_query_params q = queryParams(ignoreUnknownCells, maxRange);
    check(sbm_occ_cast_rays(m_, n, origins, one_origin ? 1 : 0, directions, &q, status, ends));
  }
  // tree.getRayIntersection(origin, direction, center, intersection, delta): true iff the (un-normalised) ray's line enters the
  // voxel around center, at intersection; where octomap leaves intersection untouched so does this.
  bool getRayIntersection(const float origin[3], const float direction[3], const float center[3], float intersection[3], double delta = 0.0) {
    int32_t found = 0;
    float p[3];
    check(sbm_occ_ray_intersections(m_, 1, origin, 1, direction, center, delta, p, &found));
    if (found) intersection[0] = p[0], intersection[1] = p[1], intersection[2] = p[2];
    return found != 0;
  }
  // n rays in host memory: origins n triples, or one that every ray starts from (one_origin); a ray that is not found leaves a NaN
  // triple; found may be null
  void getRayIntersections(const float* origins, bool one_origin, const float* directions, const float* centers, size_t n,
                           float* intersections, int32_t* found = nullptr, double delta = 0.0) {
    check(sbm_occ_ray_intersections(m_, n, origins, one_origin ? 1 : 0, directions, centers, delta, intersections, found));
  }
  // One ray per pixel of a width x height virtual camera at `pose`, into DEVICE memory (d_end may be null)
  void castView(int width, int height, int scale, const sbm_stereo_model& model, const float pose[12], void* d_status, void* d_end,
                bool ignoreUnknownCells = false, double maxRange = -1.0, bool sync = true) {
    const sbm_occ_query_params q = queryParams(ignoreUnknownCells, maxRange);
    check(sbm_occ_cast_view_device(m_, width, height, scale, &model, pose, &q, d_status, d_end, sync ? 1 : 0));
  }

  // The tree above the voxels as they are now (a snapshot; rebuild() it after further inserts). The default reading is what
  // writeBinary holds; SBM_OCC_TREE_LOGODDS keeps the log-odds of a log-odds map.
  std::unique_ptr<OccupancyTree> buildTree(int reading = SBM_OCC_TREE_MAXLIKELIHOOD) {
    std::unique_ptr<OccupancyTree> t(new OccupancyTree(m_, occupancyThresLog()));
    t->rebuild(reading, rp_);
    return t;
  }

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
  sbm_occ_query_params queryParams(bool ignoreUnknownCells, double maxRange) const {
    sbm_occ_query_params q;
    sbm_occ_query_params_default(&q);
    q.max_range = maxRange;
    q.occupancy_thres_log = occupancyThresLog();
    q.ignore_unknown = ignoreUnknownCells ? 1 : 0;
    return q;
  }
  bool colorOne(const uint64_t* key, const float* point, uint32_t color, int op) {
    check(key ? sbm_occ_color_keys(m_, 1, key, &color, op) : sbm_occ_color_points(m_, 1, point, &color, op));
    return lastColor().found == 1;
  }
  float hitOrMiss(bool occupied) const {
    float c[5];
    check(sbm_occ_ray_logodds(&rp_, c));
    return occupied ? c[0] : c[1];
  }
  struct Box {
    float min[3], max[3];
    uint16_t min_key[3], max_key[3];
    int enabled;
  };
  Box box() {
    Box b;
    check(sbm_occ_get_bbx(m_, b.min, b.max, b.min_key, b.max_key, &b.enabled));
    return b;
  }
  static void check(int st) {
    if (st != SBM_OK) throw Error(st, sbm_strerror(st));
  }
  sbm_occ_params p_;
  sbm_occ_ray_params rp_;
  sbm_handle* h_ = nullptr;
  sbm_occ_map* m_ = nullptr;
};

}  // namespace sbm

#endif  // SBM_OCCUPANCY_HPP_
