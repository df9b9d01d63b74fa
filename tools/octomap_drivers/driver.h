// Shared by the drivers of tools/make_occupancy_*_fixtures.py: the record protocol between a generator and its driver, driver
// side (tools/octomap_kit.py holds the other side). This project's text; it calls octomap's API only.
//
// Everything is little-endian and unpadded. A generator writes <tag>.in, the driver answers in <tag>.out:
//   head      five doubles (prob_hit, prob_miss, clamp_min, clamp_max, occupancy_thres), double resolution
//   scan      float origin[3], double max_range, int32 n, float points[3 n]        -> insertPointCloud
//   scans     int32 count, that many scans
//   points    int32 n, float points[3 n]
//   hits      int32 n, uint16 keys[3 n], uint32 counts[n]                           -> updateNode(key, true), counts[i] times
//   stream    uint32 n, n bytes (either direction)
//   node      uint16 key[3], uint16 depth, float log-odds (out); leaves: uint32 n, n nodes
#pragma once
#include <octomap/octomap.h>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

typedef std::chrono::steady_clock Clock;
static inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T> static void wr(FILE* f, const T& v) { fwrite(&v, sizeof(T), 1, f); }

// driver <in> <out>
static inline bool open_files(int argc, char** argv, FILE*& in, FILE*& out) {
  if (argc != 3) return false;
  in = fopen(argv[1], "rb");
  out = fopen(argv[2], "wb");
  return in && out;
}

static inline bool head_in(FILE* in, double* prob, double* resolution) { return rd(in, prob, 5) && rd(in, resolution, 1); }

static inline void set_params(octomap::OcTree& tree, const double* prob) {
  tree.setProbHit(prob[0]);
  tree.setProbMiss(prob[1]);
  tree.setClampingThresMin(prob[2]);
  tree.setClampingThresMax(prob[3]);
  tree.setOccupancyThres(prob[4]);
}

// the five log-odds constants a tree made of its probabilities
static inline void constants_out(const octomap::OcTree& tree, FILE* out) {
  float constants[5] = {tree.getProbHitLog(), tree.getProbMissLog(), tree.getClampingThresMinLog(), tree.getClampingThresMaxLog(),
                        tree.getOccupancyThresLog()};
  fwrite(constants, 4, 5, out);
}

static inline bool points_in(FILE* in, std::vector<float>& pts) {
  int32_t n;
  if (!rd(in, &n, 1)) return false;
  pts.resize(3 * (size_t)n);
  return rd(in, pts.data(), pts.size());
}

struct Scan {
  octomap::point3d origin;
  double max_range;
  octomap::Pointcloud cloud;
};

static inline bool scan_read(FILE* in, Scan& s) {
  float o[3];
  std::vector<float> pts;
  if (!rd(in, o, 3) || !rd(in, &s.max_range, 1) || !points_in(in, pts)) return false;
  s.origin = octomap::point3d(o[0], o[1], o[2]);
  for (size_t i = 0; i < pts.size(); i += 3) s.cloud.push_back(pts[i], pts[i + 1], pts[i + 2]);
  return true;
}

static inline bool scan_in(FILE* in, octomap::OcTree& tree) {
  Scan s;
  if (!scan_read(in, s)) return false;
  tree.insertPointCloud(s.cloud, s.origin, s.max_range);
  return true;
}

static inline bool scans_in(FILE* in, octomap::OcTree& tree) {
  int32_t n;
  if (!rd(in, &n, 1)) return false;
  for (int s = 0; s < n; s++)
    if (!scan_in(in, tree)) return false;
  return true;
}

static inline bool hits_in(FILE* in, octomap::OcTree& tree) {
  int32_t n;
  if (!rd(in, &n, 1)) return false;
  std::vector<uint16_t> k(3 * (size_t)n);
  std::vector<uint32_t> c(n);
  if (!rd(in, k.data(), k.size()) || !rd(in, c.data(), c.size())) return false;
  for (int i = 0; i < n; i++)
    for (uint32_t j = 0; j < c[i]; j++) tree.updateNode(octomap::OcTreeKey(k[3 * i], k[3 * i + 1], k[3 * i + 2]), true);
  return true;
}

static inline bool stream_in(FILE* in, std::string& s) {
  uint32_t n;
  if (!rd(in, &n, 1)) return false;
  s.assign(n, '\0');
  return rd(in, &s[0], n);
}

static inline void stream_out(const std::string& s, FILE* out) {
  wr(out, (uint32_t)s.size());
  fwrite(s.data(), 1, s.size(), out);
}

static inline void node_out(FILE* out, const octomap::OcTreeKey& k, unsigned depth, float value) {
  uint16_t w[4] = {k[0], k[1], k[2], (uint16_t)depth};
  fwrite(w, 2, 4, out);
  wr(out, value);
}

// begin_leafs() as nodes; false at a leaf that is not at depth `only`, where one is asked for
static inline bool leaves_out(const octomap::OcTree& tree, FILE* out, unsigned only = 0) {
  uint32_t n = 0;
  for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) n++;
  wr(out, n);
  for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) {
    if (only && it.getDepth() != only) return false;
    node_out(out, it.getKey(), it.getDepth(), it->getLogOdds());
  }
  return true;
}

// the voxels, keys and values apart: uint32 n, uint16 keys[3 n], float log-odds[n], of the depth-16 leaves of an expanded copy
static inline bool voxels_out(const octomap::OcTree& tree, FILE* out, bool count_only = false) {
  octomap::OcTree copy(tree);
  copy.expand();
  std::vector<uint16_t> keys;
  std::vector<float> values;
  for (octomap::OcTree::leaf_iterator it = copy.begin_leafs(), end = copy.end_leafs(); it != end; ++it) {
    if (it.getDepth() != 16) return false;
    octomap::OcTreeKey k = it.getKey();
    keys.push_back(k[0]);
    keys.push_back(k[1]);
    keys.push_back(k[2]);
    values.push_back(it->getLogOdds());
  }
  wr(out, (uint32_t)values.size());
  if (count_only) return true;
  fwrite(keys.data(), 2, keys.size(), out);
  fwrite(values.data(), 4, values.size(), out);
  return true;
}

// search(point) per point: int32 found, float log-odds
static inline void search_out(octomap::OcTree& tree, const std::vector<float>& pts, FILE* out) {
  for (size_t i = 0; i < pts.size(); i += 3) {
    octomap::OcTreeNode* node = tree.search(octomap::point3d(pts[i], pts[i + 1], pts[i + 2]));
    wr(out, (int32_t)(node ? 1 : 0));
    wr(out, (float)(node ? node->getLogOdds() : 0.f));
  }
}
