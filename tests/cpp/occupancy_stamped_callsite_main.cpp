// A long-running mapper's map over include/sbm_occupancy.hpp in octomap's spelling (OcTreeStamped): it replays a recorded case
// (tests/occupancy_stamped_cases.py describes the steps) on a map with stamps enabled, setting the map's clock before every step.
// A failure prints "error <code>" and exits with 4.
//
//   occupancy_stamped_callsite_main <steps.bin> <capacity> <answers.bin> <stream prefix>
//
// steps.bin: double prob_hit, prob_miss, clamp_min, clamp_max, occupancy_thres, max_range, int32 steps; per step int32 kind,
// uint32 clock, int32 n, int32 flags, uint32 time_thres, float origin[3], float box[6], uint64 keys[n], float points[3 n],
// float values[n], uint8 ops[n]. Kind 0 insertPointCloud (flags: 1 discretize, 2 useBBXLimit with the box, 4
// enableChangeDetection), 1 edit(keys, ops, values), 2 degradeOutdatedNodes(time_thres), 3 forgetOlderThan(time_thres), 4 a snapshot:
// buildTree(LOGODDS), its begin_leafs() with stamps, getLastUpdateTime() and writeStamped(<prefix><step>), 5 writeStamped, readStamped.
// answers.bin, per step: uint64 count (what kind 2 or 3 returned, else 0), uint32 m, uint64 key[m], float value[m], uint32
// stamp[m] of leavesStamped(), then int32 state, float value, uint32 stamp of searchStamped at the first voxel's centre (three
// zero words for an empty map). After a snapshot's record: uint32 m, uint64 key[m], int32 depth[m], float value[m], uint32 stamp[m] of
// the tree's leavesStamped(), and uint32 getLastUpdateTime().
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "sbm_occupancy.hpp"

template <class T> static bool take(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[3], "wb");
  double p[6];
  int32_t steps;
  if (!in || !out || std::fread(p, 8, 6, in) != 6 || std::fread(&steps, 4, 1, in) != 1) return 3;
  try {
    sbm::OccupancyMap tree((size_t)std::atoll(argv[2]), 0.1);
    sbm_occ_ray_params& rp = tree.rayParams();
    rp.prob_hit = p[0], rp.prob_miss = p[1], rp.clamp_min = p[2], rp.clamp_max = p[3], rp.occupancy_thres = p[4];
    tree.enableStamps();
    if (!tree.stampsEnabled()) return 5;
    for (int s = 0; s < steps; s++) {
      int32_t kind, n, flags;
      uint32_t clock, thres;
      float origin[3], box[6];
      std::vector<uint64_t> keys;
      std::vector<float> points, values;
      std::vector<uint8_t> ops;
      if (std::fread(&kind, 4, 1, in) != 1 || std::fread(&clock, 4, 1, in) != 1 || std::fread(&n, 4, 1, in) != 1 || std::fread(&flags, 4, 1, in) != 1 ||
          std::fread(&thres, 4, 1, in) != 1 || std::fread(origin, 4, 3, in) != 3 || std::fread(box, 4, 6, in) != 6)
        return 3;
      if (!take(in, keys, (size_t)n) || !take(in, points, 3 * (size_t)n) || !take(in, values, (size_t)n) || !take(in, ops, (size_t)n)) return 3;
      tree.setTime(clock);
      if (tree.time() != clock) return 5;
      uint64_t count = 0;
      if (kind == 0) {
        if (flags & 2) {
          tree.setBBXMin(box);
          tree.setBBXMax(box + 3);
        }
        tree.useBBXLimit((flags & 2) != 0);
        tree.enableChangeDetection((flags & 4) != 0);
        tree.insertPointCloud(points.data(), (size_t)n, origin, p[5], true, (flags & 1) != 0);
      } else if (kind == 1) {
        tree.edit(keys, ops, values);
      } else if (kind == 2) {
        count = tree.degradeOutdatedNodes(thres);
      } else if (kind == 3) {
        count = tree.forgetOlderThan(thres);
      } else if (kind == 5) {
        const std::string path = std::string(argv[4]) + std::to_string(s);
        tree.writeStamped(path);
        tree.readStamped(path);
      } else if (kind != 4) {
        return 3;
      }
      std::vector<float> lo;
      std::vector<uint32_t> stamps;
      const std::vector<uint64_t> k = tree.leavesStamped(lo, stamps);
      const uint32_t m = (uint32_t)k.size();
      std::fwrite(&count, 8, 1, out);
      std::fwrite(&m, 4, 1, out);
      std::fwrite(k.data(), 8, m, out);
      std::fwrite(lo.data(), 4, m, out);
      std::fwrite(stamps.data(), 4, m, out);
      int32_t state = 0;
      float value = 0.f;
      uint32_t stamp = 0;
      if (m) {
        const float c[3] = {(float)(((double)((int)(k[0] >> 32 & 0xFFFF) - 32768) + 0.5) * 0.1), (float)(((double)((int)(k[0] >> 16 & 0xFFFF) - 32768) + 0.5) * 0.1),
                            (float)(((double)((int)(k[0] & 0xFFFF) - 32768) + 0.5) * 0.1)};
        state = tree.searchStamped(c[0], c[1], c[2], &value, &stamp);
      }
      std::fwrite(&state, 4, 1, out);
      std::fwrite(&value, 4, 1, out);
      std::fwrite(&stamp, 4, 1, out);
      if (kind == 4) {
        std::unique_ptr<sbm::OccupancyTree> t = tree.buildTree(SBM_OCC_TREE_LOGODDS);
        std::vector<uint32_t> st;
        const std::vector<sbm::OccupancyLeaf> leaves = t->leavesStamped(st);
        const uint32_t n2 = (uint32_t)leaves.size(), root = t->getLastUpdateTime();
        std::fwrite(&n2, 4, 1, out);
        for (const sbm::OccupancyLeaf& l : leaves) std::fwrite(&l.key, 8, 1, out);
        for (const sbm::OccupancyLeaf& l : leaves) std::fwrite(&l.depth, 4, 1, out);
        for (const sbm::OccupancyLeaf& l : leaves) std::fwrite(&l.value, 4, 1, out);
        std::fwrite(st.data(), 4, st.size(), out);
        std::fwrite(&root, 4, 1, out);
        t->writeStamped(std::string(argv[4]) + std::to_string(s));
      }
    }
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  std::fclose(out);
  return 0;
}
