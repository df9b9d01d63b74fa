// A long-running mapper's two loops over include/sbm_occupancy.hpp in octomap's spelling: the sliding window (after every key
// frame, forget what lies outside a box around the robot) and the replay of another map's changedKeys (a second map follows
// the first through updateNode / setNodeValue by key). The cloud (per scan: a float count, three floats of origin, then the
// triples) is read from a file. Prints per scan "size <voxels> removed <n> mirror <voxels>", then "marked <state>" of a voxel the
// caller marked, cleared and deleted by hand; a failure prints "error <code>" and exits with 4.
//
//   occupancy_edit_callsite_main <cloud.raw> <floats> <capacity> <half window in voxels>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sbm_occupancy.hpp"

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  std::vector<float> cloud((size_t)std::atoll(argv[2]));
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(cloud.data(), sizeof(float), cloud.size(), f) != cloud.size()) return 3;
  std::fclose(f);
  const int half = std::atoi(argv[4]);
  try {
    sbm::OccupancyMap tree((size_t)std::atoll(argv[3]), 0.1), mirror((size_t)std::atoll(argv[3]), 0.1);
    tree.enableChangeDetection(true);
    for (size_t at = 0; at + 4 <= cloud.size();) {
      const size_t n = (size_t)cloud[at];
      const float* origin = cloud.data() + at + 1;
      tree.resetChangeDetection();
      tree.insertPointCloud(cloud.data() + at + 4, n, origin);
      // the replay: what changed in `tree` is set in `mirror`, by key
      std::vector<float> values;
      const std::vector<uint64_t> keys = tree.leaves(values);
      std::vector<uint64_t> changed;
      std::vector<float> changed_values;
      for (const std::pair<uint64_t, bool>& c : tree.changedKeys()) {
        size_t lo = 0, hi = keys.size();
        while (lo < hi) {
          const size_t mid = (lo + hi) / 2;
          if (keys[mid] < c.first) lo = mid + 1;
          else hi = mid;
        }
        if (lo == keys.size() || keys[lo] != c.first) return 5;
        changed.push_back(c.first);
        changed_values.push_back(values[lo]);
      }
      mirror.setNodeValue(changed, changed_values);
      // the window: everything outside the box around the robot goes, in both maps
      uint64_t at_key;
      if (!tree.coordToKeyChecked(origin, &at_key)) return 5;
      uint16_t lo[3], hi[3];
      for (int i = 0; i < 3; i++) {
        const int k = (int)(at_key >> (32 - 16 * i) & 0xFFFF);
        lo[i] = (uint16_t)(k - half < 0 ? 0 : k - half);
        hi[i] = (uint16_t)(k + half > 65535 ? 65535 : k + half);
      }
      tree.deleteBBX(lo, hi, true);
      const size_t removed = (size_t)tree.lastEdit().removed;
      mirror.deleteBBX(lo, hi, true);
      std::printf("size %zu removed %zu mirror %zu\n", tree.size(), removed, mirror.size());
      at += 4 + 3 * n;
    }
    // a caller's own marks: by point and by key, bool and float, then forgotten
    const float p[3] = {100.05f, -100.05f, 20.05f};
    uint64_t key;
    if (!tree.coordToKeyChecked(p, &key)) return 5;
    tree.updateNode(p, true);
    tree.updateNode(key, true);
    tree.updateNode(key, -0.25f);
    tree.setNodeValue(p, 1.5f);
    const int marked = tree.search(p[0], p[1], p[2]);
    tree.updateNode(std::vector<uint64_t>(3, key), false);
    tree.edit({key, key}, {SBM_OCC_EDIT_DELETE, SBM_OCC_EDIT_UPDATE}, {0.f, 0.5f});
    const float far[3] = {5000.f, 0.f, 0.f};
    if (tree.deleteNode(far) || !tree.deleteNode(p, 15) || !tree.deleteNode(key)) return 5;
    std::printf("marked %d then %d\n", marked, tree.search(p[0], p[1], p[2]));
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  return 0;
}
