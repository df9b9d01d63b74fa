// A mapper's key-frame step with octomap's three insert switches, through include/sbm_occupancy.hpp in octomap's spelling: a
// local map bounded by a box, one ray per end voxel, and a consumer that reads only what the scan changed. The cloud (per scan:
// a float count, three floats of origin, then the triples) is read from a file. Prints per scan "changes <n> created <m>" and
// at the end "size <voxels>"; a failure prints "error <code>" and exits with 4.
//
//   occupancy_options_callsite_main <cloud.raw> <floats> <capacity> <max_range> <discretize 0|1> [<min x y z> <max x y z>]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sbm_occupancy.hpp"

int main(int argc, char** argv) {
  if (argc != 6 && argc != 12) return 2;
  std::vector<float> cloud((size_t)std::atoll(argv[2]));
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(cloud.data(), sizeof(float), cloud.size(), f) != cloud.size()) return 3;
  std::fclose(f);
  try {
    sbm::OccupancyMap tree((size_t)std::atoll(argv[3]), 0.1);
    if (argc == 12) {
      const float lo[3] = {(float)std::atof(argv[6]), (float)std::atof(argv[7]), (float)std::atof(argv[8])};
      const float hi[3] = {(float)std::atof(argv[9]), (float)std::atof(argv[10]), (float)std::atof(argv[11])};
      tree.setBBXMin(lo);
      tree.setBBXMax(hi);
      tree.useBBXLimit(true);
      float back[3];
      tree.getBBXMax(back);
      const uint16_t centre[3] = {32768, 32768, 32768};
      if (!tree.bbxSet() || back[0] != hi[0] || tree.inBBX(hi) != (lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return 5;
      (void)tree.inBBX(centre);
    }
    tree.enableChangeDetection(true);
    if (!tree.isChangeDetectionEnabled()) return 5;
    for (size_t at = 0; at + 4 <= cloud.size();) {
      const size_t n = (size_t)cloud[at];
      tree.resetChangeDetection();
      tree.insertPointCloud(cloud.data() + at + 4, n, cloud.data() + at + 1, std::atof(argv[4]), false, std::atoi(argv[5]) != 0);
      size_t created = 0;
      const std::vector<std::pair<uint64_t, bool>> changed = tree.changedKeys();
      for (const std::pair<uint64_t, bool>& c : changed) created += c.second;
      if (changed.size() != tree.numChangesDetected()) return 5;
      std::printf("changes %zu created %zu\n", changed.size(), created);
      at += 4 + 3 * n;
    }
    std::printf("size %zu\n", tree.size());
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  return 0;
}
