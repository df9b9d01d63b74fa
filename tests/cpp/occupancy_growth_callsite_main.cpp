// A mapper that cannot know its voxel count, through include/sbm_occupancy.hpp: a map created for ONE voxel with setGrowth(true)
// takes the scans a pre-sized map takes, and after every scan both hold the same voxels with the same log-odds bits. Half way
// the pre-sized map is moved into a larger table by hand (reserve), which must change nothing. The cloud (per scan: a float
// count, three floats of origin, then the triples) is read from a file. Prints per scan "scan <i> size <voxels>" and at the end
// "capacity <grown map's> grown <tables> reserved <pre-sized map's capacity>"; a difference prints "differ <scan>" and exits
// with 5, a failure prints "error <code>" and exits with 4.
//
//   occupancy_growth_callsite_main <cloud.raw> <floats> <capacity of the pre-sized map> <max_range>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sbm_occupancy.hpp"

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  std::vector<float> cloud((size_t)std::atoll(argv[2]));
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(cloud.data(), sizeof(float), cloud.size(), f) != cloud.size()) return 3;
  std::fclose(f);
  try {
    const size_t sized = (size_t)std::atoll(argv[3]);
    sbm::OccupancyMap grown(1, 0.1), ample(sized, 0.1);
    if (grown.capacity() != 1 || grown.growth().enabled != 0 || ample.capacity() != sized) return 5;
    grown.setGrowth(true);
    if (grown.growth().enabled != 1 || grown.growth().max_capacity != ((uint64_t)1 << 30)) return 5;
    size_t scan = 0;
    for (size_t at = 0; at + 4 <= cloud.size(); scan++) {
      const size_t n = (size_t)cloud[at];
      grown.insertPointCloud(cloud.data() + at + 4, n, cloud.data() + at + 1, std::atof(argv[4]));
      ample.insertPointCloud(cloud.data() + at + 4, n, cloud.data() + at + 1, std::atof(argv[4]));
      if (scan == 0) {
        ample.reserve(4 * sized);
        ample.reserve(sized);   // never shrinks
      }
      std::vector<float> va, vb;
      const std::vector<uint64_t> ka = grown.leaves(va), kb = ample.leaves(vb);
      if (ka != kb || va.size() != vb.size() || (va.size() && std::memcmp(va.data(), vb.data(), va.size() * sizeof(float)) != 0)) {
        std::printf("differ %zu\n", scan);
        return 5;
      }
      std::printf("scan %zu size %zu\n", scan, ka.size());
      at += 4 + 3 * n;
    }
    if (grown.overflow() != 0 || ample.overflow() != 0) return 5;
    std::printf("capacity %zu grown %llu reserved %zu\n", grown.capacity(), (unsigned long long)grown.growth().grown, ample.capacity());
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  return 0;
}
