// A call site of octomap's .ot file through include/sbm_occupancy.hpp: a map is built from scans, saved with its probabilities,
// read back into a second tree and extended,
//
//     octomap::OcTree tree(0.1);
//     tree.insertPointCloud(scan, origin, maxrange);  ...
//     tree.write("map.ot");
//     octomap::OcTree* again = dynamic_cast<octomap::OcTree*>(octomap::AbstractOcTree::read("map.ot"));
//     again->insertPointCloud(next_scan, origin, maxrange);  ...
//
// with sbm::OccupancyMap in the trees' places. The scans are read from one file: per scan a float count, three floats of origin,
// then the triples. The first <k> scans go into the first map, which writes <map.ot>; the second map reads it and takes the
// remaining scans. The output file receives per stored voxel of the second map a uint64 key and the float log-odds. Prints the
// voxels written and those at the end. A failure prints "error <code>" and exits with 4.
//
//   occupancy_ot_callsite_main <scans.raw> <floats> <k> <capacity> <max_range> <map.ot> <out.raw>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sbm_occupancy.hpp"

int main(int argc, char** argv) {
  if (argc != 8) return 2;
  std::vector<float> scans((size_t)std::atoll(argv[2]));
  FILE* in = std::fopen(argv[1], "rb");
  if (!in || std::fread(scans.data(), 4, scans.size(), in) != scans.size()) return 3;
  std::fclose(in);
  FILE* out = std::fopen(argv[7], "wb");
  if (!out) return 3;
  const int k = std::atoi(argv[3]);
  const size_t capacity = (size_t)std::atoll(argv[4]);
  const double max_range = std::atof(argv[5]);
  try {
    sbm::OccupancyMap first(capacity, 0.1), second(capacity, 0.1);
    size_t at = 0, written = 0;
    for (int s = 0; at + 4 <= scans.size(); s++) {
      const size_t m = (size_t)scans[at];
      if (at + 4 + 3 * m > scans.size()) return 3;
      if (s == k) {
        written = first.size();
        first.write(argv[6]);
        second.read(argv[6]);
      }
      (s < k ? first : second).insertPointCloud(scans.data() + at + 4, m, scans.data() + at + 1, max_range);
      at += 4 + 3 * m;
    }
    std::vector<float> v;
    const std::vector<uint64_t> keys = second.leaves(v);
    for (size_t i = 0; i < keys.size(); i++) {
      std::fwrite(&keys[i], 8, 1, out);
      std::fwrite(&v[i], 4, 1, out);
    }
    std::printf("written %zu after %zu overflow %llu\n", written, keys.size(), (unsigned long long)second.overflow());
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  std::fclose(out);
  return 0;
}
