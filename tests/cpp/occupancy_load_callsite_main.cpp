// A call site of octomap's readBinary through include/sbm_occupancy.hpp: a saved map is loaded, asked, extended and saved again,
//
//     octomap::OcTree tree(0.1);
//     tree.readBinary("slam.bt");
//     OcTreeNode* node = tree.search(x, y, z);
//     tree.insertPointCloud(scan, origin, maxrange);
//     tree.writeBinary("again.bt");
//
// with sbm::OccupancyMap in the tree's place. The points (float triples) and the scan (a float count, three floats of origin,
// then the triples; may be empty) are read from files. The output file receives per point an int32 state and the float value as
// loaded, then per stored voxel after the scan a uint64 key and the float log-odds. <again.bt> is written from the loaded map
// BEFORE the scan, through the maximum-likelihood tree. With "bytes" as the last argument the stream goes through the bytes
// form. Prints the voxels loaded and those after the scan. A failure prints "error <code>" and exits with 4.
//
//   occupancy_load_callsite_main <in.bt> <capacity> <points.raw> <points> <scan.raw> <floats> <max_range> <out.raw> <again.bt> [bytes]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sbm_occupancy.hpp"

template <class T> static bool read_all(const char* path, std::vector<T>& v, size_t count) {
  v.resize(count);
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  const size_t got = std::fread(v.data(), sizeof(T), count, f);
  std::fclose(f);
  return got == count;
}

int main(int argc, char** argv) {
  if (argc != 10 && argc != 11) return 2;
  std::vector<float> points, scan;
  const size_t npoints = (size_t)std::atoll(argv[4]);
  if (!read_all(argv[3], points, 3 * npoints) || !read_all(argv[5], scan, (size_t)std::atoll(argv[6]))) return 3;
  FILE* out = std::fopen(argv[8], "wb");
  if (!out) return 3;
  try {
    sbm::OccupancyMap map((size_t)std::atoll(argv[2]), 0.1);
    if (argc == 11 && !std::strcmp(argv[10], "bytes")) {
      std::vector<unsigned char> bt;
      FILE* f = std::fopen(argv[1], "rb");
      if (!f) return 3;
      for (int c; (c = std::fgetc(f)) != EOF;) bt.push_back((unsigned char)c);
      std::fclose(f);
      map.readBinary(bt.data(), bt.size());
    } else {
      map.readBinary(argv[1]);
    }
    const size_t loaded = map.size();
    for (size_t i = 0; i < npoints; i++) {
      float value = 0.f;
      const int32_t state = map.search(points[3 * i], points[3 * i + 1], points[3 * i + 2], &value);
      std::fwrite(&state, 4, 1, out);
      std::fwrite(&value, 4, 1, out);
    }
    map.buildTree()->writeBinary(argv[9]);
    if (scan.size() >= 4) {
      const size_t m = (size_t)scan[0];
      if (4 + 3 * m > scan.size()) return 3;
      map.insertPointCloud(scan.data() + 4, m, scan.data() + 1, std::atof(argv[7]));
    }
    std::vector<float> v;
    const std::vector<uint64_t> k = map.leaves(v);
    for (size_t i = 0; i < k.size(); i++) {
      std::fwrite(&k[i], 8, 1, out);
      std::fwrite(&v[i], 4, 1, out);
    }
    std::printf("loaded %zu after %zu overflow %llu\n", loaded, k.size(), (unsigned long long)map.overflow());
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  std::fclose(out);
  return 0;
}
