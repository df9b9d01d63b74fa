// A call site of octomap's read side for planners through include/sbm_occupancy.hpp: a tree filled with insertPointCloud, then
//
//     for (OcTree::leaf_bbx_iterator it = tree.begin_leafs_bbx(min, max, maxDepth), end = tree.end_leafs_bbx(); it != end; ++it) ...
//     tree.getUnknownLeafCenters(centres, pmin, pmax, depth);
//     tree.getMetricMin(x, y, z);  tree.getMetricMax(x, y, z);  tree.getMetricSize(x, y, z);  tree.volume();
//     tree.getRayIntersection(origin, direction, center, intersection, delta);
//
// with sbm::OccupancyMap::buildTree() in the tree's place. The cloud (per scan: a float count, three floats of origin, then the
// triples) and the box (six floats: pmin, pmax) are read from files. The output file receives, for the log-odds tree, per leaf of
// the key box and then of the point box a uint64 centre key, an int32 depth and the float value; the unknown centres as float
// triples; nine doubles (min, max, size) and the volume; then for the ray (nine floats: origin, direction, centre) an int32 found
// and three floats. Prints the four counts. A failure prints "error <code>" and exits with 4.
//
//   occupancy_planner_callsite_main <cloud.raw> <floats> <max_range> <capacity> <max_depth> <box.raw> <depth> <ray.raw> <delta> <out.raw>
#include <cstdio>
#include <cstdlib>
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

static void write_leaves(const std::vector<sbm::OccupancyLeaf>& leaves, FILE* out) {
  for (const sbm::OccupancyLeaf& l : leaves) {
    std::fwrite(&l.key, 8, 1, out);
    std::fwrite(&l.depth, 4, 1, out);
    std::fwrite(&l.value, 4, 1, out);
  }
}

int main(int argc, char** argv) {
  if (argc != 11) return 2;
  std::vector<float> cloud, box, ray;
  if (!read_all(argv[1], cloud, (size_t)std::atoll(argv[2])) || !read_all(argv[6], box, 6) || !read_all(argv[8], ray, 9)) return 3;
  FILE* out = std::fopen(argv[10], "wb");
  if (!out) return 3;
  try {
    sbm::OccupancyMap map((size_t)std::atoll(argv[4]), 0.1);
    for (size_t at = 0; at + 4 <= cloud.size();) {
      const size_t m = (size_t)cloud[at];
      if (at + 4 + 3 * m > cloud.size()) return 3;
      map.insertPointCloud(cloud.data() + at + 4, m, cloud.data() + at + 1, std::atof(argv[3]));
      at += 4 + 3 * m;
    }
    auto tree = map.buildTree(SBM_OCC_TREE_LOGODDS);
    const unsigned max_depth = (unsigned)std::atoi(argv[5]);
    uint16_t kmin[3], kmax[3];
    for (int a = 0; a < 3; a++) {   // coordToKey of the corners, which have keys
      kmin[a] = (uint16_t)((int)std::floor(10.0 * (double)box[a]) + 32768);
      kmax[a] = (uint16_t)((int)std::floor(10.0 * (double)box[3 + a]) + 32768);
    }
    const std::vector<sbm::OccupancyLeaf> by_keys = tree->leafs_bbx(kmin, kmax, max_depth);
    const std::vector<sbm::OccupancyLeaf> by_points = tree->leafs_bbx(box.data(), box.data() + 3, max_depth);
    write_leaves(by_keys, out);
    write_leaves(by_points, out);
    std::vector<float> centres;
    tree->getUnknownLeafCenters(centres, box.data(), box.data() + 3, (unsigned)std::atoi(argv[7]));
    std::fwrite(centres.data(), 4, centres.size(), out);
    double m[10];
    tree->getMetricMin(m[0], m[1], m[2]);
    tree->getMetricMax(m[3], m[4], m[5]);
    tree->getMetricSize(m[6], m[7], m[8]);
    m[9] = tree->volume();
    std::fwrite(m, 8, 10, out);
    float hit[3] = {-1.f, -2.f, -3.f};
    const int32_t found = map.getRayIntersection(ray.data(), ray.data() + 3, ray.data() + 6, hit, std::atof(argv[9])) ? 1 : 0;
    std::fwrite(&found, 4, 1, out);
    std::fwrite(hit, 4, 3, out);
    float many[6];
    int32_t flags[2];
    const float two_dirs[6] = {ray[3], ray[4], ray[5], 0.f, 0.f, 0.f}, two_centres[6] = {ray[6], ray[7], ray[8], ray[6], ray[7], ray[8]};
    map.getRayIntersections(ray.data(), true, two_dirs, two_centres, 2, many, flags, std::atof(argv[9]));
    std::fwrite(flags, 4, 2, out);
    std::fwrite(many, 4, 6, out);
    std::printf("keys %zu points %zu unknown %zu found %d\n", by_keys.size(), by_points.size(), centres.size() / 3, (int)found);
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  std::fclose(out);
  return 0;
}
