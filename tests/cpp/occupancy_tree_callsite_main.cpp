// A call site of octomap's tree above the voxels through include/sbm_occupancy.hpp: a tree filled with insertPointCloud, then
//
//     tree.updateInnerOccupancy();  tree.prune();
//     for (OcTree::leaf_iterator it = tree.begin_leafs(maxDepth), end = tree.end_leafs(); it != end; ++it) ...
//     OcTreeNode* node = tree.search(x, y, z, depth);
//     tree.writeBinary("slam.bt");                                   // main.cpp:560
//
// with sbm::OccupancyMap::buildTree() in the tree's place. The cloud (per scan: a float count, three floats of origin, then the
// triples) and the points (float triples) are read from files. The output file receives, for the log-odds tree, per leaf of
// begin_leafs(maxDepth) a uint64 centre key, an int32 depth and the float value, then per point an int32 state, the float value
// and the int32 depth of the node found; the .bt is written from the maximum-likelihood tree. Prints the voxels and, for both
// trees, size() and getNumLeafNodes(). A failure prints "error <code>" and exits with 4.
//
//   occupancy_tree_callsite_main <cloud.raw> <floats> <max_range> <capacity> <max_depth> <points.raw> <points> <depth> <out.raw> <out.bt>
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

int main(int argc, char** argv) {
  if (argc != 11) return 2;
  std::vector<float> cloud, points;
  const size_t npoints = (size_t)std::atoll(argv[7]);
  if (!read_all(argv[1], cloud, (size_t)std::atoll(argv[2])) || !read_all(argv[6], points, 3 * npoints)) return 3;
  FILE* out = std::fopen(argv[9], "wb");
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
    const std::vector<sbm::OccupancyLeaf> leaves = tree->leaves((unsigned)std::atoi(argv[5]));
    for (const sbm::OccupancyLeaf& l : leaves) {
      std::fwrite(&l.key, 8, 1, out);
      std::fwrite(&l.depth, 4, 1, out);
      std::fwrite(&l.value, 4, 1, out);
    }
    for (size_t i = 0; i < npoints; i++) {
      float value = 0.f;
      int depth = 0;
      const int32_t state = tree->search(points[3 * i], points[3 * i + 1], points[3 * i + 2], (unsigned)std::atoi(argv[8]), &value, &depth);
      const int32_t d = depth;
      std::fwrite(&state, 4, 1, out);
      std::fwrite(&value, 4, 1, out);
      std::fwrite(&d, 4, 1, out);
    }
    std::printf("voxels %zu size %zu leaves %zu listed %zu", map.size(), tree->size(), tree->getNumLeafNodes(), leaves.size());
    tree->rebuild(SBM_OCC_TREE_MAXLIKELIHOOD, map.rayParams());
    tree->writeBinary(argv[10]);
    std::printf(" bt_size %zu bt_leaves %zu\n", tree->size(), tree->getNumLeafNodes());
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  std::fclose(out);
  return 0;
}
