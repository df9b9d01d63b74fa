// Driver of tools/make_occupancy_tree_fixtures.py: trees from recorded scans or key lists, then what octomap holds above them.
// This project's text; it calls octomap's API only.
#include "driver.h"
#include <map>
#include <sstream>

static void record(octomap::OcTree& tree, const std::vector<float>& pts, FILE* out) {
  std::map<const octomap::OcTreeNode*, int> depth_of;
  std::vector<uint8_t> leaf;
  uint32_t n = 0;
  for (octomap::OcTree::tree_iterator it = tree.begin_tree(), end = tree.end_tree(); it != end; ++it) n++;
  wr(out, n);
  for (octomap::OcTree::tree_iterator it = tree.begin_tree(), end = tree.end_tree(); it != end; ++it) {
    node_out(out, it.getKey(), it.getDepth(), it->getLogOdds());
    leaf.push_back(it.isLeaf() ? 1 : 0);
    depth_of[&(*it)] = (int)it.getDepth();
  }
  fwrite(leaf.data(), 1, leaf.size(), out);
  const int max_depths[6] = {0, 15, 14, 12, 8, 1};
  for (int md : max_depths) {
    n = 0;
    for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(md), end = tree.end_leafs(); it != end; ++it) n++;
    wr(out, n);
    for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(md), end = tree.end_leafs(); it != end; ++it)
      node_out(out, it.getKey(), it.getDepth(), it->getLogOdds());
  }
  wr(out, (uint64_t)tree.calcNumNodes());
  wr(out, (uint64_t)tree.getNumLeafNodes());
  const int depths[7] = {0, 16, 15, 14, 12, 8, 1};
  for (int d : depths)
    for (size_t i = 0; i < pts.size(); i += 3) {
      octomap::OcTreeNode* node = tree.search(octomap::point3d(pts[i], pts[i + 1], pts[i + 2]), d);
      wr(out, (int32_t)(node ? 1 : 0));
      wr(out, (float)(node ? node->getLogOdds() : 0.f));
      wr(out, (int32_t)(node ? depth_of.at(node) : -1));
    }
}

int main(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, in, out)) return 2;
  int32_t ntrees;
  if (!rd(in, &ntrees, 1)) return 3;
  for (int t = 0; t < ntrees; t++) {
    double prob[5], resolution;
    int32_t hits, timing;
    std::vector<float> pts;
    if (!head_in(in, prob, &resolution) || !rd(in, &hits, 1) || !rd(in, &timing, 1)) return 3;
    octomap::OcTree tree(resolution);
    set_params(tree, prob);
    constants_out(tree, out);
    if (!(hits ? hits_in(in, tree) : scans_in(in, tree)) || !points_in(in, pts)) return 3;
    if (timing) {     // octomap's own time for what the device tree replaces
      tree.expand();  // from the voxels, as the device starts
      Clock::time_point t0 = Clock::now();
      tree.updateInnerOccupancy();
      tree.prune();
      std::ostringstream s;
      tree.writeBinary(s);
      double write_ms = ms_since(t0);
      t0 = Clock::now();
      uint64_t leaves = 0;
      for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) leaves++;
      double iterate_ms = ms_since(t0);
      uint64_t voxels = 0;
      tree.expand();
      for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) voxels++;
      wr(out, write_ms);
      wr(out, iterate_ms);
      wr(out, leaves);
      wr(out, voxels);
      wr(out, (uint64_t)s.str().size());
      continue;
    }
    {                 // the voxels: the leaves of an expanded copy
      octomap::OcTree copy(tree);
      copy.expand();
      if (!leaves_out(copy, out, 16)) return 4;
    }
    if (!hits) {
      tree.updateInnerOccupancy();
      tree.prune();
      record(tree, pts, out);
    }
    tree.toMaxLikelihood();
    tree.prune();
    record(tree, pts, out);
    std::ostringstream s;
    tree.writeBinaryConst(s);
    stream_out(s.str(), out);
  }
  fclose(out);
  return 0;
}
