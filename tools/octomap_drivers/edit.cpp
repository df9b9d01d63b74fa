// Driver of tools/make_occupancy_edit_fixtures.py: updateNode(key | point, float | bool), setNodeValue and deleteNode in item
// order, between scans and under change detection; the leaves, the changed keys and a few searches after every step.
// This project's text; it calls octomap's API only.
//
// Per case: head, int32 record (0: only the edit and delete steps are timed), int32 p, uint16 probes[3 p], int32 steps. Per step:
// int32 kind, int32 switches (bit 0 enableChangeDetection, bit 1 resetChangeDetection before the step), then
//   kind 0  a scan record                                                                   -> insertPointCloud
//   kind 1  int32 form, int32 n, uint16 keys[3 n] (form 0) or float points[3 n] (form 1), uint8 ops[n], float values[n]
//           op 0 updateNode(., float), 1 setNodeValue, 2 deleteNode(., 0), 3 updateNode(., true), 4 updateNode(., false)
//   kind 2  int32 depth, int32 n, uint16 keys[3 n]                                           -> deleteNode(key, depth)
//   kind 3  uint16 min[3], uint16 max[3], int32 outside      -> the loop users write: the depth-16 keys of the expanded tree that
//           pass (or, outside, fail) the inclusive key test are collected, then deleteNode of each
// Answer per case: the five constants; per step, with record: uint32 root_only (a root without children), float the root's value,
// the voxels (none for such a root: expanding it would fill the whole space), uint32 m, uint16 keys[3 m], uint8 created[m], and
// per probe int32 found, float value of search(key); without record: double ms of each step of kind 1, 2 or 3.
#include "driver.h"

static bool root_only(const octomap::OcTree& tree) { return tree.getRoot() && !tree.nodeHasChildren(tree.getRoot()); }

static bool key_in_box(const octomap::OcTreeKey& k, const uint16_t* lo, const uint16_t* hi) {
  return k[0] >= lo[0] && k[0] <= hi[0] && k[1] >= lo[1] && k[1] <= hi[1] && k[2] >= lo[2] && k[2] <= hi[2];
}

int main(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, in, out)) return 2;
  int32_t ncases;
  if (!rd(in, &ncases, 1)) return 3;
  for (int c = 0; c < ncases; c++) {
    double prob[5], resolution;
    int32_t record, nprobes, nsteps;
    if (!head_in(in, prob, &resolution) || !rd(in, &record, 1) || !rd(in, &nprobes, 1)) return 3;
    std::vector<uint16_t> probes(3 * (size_t)nprobes);
    if (!rd(in, probes.data(), probes.size()) || !rd(in, &nsteps, 1)) return 3;
    octomap::OcTree tree(resolution);
    set_params(tree, prob);
    constants_out(tree, out);
    for (int s = 0; s < nsteps; s++) {
      int32_t kind, sw;
      if (!rd(in, &kind, 1) || !rd(in, &sw, 1)) return 3;
      tree.enableChangeDetection((sw & 1) != 0);
      if (sw & 2) tree.resetChangeDetection();
      double ms = 0.;
      if (kind == 0) {
        if (!scan_in(in, tree)) return 3;
      } else if (kind == 1) {
        int32_t form, n;
        if (!rd(in, &form, 1) || !rd(in, &n, 1)) return 3;
        std::vector<uint16_t> k(form ? 0 : 3 * (size_t)n);
        std::vector<float> p(form ? 3 * (size_t)n : 0), values(n);
        std::vector<uint8_t> ops(n);
        if (!rd(in, k.data(), k.size()) || !rd(in, p.data(), p.size()) || !rd(in, ops.data(), ops.size()) || !rd(in, values.data(), values.size()))
          return 3;
        const Clock::time_point t0 = Clock::now();
        for (int i = 0; i < n; i++) {
          if (form) {
            const octomap::point3d q(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
            if (ops[i] == 0) tree.updateNode(q, values[i]);
            else if (ops[i] == 1) tree.setNodeValue(q, values[i]);
            else if (ops[i] == 2) tree.deleteNode(q, 0);
            else tree.updateNode(q, ops[i] == 3);
          } else {
            const octomap::OcTreeKey q(k[3 * i], k[3 * i + 1], k[3 * i + 2]);
            if (ops[i] == 0) tree.updateNode(q, values[i]);
            else if (ops[i] == 1) tree.setNodeValue(q, values[i]);
            else if (ops[i] == 2) tree.deleteNode(q, 0);
            else tree.updateNode(q, ops[i] == 3);
          }
        }
        ms = ms_since(t0);
      } else if (kind == 2) {
        int32_t depth, n;
        if (!rd(in, &depth, 1) || !rd(in, &n, 1)) return 3;
        std::vector<uint16_t> k(3 * (size_t)n);
        if (!rd(in, k.data(), k.size())) return 3;
        const Clock::time_point t0 = Clock::now();
        for (int i = 0; i < n; i++) tree.deleteNode(octomap::OcTreeKey(k[3 * i], k[3 * i + 1], k[3 * i + 2]), (unsigned)depth);
        ms = ms_since(t0);
      } else {
        uint16_t box[6];
        int32_t outside;
        if (!rd(in, box, 6) || !rd(in, &outside, 1)) return 3;
        const Clock::time_point t0 = Clock::now();
        if (tree.getRoot() && !root_only(tree)) {
          tree.expand();
          std::vector<octomap::OcTreeKey> gone;
          for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it)
            if (key_in_box(it.getKey(), box, box + 3) != (outside != 0)) gone.push_back(it.getKey());
          for (size_t i = 0; i < gone.size(); i++) tree.deleteNode(gone[i], 0);
        }
        ms = ms_since(t0);
      }
      if (!record) {
        if (kind != 0) wr(out, ms);
        continue;
      }
      const bool bare = root_only(tree);
      wr(out, (uint32_t)(bare ? 1 : 0));
      wr(out, (float)(tree.getRoot() ? tree.getRoot()->getLogOdds() : 0.f));
      if (bare) wr(out, (uint32_t)0);
      else if (!voxels_out(tree, out)) return 4;
      std::vector<uint16_t> keys;
      std::vector<uint8_t> created;
      for (octomap::KeyBoolMap::const_iterator it = tree.changedKeysBegin(); it != tree.changedKeysEnd(); ++it) {
        keys.push_back(it->first[0]);
        keys.push_back(it->first[1]);
        keys.push_back(it->first[2]);
        created.push_back(it->second ? 1 : 0);
      }
      wr(out, (uint32_t)created.size());
      fwrite(keys.data(), 2, keys.size(), out);
      fwrite(created.data(), 1, created.size(), out);
      for (int i = 0; i < nprobes; i++) {
        octomap::OcTreeNode* node = tree.search(octomap::OcTreeKey(probes[3 * i], probes[3 * i + 1], probes[3 * i + 2]));
        wr(out, (int32_t)(node ? 1 : 0));
        wr(out, (float)(node ? node->getLogOdds() : 0.f));
      }
    }
  }
  fclose(out);
  return 0;
}
