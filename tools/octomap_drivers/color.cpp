// Driver of tools/make_occupancy_color_fixtures.py: octomap::ColorOcTree -- setNodeColor and averageNodeColor by key or point in
// item order on an UNPRUNED tree (every insert and edit with lazy_eval = true), the colours of the tree after prune();
// updateInnerOccupancy();, AbstractOcTree::write / read of it, and a run resumed from its own stream.
// This project's text; it calls octomap's API only.
//
// Per case: head, int32 record (0: only times are answered), int32 steps. Per step int32 kind, then
//   kind 0  a scan record                                           -> insertPointCloud(cloud, origin, max_range, lazy_eval = true)
//   kind 1  int32 form, int32 op, int32 n, uint16 keys[3 n] (form 0) or float points[3 n] (form 1), uint8 rgb[3 n]
//           op 0 setNodeColor, 1 averageNodeColor; a point goes through coordToKeyChecked and is passed over if it has no key
//   kind 2  int32 n, uint16 keys[3 n], float values[n]              -> setNodeValue(key, value, lazy_eval = true)
//   kind 5  int32 n, uint16 keys[3 n], uint8 ops[n], float values[n]: op 0 updateNode(key, value, lazy_eval = true), 1 setNodeValue(key,
//           value, lazy_eval = true), 2 deleteNode(key), in item order
//   kind 3  a snapshot: nothing to read. A COPY of the tree (made by write / read) gets prune(); updateInnerOccupancy();
//   kind 4  a resume: nothing to read. The tree gets prune(); updateInnerOccupancy(); is written, read back and expand()ed, and
//           the case goes on with what was read
// Answer per case: the five constants; per step, with record,
//   kinds 0, 2, 4, 5  the coloured voxels: uint32 n, uint16 keys[3 n], float log-odds[n], uint8 rgb[3 n] (every leaf is at depth 16)
//   kind 1         uint32 found (items whose call returned a node), then the coloured voxels
//   kind 3         for maxDepth 16, 15, 12, 0: uint32 n and n coloured nodes of begin_leafs(maxDepth) (uint16 key[3], uint16 depth,
//                  float log-odds, uint8 rgb[3], uint8 0); the stream write() gives; int32 1 if read() gives a ColorOcTree back, and
//                  then the coloured voxels of that tree after expand()
// without record: double ms of each step of kind 1, and for kind 3 three doubles: prune + updateInnerOccupancy, write, read.
#include "driver.h"
#include <octomap/ColorOcTree.h>
#include <sstream>

typedef octomap::ColorOcTree Tree;

static void params(Tree& tree, const double* prob) {
  tree.setProbHit(prob[0]);
  tree.setProbMiss(prob[1]);
  tree.setClampingThresMin(prob[2]);
  tree.setClampingThresMax(prob[3]);
  tree.setOccupancyThres(prob[4]);
}

static bool voxels(const Tree& tree, FILE* out) {
  std::vector<uint16_t> keys;
  std::vector<float> values;
  std::vector<uint8_t> rgb;
  for (Tree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) {
    if (it.getDepth() != 16) return false;
    const octomap::OcTreeKey k = it.getKey();
    keys.push_back(k[0]);
    keys.push_back(k[1]);
    keys.push_back(k[2]);
    values.push_back(it->getLogOdds());
    const octomap::ColorOcTreeNode::Color c = it->getColor();
    rgb.push_back(c.r);
    rgb.push_back(c.g);
    rgb.push_back(c.b);
  }
  wr(out, (uint32_t)values.size());
  fwrite(keys.data(), 2, keys.size(), out);
  fwrite(values.data(), 4, values.size(), out);
  fwrite(rgb.data(), 1, rgb.size(), out);
  return true;
}

static void leaves(const Tree& tree, unsigned max_depth, FILE* out) {
  uint32_t n = 0;
  for (Tree::leaf_iterator it = tree.begin_leafs(max_depth), end = tree.end_leafs(); it != end; ++it) n++;
  wr(out, n);
  for (Tree::leaf_iterator it = tree.begin_leafs(max_depth), end = tree.end_leafs(); it != end; ++it) {
    node_out(out, it.getKey(), it.getDepth(), it->getLogOdds());
    const octomap::ColorOcTreeNode::Color c = it->getColor();
    const uint8_t b[4] = {c.r, c.g, c.b, 0};
    fwrite(b, 1, 4, out);
  }
}

static Tree* read_back(const std::string& s, const double* prob) {
  std::istringstream is(s);
  octomap::AbstractOcTree* any = octomap::AbstractOcTree::read(is);
  Tree* tree = dynamic_cast<Tree*>(any);
  if (!tree) {
    delete any;
    return 0;
  }
  params(*tree, prob);
  return tree;
}

int main(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, in, out)) return 2;
  int32_t ncases;
  if (!rd(in, &ncases, 1)) return 3;
  static const unsigned kDepths[4] = {16, 15, 12, 0};
  for (int c = 0; c < ncases; c++) {
    double prob[5], resolution;
    int32_t record, nsteps;
    if (!head_in(in, prob, &resolution) || !rd(in, &record, 1) || !rd(in, &nsteps, 1)) return 3;
    Tree* tree = new Tree(resolution);
    params(*tree, prob);
    float constants[5] = {tree->getProbHitLog(), tree->getProbMissLog(), tree->getClampingThresMinLog(), tree->getClampingThresMaxLog(),
                          tree->getOccupancyThresLog()};
    fwrite(constants, 4, 5, out);
    for (int s = 0; s < nsteps; s++) {
      int32_t kind;
      if (!rd(in, &kind, 1)) return 3;
      if (kind == 0) {
        Scan sc;
        if (!scan_read(in, sc)) return 3;
        tree->insertPointCloud(sc.cloud, sc.origin, sc.max_range, true);
      } else if (kind == 1) {
        int32_t form, op, n;
        if (!rd(in, &form, 1) || !rd(in, &op, 1) || !rd(in, &n, 1)) return 3;
        std::vector<uint16_t> k(form ? 0 : 3 * (size_t)n);
        std::vector<float> p(form ? 3 * (size_t)n : 0);
        std::vector<uint8_t> rgb(3 * (size_t)n);
        if (!rd(in, k.data(), k.size()) || !rd(in, p.data(), p.size()) || !rd(in, rgb.data(), rgb.size())) return 3;
        uint32_t found = 0;
        const Clock::time_point t0 = Clock::now();
        for (int i = 0; i < n; i++) {
          octomap::OcTreeKey key;
          if (form) {
            if (!tree->coordToKeyChecked(octomap::point3d(p[3 * i], p[3 * i + 1], p[3 * i + 2]), key)) continue;
          } else {
            key = octomap::OcTreeKey(k[3 * i], k[3 * i + 1], k[3 * i + 2]);
          }
          octomap::ColorOcTreeNode* node = op ? tree->averageNodeColor(key, rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2])
                                              : tree->setNodeColor(key, rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
          found += node ? 1 : 0;
        }
        const double ms = ms_since(t0);
        if (record) wr(out, found);
        else wr(out, ms);
      } else if (kind == 2) {
        int32_t n;
        if (!rd(in, &n, 1)) return 3;
        std::vector<uint16_t> k(3 * (size_t)n);
        std::vector<float> values(n);
        if (!rd(in, k.data(), k.size()) || !rd(in, values.data(), values.size())) return 3;
        for (int i = 0; i < n; i++) tree->setNodeValue(octomap::OcTreeKey(k[3 * i], k[3 * i + 1], k[3 * i + 2]), values[i], true);
      } else if (kind == 5) {
        int32_t n;
        if (!rd(in, &n, 1)) return 3;
        std::vector<uint16_t> k(3 * (size_t)n);
        std::vector<uint8_t> ops(n);
        std::vector<float> values(n);
        if (!rd(in, k.data(), k.size()) || !rd(in, ops.data(), ops.size()) || !rd(in, values.data(), values.size())) return 3;
        for (int i = 0; i < n; i++) {
          const octomap::OcTreeKey key(k[3 * i], k[3 * i + 1], k[3 * i + 2]);
          if (ops[i] == 0) tree->updateNode(key, values[i], true);
          else if (ops[i] == 1) tree->setNodeValue(key, values[i], true);
          else tree->deleteNode(key, 0);
        }
      } else if (kind == 3) {
        // the copy goes through write / read of the unpruned tree: octomap's copy constructor makes the children plain data nodes,
        // which have no colour
        std::ostringstream unpruned;
        tree->write(unpruned);
        Tree* made = read_back(unpruned.str(), prob);
        if (!made) return 5;
        Tree& copy = *made;
        Clock::time_point t0 = Clock::now();
        copy.prune();
        copy.updateInnerOccupancy();
        const double ms_prune = ms_since(t0);
        std::ostringstream os;
        t0 = Clock::now();
        copy.write(os);
        const double ms_write = ms_since(t0);
        t0 = Clock::now();
        Tree* back = read_back(os.str(), prob);
        const double ms_read = ms_since(t0);
        if (record) {
          for (int d = 0; d < 4; d++) leaves(copy, kDepths[d], out);
          stream_out(os.str(), out);
          wr(out, (int32_t)(back ? 1 : 0));
          if (back) {
            back->expand();
            if (!voxels(*back, out)) return 4;
          }
        } else {
          wr(out, ms_prune);
          wr(out, ms_write);
          wr(out, ms_read);
        }
        delete back;
        delete made;
        continue;
      } else if (kind == 4) {
        tree->prune();
        tree->updateInnerOccupancy();
        std::ostringstream os;
        tree->write(os);
        Tree* back = read_back(os.str(), prob);
        if (!back) return 5;
        back->expand();
        delete tree;
        tree = back;
      } else {
        return 3;
      }
      if (record && !voxels(*tree, out)) return 4;
    }
    delete tree;
  }
  fclose(out);
  return 0;
}
