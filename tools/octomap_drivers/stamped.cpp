// Driver of tools/make_occupancy_stamped_fixtures.py: octomap::OcTreeStamped -- the stamps insertPointCloud, updateNode,
// setNodeValue and deleteNode leave on an UNPRUNED tree (every insert and edit with lazy_eval = true), degradeOutdatedNodes, and
// forgetting by age as a leaf loop plus deleteNode. octomap takes its clock from time(NULL); this program defines time() itself,
// which overrides the C library's for the whole program, and returns what the generator scripts per step.
// This project's text; it calls octomap's API only.
//
// Per case: head, int32 record (0: only times are answered), int32 steps. Per step int32 kind, uint32 clock (what time() answers
// from here on), then
//   kind 0  int32 flags (1 discretize, 2 useBBXLimit, 4 enableChangeDetection), float bbx min[3], max[3] if flag 2, a scan record
//                                                       -> insertPointCloud(cloud, origin, max_range, lazy_eval = true, discretize)
//   kind 1  int32 n, uint16 keys[3 n], uint8 ops[n], float values[n], in item order: op 0 updateNode(key, value, lazy_eval = true),
//           1 setNodeValue(key, value, lazy_eval = true), 2 deleteNode(key), 3 updateNode(key, true, lazy_eval = true),
//           4 updateNode(key, false, lazy_eval = true)
//   kind 2  uint32 time_thres                           -> degradeOutdatedNodes(time_thres)
//   kind 3  uint32 time_thres                           -> the leaves with (uint32)(clock - stamp) > time_thres collected, then
//                                                          deleteNode(key) of each
//   kind 4  a snapshot: nothing to read. LOGODDS reading: the tree gets updateInnerOccupancy(); prune(); is recorded and written
//           (AbstractOcTree::write), then expand()ed again, which gives every voxel back its value and stamp (copyData).
//           MAXLIKELIHOOD reading: a second tree is made of the voxels (per voxel updateNode(key, 0.f) at the voxel's stamp, then
//           setNodeValue(key, value)), and at the step's clock gets toMaxLikelihood(); prune(); updateInnerOccupancy();
//   kind 5  a resume: nothing to read. updateInnerOccupancy(); prune(); write, read back (stamps 0) and expand(); the case goes on
//           with what was read
// Answer per case: the five constants; per step, with record,
//   kind 2  uint32 how many leaves met degradeOutdatedNodes' condition before the call
//   kind 3  uint32 how many leaves were deleted
//   kind 4  per reading: uint32 n, n nodes of begin_tree() (uint16 key[3], uint16 depth, float log-odds, uint32 stamp), uint8 leaf[n],
//           uint32 getLastUpdateTime(), and a stream: write() for LOGODDS, writeBinaryConst() for MAXLIKELIHOOD
//   every kind  the stamped voxels: uint32 n, uint16 keys[3 n], float log-odds[n], uint32 stamps[n] (every leaf is at depth 16)
// without record: double ms of each step (kind 4: of updateInnerOccupancy(); prune(); alone).
#include "driver.h"
#include <octomap/OcTreeStamped.h>
#include <ctime>
#include <sstream>

typedef octomap::OcTreeStamped Tree;

static unsigned int g_clock = 0;
extern "C" time_t time(time_t* t) {
  if (t) *t = (time_t)g_clock;
  return (time_t)g_clock;
}

static void params(Tree& tree, const double* prob) {
  tree.setProbHit(prob[0]);
  tree.setProbMiss(prob[1]);
  tree.setClampingThresMin(prob[2]);
  tree.setClampingThresMax(prob[3]);
  tree.setOccupancyThres(prob[4]);
}

static bool voxels(Tree& tree, FILE* out) {
  std::vector<uint16_t> keys;
  std::vector<float> values;
  std::vector<uint32_t> stamps;
  for (Tree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) {
    if (it.getDepth() != 16) return false;
    const octomap::OcTreeKey k = it.getKey();
    keys.push_back(k[0]);
    keys.push_back(k[1]);
    keys.push_back(k[2]);
    values.push_back(it->getLogOdds());
    stamps.push_back((uint32_t)it->getTimestamp());
  }
  wr(out, (uint32_t)values.size());
  fwrite(keys.data(), 2, keys.size(), out);
  fwrite(values.data(), 4, values.size(), out);
  fwrite(stamps.data(), 4, stamps.size(), out);
  return true;
}

static void nodes(Tree& tree, FILE* out) {
  uint32_t n = 0;
  for (Tree::tree_iterator it = tree.begin_tree(), end = tree.end_tree(); it != end; ++it) n++;
  wr(out, n);
  std::vector<uint8_t> leaf;
  for (Tree::tree_iterator it = tree.begin_tree(), end = tree.end_tree(); it != end; ++it) {
    node_out(out, it.getKey(), it.getDepth(), it->getLogOdds());
    wr(out, (uint32_t)it->getTimestamp());
    leaf.push_back(it.isLeaf() ? 1 : 0);
  }
  fwrite(leaf.data(), 1, leaf.size(), out);
  wr(out, (uint32_t)tree.getLastUpdateTime());
}

int main(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, in, out)) return 2;
  int32_t ncases;
  if (!rd(in, &ncases, 1)) return 3;
  for (int c = 0; c < ncases; c++) {
    double prob[5], resolution;
    int32_t record, nsteps;
    if (!head_in(in, prob, &resolution) || !rd(in, &record, 1) || !rd(in, &nsteps, 1)) return 3;
    g_clock = 0;
    Tree* held = new Tree(resolution);
    params(*held, prob);
    float constants[5] = {held->getProbHitLog(), held->getProbMissLog(), held->getClampingThresMinLog(), held->getClampingThresMaxLog(),
                          held->getOccupancyThresLog()};
    fwrite(constants, 4, 5, out);
    for (int s = 0; s < nsteps; s++) {
      int32_t kind;
      uint32_t clock;
      if (!rd(in, &kind, 1) || !rd(in, &clock, 1)) return 3;
      g_clock = clock;
      Tree& tree = *held;
      uint32_t answer = 0;
      double ms = 0.;
      if (kind == 0) {
        int32_t flags;
        if (!rd(in, &flags, 1)) return 3;
        if (flags & 2) {
          float b[6];
          if (!rd(in, b, 6)) return 3;
          tree.setBBXMin(octomap::point3d(b[0], b[1], b[2]));
          tree.setBBXMax(octomap::point3d(b[3], b[4], b[5]));
        }
        tree.useBBXLimit((flags & 2) != 0);
        tree.enableChangeDetection((flags & 4) != 0);
        Scan sc;
        if (!scan_read(in, sc)) return 3;
        const Clock::time_point t0 = Clock::now();
        tree.insertPointCloud(sc.cloud, sc.origin, sc.max_range, true, (flags & 1) != 0);
        ms = ms_since(t0);
      } else if (kind == 1) {
        int32_t n;
        if (!rd(in, &n, 1)) return 3;
        std::vector<uint16_t> k(3 * (size_t)n);
        std::vector<uint8_t> ops(n);
        std::vector<float> values(n);
        if (!rd(in, k.data(), k.size()) || !rd(in, ops.data(), ops.size()) || !rd(in, values.data(), values.size())) return 3;
        const Clock::time_point t0 = Clock::now();
        for (int i = 0; i < n; i++) {
          const octomap::OcTreeKey key(k[3 * i], k[3 * i + 1], k[3 * i + 2]);
          if (ops[i] == 0) tree.updateNode(key, values[i], true);
          else if (ops[i] == 1) tree.setNodeValue(key, values[i], true);
          else if (ops[i] == 2) tree.deleteNode(key, 0);
          else tree.updateNode(key, ops[i] == 3, true);
        }
        ms = ms_since(t0);
      } else if (kind == 2) {
        uint32_t thres;
        if (!rd(in, &thres, 1)) return 3;
        for (Tree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it)
          if (tree.isNodeOccupied(*it) && (g_clock - it->getTimestamp()) > thres) answer++;
        const Clock::time_point t0 = Clock::now();
        tree.degradeOutdatedNodes(thres);
        ms = ms_since(t0);
      } else if (kind == 3) {
        uint32_t thres;
        if (!rd(in, &thres, 1)) return 3;
        const Clock::time_point t0 = Clock::now();
        std::vector<octomap::OcTreeKey> old;
        for (Tree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it)
          if ((g_clock - it->getTimestamp()) > thres) old.push_back(it.getKey());
        for (size_t i = 0; i < old.size(); i++) tree.deleteNode(old[i], 0);   // its bool says whether the root went, not the leaf
        answer = (uint32_t)old.size();
        ms = ms_since(t0);
      } else if (kind == 4) {
        const Clock::time_point t0 = Clock::now();
        tree.updateInnerOccupancy();
        tree.prune();
        ms = ms_since(t0);
        if (record) {
          nodes(tree, out);
          std::ostringstream os;
          tree.write(os);
          stream_out(os.str(), out);
        }
        tree.expand();
        if (record) {
          Tree ml(resolution);
          params(ml, prob);
          for (Tree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) {
            g_clock = it->getTimestamp();
            ml.updateNode(it.getKey(), 0.f, true);
            ml.setNodeValue(it.getKey(), it->getLogOdds(), true);
          }
          g_clock = clock;
          ml.toMaxLikelihood();
          ml.prune();
          ml.updateInnerOccupancy();
          nodes(ml, out);
          std::ostringstream os;
          ml.writeBinaryConst(os);
          stream_out(os.str(), out);
        }
      } else if (kind == 5) {
        tree.updateInnerOccupancy();
        tree.prune();
        std::ostringstream os;
        tree.write(os);
        std::istringstream is(os.str());
        octomap::AbstractOcTree* any = octomap::AbstractOcTree::read(is);
        Tree* back = dynamic_cast<Tree*>(any);
        if (!back) return 5;
        params(*back, prob);
        back->expand();
        delete held;
        held = back;
      } else {
        return 3;
      }
      if (!record) {
        wr(out, ms);
        continue;
      }
      if (kind == 2 || kind == 3) wr(out, answer);
      if (!voxels(*held, out)) return 4;
    }
    delete held;
  }
  fclose(out);
  return 0;
}
