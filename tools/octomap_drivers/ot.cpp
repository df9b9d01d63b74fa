// Driver of tools/make_occupancy_ot_fixtures.py: AbstractOcTree::write / read of octomap::OcTree.
// This project's text; it calls octomap's API only.
#include "driver.h"
#include <sstream>

// read() of a stream -> ok, size, calcNumNodes, leaves, search(points)
static octomap::OcTree* read_back(const std::string& s, const double* prob, const std::vector<float>& pts, FILE* out) {
  std::istringstream is(s);
  octomap::AbstractOcTree* any = octomap::AbstractOcTree::read(is);
  octomap::OcTree* tree = dynamic_cast<octomap::OcTree*>(any);
  wr(out, (int32_t)(tree ? 1 : any ? 2 : 0));
  if (!tree) return 0;
  set_params(*tree, prob);
  wr(out, (uint64_t)tree->size());
  wr(out, (uint64_t)tree->calcNumNodes());
  leaves_out(*tree, out);
  search_out(*tree, pts, out);
  return tree;
}

int main(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, in, out)) return 2;
  int32_t njobs;
  if (!rd(in, &njobs, 1)) return 3;
  for (int t = 0; t < njobs; t++) {
    double prob[5], resolution;
    int32_t kind;
    std::vector<float> pts;
    if (!head_in(in, prob, &resolution) || !rd(in, &kind, 1) || !points_in(in, pts)) return 3;
    if (kind == 0) {          // a scene: scans, a stream after each, its read-back; `resume` >= 0: read that stream and go on
      int32_t resume, nscans;
      if (!rd(in, &resume, 1) || !rd(in, &nscans, 1)) return 3;
      octomap::OcTree tree(resolution);
      set_params(tree, prob);
      octomap::OcTree* resumed = 0;
      for (int s = 0; s < nscans; s++) {
        const long at = ftell(in);
        if (!scan_in(in, tree)) return 3;
        if (resumed) {
          fseek(in, at, SEEK_SET);
          if (!scan_in(in, *resumed)) return 3;
        }
        std::ostringstream a, b;
        tree.write(a);
        octomap::OcTree copy(tree);
        copy.updateInnerOccupancy();
        copy.prune();
        copy.write(b);
        stream_out(a.str(), out);
        wr(out, (int32_t)(a.str() == b.str() ? 1 : 0));
        if (a.str() != b.str()) stream_out(b.str(), out);
        octomap::OcTree* back = read_back(a.str(), prob, pts, out);
        if (s == resume) resumed = back;
        else delete back;
      }
      if (resume >= 0) {
        if (!resumed) return 5;
        leaves_out(*resumed, out);
        tree.expand();
        resumed->expand();
        leaves_out(tree, out);
        leaves_out(*resumed, out);
        delete resumed;
      }
    } else {                  // a stream given: its read-back
      std::string s;
      if (!stream_in(in, s)) return 3;
      delete read_back(s, prob, pts, out);
      fflush(out);
    }
  }
  fclose(out);
  return 0;
}
