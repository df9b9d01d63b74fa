// Driver of tools/make_occupancy_load_fixtures.py: readBinary of recorded streams, then what octomap holds.
// This project's text; it calls octomap's API only.
#include "driver.h"
#include <sstream>

int main(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, in, out)) return 2;
  int32_t nstreams;
  if (!rd(in, &nstreams, 1)) return 3;
  for (int t = 0; t < nstreams; t++) {
    double prob[5], resolution;
    int32_t timing, file, post;
    if (!head_in(in, prob, &resolution) || !rd(in, &timing, 1)) return 3;
    octomap::OcTree tree(resolution);
    set_params(tree, prob);
    if (timing) {       // build the scene, write it, and time reading it back
      if (!scans_in(in, tree)) return 3;
      std::ostringstream s;
      tree.writeBinary(s);
      const std::string bt = s.str();
      double best = 1e300;
      uint64_t nodes = 0, voxels = 0;
      for (int rep = 0; rep < 5; rep++) {
        octomap::OcTree back(resolution);
        std::istringstream is(bt);
        Clock::time_point t0 = Clock::now();
        const bool ok = back.readBinary(is);
        const double ms = ms_since(t0);
        if (!ok) return 5;
        if (ms < best) best = ms;
        nodes = back.size();
      }
      tree.expand();
      for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) voxels++;
      wr(out, best);
      wr(out, nodes);
      wr(out, voxels);
      wr(out, (uint64_t)bt.size());
      continue;
    }
    bool ok;
    if (!rd(in, &file, 1)) return 3;
    if (!file) {        // no stream at all: a file that is not there
      ok = tree.readBinary(std::string(argv[2]) + ".does-not-exist");
    } else {
      std::string bt;
      if (!stream_in(in, bt)) return 3;
      std::istringstream is(bt);
      ok = tree.readBinary(is);
    }
    std::vector<float> pts;
    if (!points_in(in, pts) || !rd(in, &post, 1)) return 3;
    wr(out, (int32_t)(ok ? 1 : 0));
    wr(out, (uint64_t)tree.size());
    wr(out, (uint64_t)tree.calcNumNodes());
    if (ok) {
      leaves_out(tree, out);
      search_out(tree, pts, out);
    }
    if (post) {
      if (!scan_in(in, tree)) return 3;
      leaves_out(tree, out);
    }
  }
  fclose(out);
  return 0;
}
