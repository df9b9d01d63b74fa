// Driver of tools/make_occupancy_query_fixtures.py: trees from recorded scans or key lists, then search and castRay.
// This project's text; it calls octomap's API only.
#include "driver.h"
#include <cmath>

int main(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, in, out)) return 2;
  int32_t ntrees;
  if (!rd(in, &ntrees, 1)) return 3;
  for (int t = 0; t < ntrees; t++) {
    double prob[5], resolution;
    int32_t hits, nsets;
    if (!head_in(in, prob, &resolution) || !rd(in, &hits, 1)) return 3;
    octomap::OcTree tree(resolution);
    set_params(tree, prob);
    constants_out(tree, out);
    if (!(hits ? hits_in(in, tree) : scans_in(in, tree))) return 3;
    if (!voxels_out(tree, out)) return 4;
    if (!rd(in, &nsets, 1)) return 3;
    for (int q = 0; q < nsets; q++) {
      int32_t timing, nrays;
      std::vector<float> pts;
      if (!rd(in, &timing, 1) || !points_in(in, pts) || !rd(in, &nrays, 1)) return 3;
      for (size_t i = 0; i < pts.size(); i += 3) {
        octomap::OcTreeNode* node = tree.search(octomap::point3d(pts[i], pts[i + 1], pts[i + 2]));
        wr(out, (int32_t)(node ? 1 : 0));
        wr(out, (int32_t)(node && tree.isNodeOccupied(node) ? 1 : 0));
        wr(out, (float)(node ? node->getLogOdds() : 0.f));
      }
      std::vector<float> rays(6 * (size_t)nrays);
      std::vector<int32_t> ignore(nrays);
      std::vector<double> range(nrays);
      for (int i = 0; i < nrays; i++)
        if (!rd(in, &rays[6 * i], 6) || !rd(in, &ignore[i], 1) || !rd(in, &range[i], 1)) return 3;
      std::vector<int32_t> ret(nrays);
      std::vector<float> ends(3 * (size_t)nrays);
      Clock::time_point t0 = Clock::now();
      for (int i = 0; i < nrays; i++) {
        const float* r = &rays[6 * i];
        octomap::point3d end(NAN, NAN, NAN);
        ret[i] = tree.castRay(octomap::point3d(r[0], r[1], r[2]), octomap::point3d(r[3], r[4], r[5]), end, ignore[i] != 0, range[i]) ? 1 : 0;
        ends[3 * i] = end.x();
        ends[3 * i + 1] = end.y();
        ends[3 * i + 2] = end.z();
      }
      double ms = ms_since(t0);
      if (timing) {
        wr(out, ms);
      } else {
        fwrite(ret.data(), 4, ret.size(), out);
        fwrite(ends.data(), 4, ends.size(), out);
      }
    }
  }
  fclose(out);
  return 0;
}
