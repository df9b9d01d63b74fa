// Driver of tools/make_occupancy_ray_fixtures.py: insertPointCloud on recorded scans, the leaves after every scan.
// This project's text; it calls octomap's API only.
#include "driver.h"
#include <sstream>

int main(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, in, out)) return 2;
  int32_t ncases;
  if (!rd(in, &ncases, 1)) return 3;
  for (int c = 0; c < ncases; c++) {
    double prob[5], resolution;
    int32_t timing, nscans;
    if (!head_in(in, prob, &resolution) || !rd(in, &timing, 1) || !rd(in, &nscans, 1)) return 3;
    octomap::OcTree tree(resolution);
    set_params(tree, prob);
    constants_out(tree, out);
    for (int s = 0; s < nscans; s++) {
      Scan scan;
      if (!scan_read(in, scan)) return 3;
      Clock::time_point t0 = Clock::now();
      tree.insertPointCloud(scan.cloud, scan.origin, scan.max_range);
      double ms = ms_since(t0);
      if (!voxels_out(tree, out, timing != 0)) return 4;
      if (timing) wr(out, ms);
    }
    std::ostringstream s;
    tree.writeBinary(s);
    wr(out, (uint32_t)tree.size());
    stream_out(timing ? std::string() : s.str(), out);
  }
  fclose(out);
  return 0;
}
