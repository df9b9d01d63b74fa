// Driver of tools/make_occupancy_fixtures.py: the calls of buildOccupancyGridMap's inner loop on recorded points.
// This project's text; it calls octomap's API only.
#include "driver.h"
#include <sstream>

int main(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, in, out)) return 2;
  double resolution;
  float range_max;
  int32_t n, groups;
  if (!rd(in, &resolution, 1) || !rd(in, &range_max, 1) || !rd(in, &n, 1) || !rd(in, &groups, 1)) return 3;
  std::vector<float> pts(6 * (size_t)n);
  std::vector<uint8_t> mask(n);
  if (!rd(in, pts.data(), pts.size()) || !rd(in, mask.data(), mask.size())) return 3;
  float rangeMaxSqrd = range_max * range_max;
  std::vector<octomap::OcTree*> trees;
  for (int g = 0; g < groups; g++) trees.push_back(new octomap::OcTree(resolution));
  for (int i = 0; i < n; i++) {
    const float* p = &pts[6 * (size_t)i];
    octomap::point3d pt(p[0], p[1], p[2]);
    octomap::point3d sensorOrigin(p[3], p[4], p[5]);
    octomap::point3d v(pt.x() - sensorOrigin.x(), pt.y() - sensorOrigin.y(), pt.z() - sensorOrigin.z());
    double norm = v.norm();
    octomap::OcTreeKey key(0, 0, 0);
    uint8_t ok = trees[0]->coordToKeyChecked(pt, key) ? 1 : 0;
    uint16_t k[3] = {0, 0, 0};
    if (ok) { k[0] = key[0]; k[1] = key[1]; k[2] = key[2]; }
    wr(out, norm);
    wr(out, ok);
    fwrite(k, 2, 3, out);
    if (norm <= rangeMaxSqrd && ok)
      for (int g = 0; g < groups; g++)
        if (mask[i] >> g & 1) trees[g]->updateNode(key, true);
  }
  for (int g = 0; g < groups; g++) {
    std::ostringstream s;
    trees[g]->writeBinary(s);
    wr(out, (uint32_t)trees[g]->getNumLeafNodes());
    wr(out, (uint32_t)trees[g]->size());
    stream_out(s.str(), out);
  }
  fclose(out);
  return 0;
}
