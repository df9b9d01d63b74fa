// Driver of tools/make_occupancy_option_fixtures.py: insertPointCloud with octomap's bounding box, change detection and
// discretize switched per scan; the leaves and the changed keys after every scan.
// This project's text; it calls octomap's API only.
//
// Per case: head, int32 scans. Per scan: int32 switches (bit 0 useBBXLimit, 1 enableChangeDetection, 2 discretize,
// 3 resetChangeDetection before the scan, 4 a box follows), [float min[3], float max[3]], then a scan record.
// Answer per case: the five constants; per scan the voxels, then uint32 m, uint16 keys[3 m], uint8 created[m].
#include "driver.h"

int main(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, in, out)) return 2;
  int32_t ncases;
  if (!rd(in, &ncases, 1)) return 3;
  for (int c = 0; c < ncases; c++) {
    double prob[5], resolution;
    int32_t nscans;
    if (!head_in(in, prob, &resolution) || !rd(in, &nscans, 1)) return 3;
    octomap::OcTree tree(resolution);
    set_params(tree, prob);
    constants_out(tree, out);
    for (int s = 0; s < nscans; s++) {
      int32_t sw;
      if (!rd(in, &sw, 1)) return 3;
      if (sw & 16) {
        float b[6];
        if (!rd(in, b, 6)) return 3;
        tree.setBBXMin(octomap::point3d(b[0], b[1], b[2]));
        tree.setBBXMax(octomap::point3d(b[3], b[4], b[5]));
      }
      tree.useBBXLimit((sw & 1) != 0);
      tree.enableChangeDetection((sw & 2) != 0);
      if (sw & 8) tree.resetChangeDetection();
      Scan scan;
      if (!scan_read(in, scan)) return 3;
      tree.insertPointCloud(scan.cloud, scan.origin, scan.max_range, false, (sw & 4) != 0);
      if (!voxels_out(tree, out)) return 4;
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
    }
  }
  fclose(out);
  return 0;
}
