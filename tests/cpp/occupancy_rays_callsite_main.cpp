// The reference's buildOccupancyGridMap (src/slam/src/core/main.cpp:495-561) with octomap's insertPointCloud in place of
// updateNode, through include/sbm_occupancy.hpp: the loop over nodes, each with its decimated disparity map and its pose, whose
// translation is the sensorOrigin of main.cpp:520, then writeBinary. With a cloud file the same scans go in as point clouds
// (insertPointCloud's own signature) instead. The planes (int16, dense), the poses (12 floats each), the camera model
// (sbm_stereo_model, raw) and the cloud (per scan: a float count, three floats of origin, then the triples) are read from
// files. Prints "size <voxels> overflow <cells>"; a failure prints "error <code>" and exits with 4.
//
//   occupancy_rays_callsite_main <planes.raw> <n> <width> <height> <scale> <poses.raw> <model.raw> <capacity> <max_range> <out.bt>
//                                [<cloud.raw> <floats>]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sbm_occupancy.hpp"

template <class T> static bool read_all(const char* path, std::vector<T>& v, size_t count) {
  v.resize(count);
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  const size_t got = std::fread(v.data(), sizeof(T), count, f);
  std::fclose(f);
  return got == count;
}

int main(int argc, char** argv) {
  if (argc != 11 && argc != 13) return 2;
  const int n = std::atoi(argv[2]), W = std::atoi(argv[3]), H = std::atoi(argv[4]), scale = std::atoi(argv[5]);
  if (n <= 0 || W <= 0 || H <= 0 || scale <= 0) return 2;
  std::vector<int16_t> planes;
  std::vector<float> poses, cloud;
  std::vector<sbm_stereo_model> model;
  if (!read_all(argv[1], planes, (size_t)n * W * H) || !read_all(argv[6], poses, (size_t)n * 12) || !read_all(argv[7], model, 1))
    return 3;
  if (argc == 13 && !read_all(argv[11], cloud, (size_t)std::atoll(argv[12]))) return 3;
  try {
    // --- main.cpp:499-501 ---------------------------------------------------------------------------------------------------
    sbm::OccupancyMap tree((size_t)std::atoll(argv[8]), 0.1);
    tree.rayParams().max_range = std::atof(argv[9]);
    if (argc == 13) {
      for (size_t at = 0; at + 4 <= cloud.size();) {
        const size_t m = (size_t)cloud[at];
        if (at + 4 + 3 * m > cloud.size()) return 3;
        tree.insertPointCloud(cloud.data() + at + 4, m, cloud.data() + at + 1, tree.rayParams().max_range);
        at += 4 + 3 * m;
      }
    } else {
      // --- main.cpp:503-558: one node per iteration, the pose the caller pairs with it -----------------------------------------
      for (int i = 0; i < n; i++)
        tree.insertRays(planes.data() + (size_t)i * W * H, W, H, scale, model[0], poses.data() + 12 * (size_t)i);
    }
    std::printf("size %zu overflow %llu\n", tree.size(), (unsigned long long)tree.overflow());
    // --- main.cpp:560 -------------------------------------------------------------------------------------------------------
    tree.writeBinaryLogOdds(argv[10]);
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  return 0;
}
