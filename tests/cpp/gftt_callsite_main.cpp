// The reference's keypoint selection call (src/slam/src/core/main.cpp:241-243) through include/sbm_gftt.hpp: a dense uint16
// eigenvalue map read from a raw file and its Max register, handed to generateKeypoints2 with the reference's signature when
// OpenCV headers are present (-DSBM_TEST_WITH_OPENCV; cv::KeyPoint size = blockSize), through the plain form otherwise. The
// points are written as float pairs (x, y), then the sizes when the overload ran.
//
//   gftt_callsite_main <eig.raw> <width> <height> <max> <kpts_out.raw>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sbm_gftt.hpp"

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
  const unsigned short maxEigen = (unsigned short)std::atoi(argv[4]);
  std::vector<uint16_t> map((size_t)W * H);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  const size_t got = std::fread(map.data(), 2, map.size(), f);
  std::fclose(f);
  if (got != map.size()) return 3;
  std::vector<float> out;
  try {
#ifdef SBM_TEST_WITH_OPENCV
#ifdef SBM_MOCK_OPENCV
    cv::Mat eig(H, W, CV_16S, map.data());   // (the mock has no CV_16U; the element size is what matters)
#else
    cv::Mat eig(H, W, CV_16UC1, map.data());
#endif
    std::vector<cv::KeyPoint> kpts2d;
    // --- main.cpp:241-243 -------------------------------------------------------------------------------------------------
    sbm::generateKeypoints2(eig, maxEigen, kpts2d);
    for (const cv::KeyPoint& k : kpts2d) { out.push_back(k.pt.x); out.push_back(k.pt.y); }
    for (const cv::KeyPoint& k : kpts2d) out.push_back(k.size);
#else
    sbm::generateKeypoints2(map.data(), (size_t)W * 2, W, H, maxEigen, out);
#endif
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  FILE* o = std::fopen(argv[5], "wb");
  if (!o) return 5;
  std::fwrite(out.data(), sizeof(float), out.size(), o);
  std::fclose(o);
  return 0;
}
