// The reference's keypoint detection call of the CV_GFTT modes (src/slam/src/core/main.cpp:239) through include/sbm_gftt.hpp:
// an 8-bit frame read from a raw file, handed to generateKeypoints with the reference's signature when OpenCV headers are present
// (-DSBM_TEST_WITH_OPENCV; cv::KeyPoint size = blockSize), through the plain form otherwise. The points are written as float
// pairs (x, y), then the sizes when the overload ran. <stride> >= <width> is the row step of the frame in memory.
//
//   gftt_cv_callsite_main <img.raw> <width> <height> <stride> <kpts_out.raw>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sbm_gftt.hpp"

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]), S = std::atoi(argv[4]);
  if (S < W) return 2;
  std::vector<uint8_t> frame((size_t)S * H, 0x5a);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  size_t got = 0;
  for (int y = 0; y < H; y++) got += std::fread(frame.data() + (size_t)y * S, 1, (size_t)W, f);
  std::fclose(f);
  if (got != (size_t)W * H) return 3;
  std::vector<float> out;
  try {
#ifdef SBM_TEST_WITH_OPENCV
    if (S != W) return 2;   // (the mock's Mat has no step argument)
    cv::Mat imageLeft(H, W, CV_8UC1, frame.data());
    std::vector<cv::KeyPoint> kpts2d;
    // --- main.cpp:239 -----------------------------------------------------------------------------------------------------
    sbm::generateKeypoints(imageLeft, kpts2d);
    for (const cv::KeyPoint& k : kpts2d) { out.push_back(k.pt.x); out.push_back(k.pt.y); }
    for (const cv::KeyPoint& k : kpts2d) out.push_back(k.size);
#else
    sbm::generateKeypoints(frame.data(), (size_t)S, W, H, out);
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
