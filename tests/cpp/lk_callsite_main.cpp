// The reference's sparse-depth call (src/slam/src/core/Stereo.cpp:136) through include/sbm_lkstereo.hpp: an 8-bit pair and the
// left points (float pairs) read from raw files, handed to computeCorrespondences with the reference's signature when OpenCV
// headers are present (-DSBM_TEST_WITH_OPENCV), through the plain form otherwise. One line per point is printed:
// "<right.x bits> <right.y bits> <status>", the floats as 8 hex digits. <stride> >= <width> is the row step of both frames in
// memory. A failure prints "error <code>" and exits with 4.
//
//   lk_callsite_main <left.raw> <right.raw> <width> <height> <stride> <pts.raw>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sbm_lkstereo.hpp"

static bool read_frame(const char* path, int W, int H, int S, std::vector<uint8_t>& frame) {
  frame.assign((size_t)S * H, 0x5a);
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  size_t got = 0;
  for (int y = 0; y < H; y++) got += std::fread(frame.data() + (size_t)y * S, 1, (size_t)W, f);
  std::fclose(f);
  return got == (size_t)W * H;
}

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), S = std::atoi(argv[5]);
  if (S < W || W <= 0 || H <= 0) return 2;
  std::vector<uint8_t> left, right;
  if (!read_frame(argv[1], W, H, S, left) || !read_frame(argv[2], W, H, S, right)) return 3;
  std::vector<float> xy;
  {
    FILE* f = std::fopen(argv[6], "rb");
    if (!f) return 3;
    float v[2];
    while (std::fread(v, sizeof(float), 2, f) == 2) { xy.push_back(v[0]); xy.push_back(v[1]); }
    std::fclose(f);
  }
  std::vector<float> out;
  std::vector<unsigned char> status;
  try {
#ifdef SBM_TEST_WITH_OPENCV
    if (S != W) return 2;   // (the mock's Mat has no step argument)
    const cv::Mat imageLeft(H, W, CV_8UC1, left.data()), imageRight(H, W, CV_8UC1, right.data());
    std::vector<cv::Point2f> leftCorners, rightCorners;
    for (size_t i = 0; i < xy.size() / 2; i++) leftCorners.push_back(cv::Point2f(xy[2 * i], xy[2 * i + 1]));
    // --- Stereo.cpp:136 -----------------------------------------------------------------------------------------------------
    rightCorners = sbm::computeCorrespondences(imageLeft, imageRight, leftCorners, status);
    for (const cv::Point2f& p : rightCorners) { out.push_back(p.x); out.push_back(p.y); }
#else
    out = sbm::computeCorrespondences(left.data(), (size_t)S, right.data(), (size_t)S, W, H, xy, status);
#endif
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  for (size_t i = 0; i < status.size(); i++) {
    uint32_t bx, by;
    std::memcpy(&bx, &out[2 * i], 4);
    std::memcpy(&by, &out[2 * i + 1], 4);
    std::printf("%08x %08x %d\n", bx, by, (int)status[i]);
  }
  return 0;
}
