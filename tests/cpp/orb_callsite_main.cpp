// The reference's descriptor call (src/slam/src/core/main.cpp:246-248) through include/sbm_orb.hpp: a dense u8 frame, float
// keypoints and the sampling pattern read from raw files; the pattern is handed over with sbm::setOrbPattern, then
// computeDescriptor runs with the reference's signature when OpenCV headers are present (-DSBM_TEST_WITH_OPENCV; cv::KeyPoint
// with angle -1 and size 3, as generateKeypoints2 makes them), through the plain form otherwise. Written out: the number of
// kept points (int32), their (x, y) as float pairs, then their descriptors (32 bytes each).
//
//   orb_callsite_main <img.raw> <width> <height> <kpts.raw> <pattern.raw> <out.raw>
// Exit codes: 4 = an sbm::Error, whose status is printed; 6 = computeDescriptor without a pattern did not throw SBM_ERR_NULL.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sbm_orb.hpp"

template <class T>
static bool read_all(const char* path, std::vector<T>& v) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)n / sizeof(T));
  const size_t got = std::fread(v.data(), sizeof(T), v.size(), f);
  std::fclose(f);
  return got == v.size();
}

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
  std::vector<uint8_t> img;
  std::vector<float> xy;
  std::vector<int> pattern;
  if (!read_all(argv[1], img) || !read_all(argv[4], xy) || !read_all(argv[5], pattern) || img.size() != (size_t)W * H ||
      pattern.size() != 1024)
    return 3;
  std::vector<uint8_t> desc;
  int k = 0;
  try {
    try {   // the free function has no pattern yet
      std::vector<float> t(xy);
      sbm::computeDescriptor(img.data(), (size_t)W, W, H, t, desc);
      return 6;
    } catch (const sbm::Error& e) {
      if (e.code != SBM_ERR_NULL) return 6;
    }
    sbm::setOrbPattern(pattern.data());
#ifdef SBM_TEST_WITH_OPENCV
    cv::Mat imageLeft(H, W, CV_8U, img.data());
    std::vector<cv::KeyPoint> kpts2d;
    for (size_t i = 0; i + 1 < xy.size(); i += 2) kpts2d.push_back(cv::KeyPoint(cv::Point2f(xy[i], xy[i + 1]), 3.f));
    cv::Mat d;
    // --- main.cpp:246-248 -------------------------------------------------------------------------------------------------
    sbm::computeDescriptor(imageLeft, cv::noArray(), kpts2d, true, d);
    k = (int)kpts2d.size();
    if (d.rows != k) return 7;
    xy.clear();
    for (const cv::KeyPoint& kp : kpts2d) {
      if (kp.size != 3.f) return 8;
      xy.push_back(kp.pt.x);
      xy.push_back(kp.pt.y);
    }
    desc.assign(d.ptr<uint8_t>(0), d.ptr<uint8_t>(0) + (size_t)k * 32);
#else
    sbm::computeDescriptor(img.data(), (size_t)W, W, H, xy, desc);
    k = (int)(xy.size() / 2);
#endif
  } catch (const sbm::Error& e) {
    std::fprintf(stderr, "%d %s\n", e.code, e.what());
    return 4;
  }
  FILE* o = std::fopen(argv[6], "wb");
  if (!o) return 5;
  std::fwrite(&k, sizeof(int), 1, o);
  std::fwrite(xy.data(), sizeof(float), xy.size(), o);
  std::fwrite(desc.data(), 1, desc.size(), o);
  std::fclose(o);
  return 0;
}
