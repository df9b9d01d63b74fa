// The reference's two matching calls (matchingNoGuess / matchingGuess, src/slam/src/core/Registration.cpp) through
// include/sbm_match.hpp: descriptors, 3-D points, keypoints, guessCameraRef and K read from raw files, run with the reference's
// types when OpenCV headers are present (-DSBM_TEST_WITH_OPENCV; std::multimap results), through the plain form otherwise.
// Written out: the no-guess pair count (int32) and its (from, to) pairs, then the same for the guided call.
//
//   match_callsite_main <desc_from.raw> <desc_to.raw> <xyz_from.raw> <kpts_to.raw> <T.raw> <K.raw> <width> <height> <out.raw>
// Exit codes: 3 = unreadable input, 4 = an sbm::Error, whose status is printed.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "sbm_match.hpp"

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

static void put(FILE* o, const std::vector<std::pair<int, int>>& p) {
  const int k = (int)p.size();
  std::fwrite(&k, sizeof(int), 1, o);
  for (const auto& pq : p) {
    std::fwrite(&pq.first, sizeof(int), 1, o);
    std::fwrite(&pq.second, sizeof(int), 1, o);
  }
}

int main(int argc, char** argv) {
  if (argc != 10) return 2;
  std::vector<uint8_t> df, dt;
  std::vector<float> xyz, kt, T;
  std::vector<double> K;
  if (!read_all(argv[1], df) || !read_all(argv[2], dt) || !read_all(argv[3], xyz) || !read_all(argv[4], kt) ||
      !read_all(argv[5], T) || !read_all(argv[6], K) || T.size() != 12 || K.size() != 4)
    return 3;
  const int W = std::atoi(argv[7]), H = std::atoi(argv[8]);
  const int nf = (int)(df.size() / 32), nt = (int)(dt.size() / 32);
  if ((int)xyz.size() != 3 * nf || (int)kt.size() != 2 * nt) return 3;
  std::vector<std::pair<int, int>> a, b;
  try {
#ifdef SBM_TEST_WITH_OPENCV
    cv::Mat descriptorsFrom(nf, 32, CV_8U, df.data()), descriptorsTo(nt, 32, CV_8U, dt.data());
    std::vector<cv::Point3f> kptsFrom3D;
    for (int i = 0; i < nf; i++) kptsFrom3D.push_back(cv::Point3f(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
    std::vector<cv::KeyPoint> kptsTo;
    for (int i = 0; i < nt; i++) kptsTo.push_back(cv::KeyPoint(cv::Point2f(kt[2 * i], kt[2 * i + 1]), 3.f));
    std::multimap<int, int> m0, m1;
    sbm::matchingNoGuess(descriptorsFrom, descriptorsTo, m0);
    sbm::matchingGuess(kptsFrom3D, kptsTo, descriptorsFrom, descriptorsTo, T.data(), K.data(), cv::Size(W, H), m1);
    a.assign(m0.begin(), m0.end());
    b.assign(m1.begin(), m1.end());
#else
    a = sbm::default_matcher().noGuess(df.data(), 32, nf, dt.data(), 32, nt);
    b = sbm::default_matcher().guess(xyz.data(), kt.data(), df.data(), 32, nf, dt.data(), 32, nt, T.data(), K.data(), W, H);
#endif
  } catch (const sbm::Error& e) {
    std::fprintf(stderr, "%d %s\n", e.code, e.what());
    return 4;
  }
  FILE* o = std::fopen(argv[9], "wb");
  if (!o) return 5;
  put(o, a);
  put(o, b);
  std::fclose(o);
  return 0;
}
