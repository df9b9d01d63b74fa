// The reference's estimateMotion call (estimateMotion3DTo2D, src/slam/src/core/Registration.cpp:337-397) through
// include/sbm_pnp.hpp: n correspondences with their VW ids, the from-frame's 3-D points, the to-frame's keypoints and 3-D points,
// K and the localTransform read from raw files; run with the reference's std::map types when OpenCV headers are present
// (-DSBM_TEST_WITH_OPENCV), through the plain form otherwise. A NaN from-point stands for an id words3A does not hold.
// Written out: status, then the 12 transform floats, the 36 covariance doubles, the match count and ids, the inlier count and ids.
//
//   pnp_callsite_main <ids.raw> <xyz_from.raw> <kpts_to.raw> <xyz_to.raw> <K.raw> <local.raw> <min_inliers> <refine> <out.raw>
// Exit codes: 3 = unreadable input, 4 = an sbm::Error, whose status is printed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "sbm_pnp.hpp"

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

static void put_ids(FILE* o, const std::vector<int>& v) {
  const int k = (int)v.size();
  std::fwrite(&k, sizeof(int), 1, o);
  if (k) std::fwrite(v.data(), sizeof(int), v.size(), o);
}

int main(int argc, char** argv) {
  if (argc != 10) return 2;
  std::vector<int> ids;
  std::vector<float> xa, kb, xb, local;
  std::vector<double> K;
  if (!read_all(argv[1], ids) || !read_all(argv[2], xa) || !read_all(argv[3], kb) || !read_all(argv[4], xb) ||
      !read_all(argv[5], K) || !read_all(argv[6], local) || K.size() != 4 || (local.size() != 12 && !local.empty()))
    return 3;
  const int n = (int)ids.size();
  if ((int)xa.size() != 3 * n || (int)kb.size() != 2 * n || (int)xb.size() != 3 * n) return 3;
  const int min_inliers = std::atoi(argv[7]), refine = std::atoi(argv[8]);
  const float* lt = local.empty() ? nullptr : local.data();
  sbm::Motion m;
  try {
#ifdef SBM_TEST_WITH_OPENCV
    std::map<int, cv::Point3f> words3A, words3B;
    std::map<int, cv::KeyPoint> wordsB;
    for (int i = 0; i < n; i++) {
      if (!std::isnan(xa[3 * i])) words3A[ids[i]] = cv::Point3f(xa[3 * i], xa[3 * i + 1], xa[3 * i + 2]);
      words3B[ids[i]] = cv::Point3f(xb[3 * i], xb[3 * i + 1], xb[3 * i + 2]);
      wordsB[ids[i]] = cv::KeyPoint(cv::Point2f(kb[2 * i], kb[2 * i + 1]), 3.f);
    }
    m = sbm::estimateMotion3DTo2D(words3A, wordsB, K.data(), lt, min_inliers, refine, words3B);
#else
    m = sbm::default_motion_estimator().estimate(xa.data(), kb.data(), xb.data(), ids.data(), n, K.data(), lt, min_inliers, refine);
#endif
  } catch (const sbm::Error& e) {
    std::fprintf(stderr, "%d %s\n", e.code, e.what());
    return 4;
  }
  FILE* o = std::fopen(argv[9], "wb");
  if (!o) return 5;
  std::fwrite(&m.status, sizeof(int), 1, o);
  std::fwrite(m.transform, sizeof(float), 12, o);
  std::fwrite(m.covariance, sizeof(double), 36, o);
  put_ids(o, m.matches);
  put_ids(o, m.inliers);
  std::fclose(o);
  return 0;
}
