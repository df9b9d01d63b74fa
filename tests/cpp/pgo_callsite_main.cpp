// The reference's call site src/slam/src/core/main.cpp:328 through include/sbm_pgo.hpp, against a stand-in for the caller's map
// types: Transform (twelve floats, the reference's accessors and its constructor from doubles) and Link (from, to, transform,
// a 6 x 6 double matrix with at<double>). A square of four poses with one loop closure; prints the return value and the number
// of poses. Built by tests/test_pgo_cabi.py (compile and link only; running it needs a GPU).
#include <cstdio>
#include <map>

#include "sbm_pgo.hpp"

struct Transform {   // stand-in for core/Transform.h
  float m[12];
  Transform() : m{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0} {}
  Transform(double r11, double r12, double r13, double o14, double r21, double r22, double r23, double o24, double r31, double r32,
            double r33, double o34)
      : m{(float)r11, (float)r12, (float)r13, (float)o14, (float)r21, (float)r22, (float)r23, (float)o24, (float)r31, (float)r32,
          (float)r33, (float)o34} {}
  float r11() const { return m[0]; } float r12() const { return m[1]; } float r13() const { return m[2]; } float o14() const { return m[3]; }
  float r21() const { return m[4]; } float r22() const { return m[5]; } float r23() const { return m[6]; } float o24() const { return m[7]; }
  float r31() const { return m[8]; } float r32() const { return m[9]; } float r33() const { return m[10]; } float o34() const { return m[11]; }
};
struct Mat66 {   // stand-in for cv::Mat(6, 6, CV_64FC1)
  double v[36];
  template <class T> const T& at(int r, int c) const { return v[6 * r + c]; }
};
struct Link {    // stand-in for core/Link.h
  int from_, to_;
  Transform t_;
  Mat66 inf_;
  int from() const { return from_; }
  int to() const { return to_; }
  const Transform& transform() const { return t_; }
  const Mat66& infMatrix() const { return inf_; }
};

int main() {
  std::map<int, Transform> poses, optimized_poses;
  std::multimap<int, Link> links;
  Mat66 eye = {};
  for (int i = 0; i < 6; i++) eye.v[7 * i] = 1.0;
  const Transform step(1, 0, 0, 1.0, 0, 1, 0, 0, 0, 0, 1, 0);
  for (int id = 1; id <= 4; id++) poses[id] = Transform(1, 0, 0, 1.05 * (id - 1), 0, 1, 0, 0.01 * id, 0, 0, 1, 0);
  for (int id = 1; id < 4; id++) links.insert(std::make_pair(id, Link{id, id + 1, step, eye}));
  links.insert(std::make_pair(4, Link{4, 1, Transform(1, 0, 0, -3.0, 0, 1, 0, 0, 0, 0, 1, 0), eye}));
  sbm_params bm;
  sbm_params_default(&bm, 0, 0);
  sbm_handle* h = nullptr;
  if (sbm_create(&h, &bm, 0) != SBM_OK) return 3;
  try {
    // --- main.cpp:328 --------------------------------------------------------------------------------------------------------
    const double err = sbm::runOptimizeRobust(h, poses, links, 20, &optimized_poses);
    const double err2 = sbm::runOptimize(h, poses, links, 5, &optimized_poses);
    std::printf("err %g %g poses %zu\n", err, err2, optimized_poses.size());
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    sbm_destroy(h);
    return 4;
  }
  sbm_destroy(h);
  return 0;
}
