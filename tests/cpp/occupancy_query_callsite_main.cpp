// A call site of octomap's read side through include/sbm_occupancy.hpp: a tree filled with insertPointCloud, then per ray
//
//     octomap::point3d end;  bool hit = tree.castRay(origin, direction, end, ignoreUnknownCells, maxRange);
//
// and per point tree.search(x, y, z), with sbm::OccupancyMap in the tree's place. The cloud (per scan: a float count, three
// floats of origin, then the triples), the rays (eight doubles each: origin, direction, ignoreUnknownCells, maxRange) and the
// points (float triples) are read from files. Per ray the output file receives an int32 return value, an int32 status and the
// three floats of `end`, which the caller set to NaN before the call as the fixture's driver does; then per point an int32 state
// and the float log-odds. The second half of the rays goes through castRays in one batch. A failure prints "error <code>" and
// exits with 4.
//
//   occupancy_query_callsite_main <cloud.raw> <floats> <max_range> <capacity> <rays.raw> <rays> <points.raw> <points> <out.raw>
#include <cmath>
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
  if (argc != 10) return 2;
  std::vector<float> cloud, points;
  std::vector<double> rays;
  const size_t nrays = (size_t)std::atoll(argv[6]), npoints = (size_t)std::atoll(argv[8]);
  if (!read_all(argv[1], cloud, (size_t)std::atoll(argv[2])) || !read_all(argv[5], rays, 8 * nrays) ||
      !read_all(argv[7], points, 3 * npoints))
    return 3;
  FILE* out = std::fopen(argv[9], "wb");
  if (!out) return 3;
  try {
    sbm::OccupancyMap tree((size_t)std::atoll(argv[4]), 0.1);
    for (size_t at = 0; at + 4 <= cloud.size();) {
      const size_t m = (size_t)cloud[at];
      if (at + 4 + 3 * m > cloud.size()) return 3;
      tree.insertPointCloud(cloud.data() + at + 4, m, cloud.data() + at + 1, std::atof(argv[3]));
      at += 4 + 3 * m;
    }
    const size_t single = nrays / 2;
    for (size_t i = 0; i < single; i++) {
      const double* r = &rays[8 * i];
      const float origin[3] = {(float)r[0], (float)r[1], (float)r[2]}, direction[3] = {(float)r[3], (float)r[4], (float)r[5]};
      float end[3] = {NAN, NAN, NAN};
      int status = 0;
      const int32_t hit = tree.castRay(origin, direction, end, r[6] != 0, r[7], &status) ? 1 : 0, st = status;
      std::fwrite(&hit, 4, 1, out);
      std::fwrite(&st, 4, 1, out);
      std::fwrite(end, 4, 3, out);
    }
    // the rest in batches of equal (ignoreUnknownCells, maxRange)
    for (size_t a = single; a < nrays;) {
      size_t b = a + 1;
      while (b < nrays && rays[8 * b + 6] == rays[8 * a + 6] && rays[8 * b + 7] == rays[8 * a + 7]) b++;
      std::vector<float> o, d, e(3 * (b - a));
      std::vector<int32_t> st(b - a);
      for (size_t i = a; i < b; i++)
        for (int j = 0; j < 3; j++) {
          o.push_back((float)rays[8 * i + j]);
          d.push_back((float)rays[8 * i + 3 + j]);
        }
      tree.castRays(o.data(), false, d.data(), b - a, st.data(), e.data(), rays[8 * a + 6] != 0, rays[8 * a + 7]);
      for (size_t i = 0; i < b - a; i++) {
        const int32_t hit = st[i] == SBM_OCC_RAY_HIT;
        std::fwrite(&hit, 4, 1, out);
        std::fwrite(&st[i], 4, 1, out);
        std::fwrite(&e[3 * i], 4, 3, out);
      }
      a = b;
    }
    for (size_t i = 0; i < npoints; i++) {
      float value = 0.f;
      const int32_t state = tree.search(points[3 * i], points[3 * i + 1], points[3 * i + 2], &value);
      std::fwrite(&state, 4, 1, out);
      std::fwrite(&value, 4, 1, out);
    }
    std::printf("size %zu rays %zu points %zu\n", tree.size(), nrays, npoints);
  } catch (const sbm::Error& e) {
    std::printf("error %d\n", e.code);
    return 4;
  }
  std::fclose(out);
  return 0;
}
