// Stand-alone host check of the planners' host arithmetic (u96-slam_amd/csrc/sbm_occ.h: occ_key_to_coord, occ_coord_to_key_at,
// occ_unknown_plan, occ_unknown_axis, occ_metric_fold) under AddressSanitizer and UndefinedBehaviorSanitizer, at its boundaries:
// corners at and beyond both ends of the key space, NaN and infinite corners, every depth, pmax below pmin, the largest grid a
// call accepts and the first it refuses, axis tables filled into exact-size heap arrays (a table that runs past its step count is
// seen), and the metric fold at the extreme keys of every depth. Built and run by hand on the host: the helpers are plain C++ (no
// HIP header, no HIP call), so the tool and the header are the whole program; it never touches a GPU:
//
//     c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include \
//         tools/occupancy_planner_sanitize.cpp -o occ_planner_san && ./occ_planner_san
//
// Prints the number of checks; a finding ends the run with the sanitizer's report, a wrong answer with exit code 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../u96-slam_amd/csrc/sbm_occ.h"

static long checks = 0;
static void expect(bool ok, const char* what, double a = 0, double b = 0) {
  checks++;
  if (ok) return;
  std::printf("wrong: %s (%.17g, %.17g)\n", what, a, b);
  std::exit(1);
}

int main() {
  const double res = 0.1, factor = 1. / res;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  unsigned key = 7;
  // corners: the ends of the key space at every depth, and what lies beyond
  for (int depth = 1; depth <= 16; depth++) {
    expect(sbm::occ_coord_to_key_at(factor, -3276.75f, depth, &key) && key == (depth == 16 ? 0u : 1u << (15 - depth)), "the lowest key", depth, key);
    expect(sbm::occ_coord_to_key_at(factor, 3276.75f, depth, &key) && key == (depth == 16 ? 65535u : 65536u - (1u << (15 - depth))), "the highest key",
           depth, key);
    key = 7;
    for (float c : {-3276.81f, 3276.8f, 1e9f, -1e9f, 3e38f, -3e38f, nan, inf, -inf})
      expect(!sbm::occ_coord_to_key_at(factor, c, depth, &key) && key == 7, "a corner outside the key space", depth, c);
    expect(sbm::occ_key_to_coord(32768, depth, res) > 0 && sbm::occ_key_to_coord(32767, depth, res) < 0, "keyToCoord around zero", depth);
  }
  expect(sbm::occ_key_to_coord(123, 0, res) == 0.0, "the root's centre");
  // the plan: depths, equal corners, pmax below pmin, the cell limit
  sbm::OccUnknownPlan p;
  const float zero[3] = {0, 0, 0}, one[3] = {1, 1, 1};
  for (int depth : {-1, 17, 1 << 30, -(1 << 30)}) expect(sbm::occ_unknown_plan(res, zero, one, depth, &p) == SBM_ERR_SIZE, "a depth outside 0..16", depth);
  for (int depth = 0; depth <= 16; depth++) {
    expect(sbm::occ_unknown_plan(res, zero, zero, depth, &p) == SBM_OK && !p.steps[0] && !p.steps[1] && !p.steps[2], "pmin == pmax", depth);
    expect(sbm::occ_unknown_plan(res, one, zero, depth, &p) == SBM_OK && !p.steps[0] && !p.steps[1] && !p.steps[2], "pmax below pmin", depth);
    const float lo[3] = {-3276.75f, -3276.75f, -3276.75f}, hi[3] = {3276.75f, 3276.75f, 3276.75f};
    const int st = sbm::occ_unknown_plan(res, lo, hi, depth, &p);
    const size_t cells = (size_t)p.steps[0] * p.steps[1] * p.steps[2];
    expect(st == (cells > sbm::kOccUnknownMaxCells ? SBM_ERR_UNSUPPORTED : SBM_OK) && p.steps[0] <= 65536, "the whole key space", depth, (double)cells);
  }
  const float bad[3] = {0, nan, 0}, far[3] = {0, 0, 3276.8f};
  expect(sbm::occ_unknown_plan(res, bad, one, 0, &p) == SBM_ERR_SIZE && sbm::occ_unknown_plan(res, zero, far, 0, &p) == SBM_ERR_SIZE, "a corner without a key");
  const float lo[3] = {-51.25f, -51.25f, -51.25f};
  for (float top : {51.05f, 51.15f, 51.25f, 51.35f}) {   // around 1024 steps per axis: 2^30 cells are accepted, one more step is not
    const float hi[3] = {top, top, top};
    const int st = sbm::occ_unknown_plan(res, lo, hi, 16, &p);
    const size_t cells = (size_t)p.steps[0] * p.steps[1] * p.steps[2];
    expect(st == (cells > sbm::kOccUnknownMaxCells ? SBM_ERR_UNSUPPORTED : SBM_OK), "the cell limit", top, (double)cells);
    expect(p.steps[0] >= 1022 && p.steps[0] <= 1026, "about 1024 steps", p.steps[0]);
  }
  // the axis tables: exact-size arrays, every entry the running float sum
  for (uint32_t n : {0u, 1u, 2u, 65u, 4096u, 65536u}) {
    float* t = new float[n ? n : 1];
    sbm::occ_unknown_axis(-3276.75f, 0.1f, n, t);
    volatile float run = -3276.75f;
    for (uint32_t i = 0; i < n; i++) {
      run = run + 0.1f;
      if (t[i] != run) expect(false, "a table entry", i, t[i]);
    }
    expect(true, "a table");
    delete[] t;
  }
  // the metric fold at the extreme keys of every depth, and the empty fold
  for (int depth = 0; depth <= 16; depth++) {
    const unsigned half = depth < 16 ? 1u << (15 - depth) : 0u;
    const unsigned kmin[3] = {half, half, half}, kmax[3] = {depth ? 65536u - (depth < 16 ? half : 1u) : half, 40000u | half, half};
    double lo3[3] = {1.7976931348623157e308, 1.7976931348623157e308, 1.7976931348623157e308}, hi3[3] = {-lo3[0], -lo3[0], -lo3[0]};
    sbm::occ_metric_fold(depth, kmin, kmax, res, lo3, hi3);
    expect(std::fabs(lo3[0] + 3276.8) < 1e-9 && std::fabs(hi3[0] - 3276.8) < 1e-9, "the bounds of the whole key space", lo3[0], hi3[0]);
    expect(lo3[2] < hi3[2] && std::fabs(hi3[2] - lo3[2] - res * (double)(1 << (16 - depth))) < 1e-9, "one node's size", depth, hi3[2] - lo3[2]);
  }
  std::printf("%ld checks\n", checks);
  return 0;
}
