// The host half of the pose-graph optimiser (u96-slam_amd/csrc/sbm_pgo_plan.hip) on one graph, without the engine library:
// tests/test_pgo_plan_host.py compiles this file and that one as host C++ under the address and undefined-behaviour sanitizers.
// argv[1]: a file of int32 words nv, ne, run_max, coupling, fixed_id, then ids[nv], from[ne], to[ne], then float64 poses[12 nv],
// meas[12 ne]. Prints pgo_check's status, the plan, and what pgo_connected reaches from fixed_id (poses as hex doubles).
#include <stdio.h>

#include <map>
#include <vector>

#include "sbm_pgo.h"

using namespace sbm;

template <class T> static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <class V> static void print_ints(const char* name, const V& v) {
  printf("%s", name);
  for (auto x : v) printf(" %d", (int)x);
  printf("\n");
}

int main(int argc, char** argv) {
  FILE* f = argc == 2 ? fopen(argv[1], "rb") : nullptr;
  std::vector<int32_t> head, ids, from, to;
  std::vector<double> poses, meas;
  if (!f || !read_n(f, head, 5) || head[0] < 0 || head[1] < 0) return 2;
  const size_t nv = (size_t)head[0], ne = (size_t)head[1];
  if (!read_n(f, ids, nv) || !read_n(f, from, ne) || !read_n(f, to, ne) || !read_n(f, poses, 12 * nv) || !read_n(f, meas, 12 * ne))
    return 2;
  fclose(f);
  const std::vector<double> info(36 * ne + 1, 0.0);   // pgo_check reads it; neither the plan nor pgo_connected does
  sbm_pgo_params p = {20, head[4], head[3], head[2]};
  const sbm_pgo_graph g = {head[0], ids.data(), poses.data(), head[1], from.data(), to.data(), meas.data(), info.data()};
  int st = pgo_check(&p, &g);
  printf("check %d\n", st);
  if (st != SBM_OK) return 0;

  PgoPlan P;
  st = pgo_make_plan(&p, &g, P);
  printf("plan %d\n", st);
  sbm_pgo_plan_info o;
  pgo_plan_info(P, &o);
  printf("counts %d %d %d %d %d %d %d %d\n", o.n_free, o.n_runs, o.n_junctions, o.schur_size, o.n_coupling, o.longest_run, o.n_slots,
         o.max_junctions);
  print_ints("vrun", P.vrun);
  print_ints("slot_rc", P.slot_rc);
  print_ints("couples", P.couples);

  std::map<int, Rt> in, out;
  for (size_t i = 0; i < nv; i++) in[ids[i]] = load_rt(&poses[12 * i]);
  PgoLinks all, lin;
  all.from.assign(from.begin(), from.end());
  all.to.assign(to.begin(), to.end());
  all.meas = meas;
  all.info = info;
  for (size_t k = 0; k < ne; k++) lin.append(all, k);   // the helper of the robust loop
  std::vector<int> kept;
  pgo_connected(p.fixed_id, in, lin, out, kept);
  printf("reached");
  for (const auto& kv : out) printf(" %d", kv.first);
  printf("\nposes");
  for (const auto& kv : out) {
    double q[12];
    store_rt(kv.second, q);
    for (double v : q) printf(" %a", v);
  }
  printf("\n");
  print_ints("kept", kept);
  return 0;
}
