// sbm_pgo.h -- what the two files of the pose-graph optimiser share (sbm_pgo.hip: the kernels and the device-touching entry
// points; sbm_pgo_plan.hip: the partition and getConnectedGraph, host only). Internal. Plain C++17 over include/sbm.h and the
// standard library: nothing here needs HIP, and under HIP the rigid-transform arithmetic is device code as well. Nothing here
// contracts a multiply-add.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <vector>

#include "../../include/sbm.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define PGO_FN __host__ __device__ static inline
#else
#define PGO_FN static inline
#endif
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace sbm {

constexpr int kPgoMaxJunctions = 1024;   // the dense Schur complement is (6 * 1024)^2 doubles at most, twice (S and its factor)

// ---- rigid transforms, every sum left to right ------------------------------------------------------------------------------------
struct Rt { double R[3][3], t[3]; };

PGO_FN double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}
PGO_FN void mul33(const double A[3][3], const double B[3][3], double C[3][3]) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[i][j] = dot3(A[i][0], A[i][1], A[i][2], B[0][j], B[1][j], B[2][j]);
}
PGO_FN void mul3v(const double A[3][3], const double v[3], double o[3]) {
  for (int i = 0; i < 3; i++) o[i] = dot3(A[i][0], A[i][1], A[i][2], v[0], v[1], v[2]);
}
PGO_FN Rt load_rt(const double* p) {
  Rt r;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) r.R[i][j] = p[4 * i + j];
    r.t[i] = p[4 * i + 3];
  }
  return r;
}
PGO_FN void store_rt(const Rt& r, double* p) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) p[4 * i + j] = r.R[i][j];
    p[4 * i + 3] = r.t[i];
  }
}
PGO_FN Rt inverse(const Rt& a) {
  Rt r;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r.R[i][j] = a.R[j][i];
  double v[3];
  mul3v(r.R, a.t, v);
  for (int i = 0; i < 3; i++) r.t[i] = -v[i];
  return r;
}
PGO_FN Rt compose(const Rt& a, const Rt& b) {
  Rt r;
  mul33(a.R, b.R, r.R);
  double v[3];
  mul3v(a.R, b.t, v);
  for (int i = 0; i < 3; i++) r.t[i] = v[i] + a.t[i];
  return r;
}

// ---- the partition: host code, no device ------------------------------------------------------------------------------------------
struct PgoPlan {
  int nv = 0, ne = 0, nfree = 0, nslots = 0, nruns = 0, nj = 0, ncoupling = 0, longest = 0;
  std::vector<int> order;        // sorted position -> caller's vertex position
  std::vector<int> ids;          // ascending
  std::vector<int> hidx;         // per sorted vertex: Hessian index, -1 for the fixed one
  std::vector<int> vfree;        // Hessian index -> sorted vertex
  std::vector<int> vi, vj;       // per edge: sorted vertex of from / to
  std::vector<uint8_t> couples;  // per edge
  std::vector<int> inc_ptr, inc, slot_ptr, slot_edge, slot_rc;   // slot_rc: (row, col) Hessian indices, row > col
  std::vector<int> sub;          // per Hessian index h: the slot of (h, h - 1) or -1
  std::vector<int> jpos, jidx, vrun, run_first, run_len, jj;
  std::vector<int> adj_ptr, adj;  // per Hessian index: its off-diagonal blocks, slot * 2 + (1 when it is the block's column)
  // The index arrays the device reads, each with the pointer of the same name in d (where one call keeps them): the one list
  // that both sizes the graph buffer and drives the uploads. ids and couples stay on the host.
  template <class D, class F> void each_index(D& d, F f) const {
    f(vi, d.vi); f(vj, d.vj); f(hidx, d.hidx); f(inc_ptr, d.inc_ptr); f(inc, d.inc); f(slot_ptr, d.slot_ptr);
    f(slot_edge, d.slot_edge); f(sub, d.sub); f(jpos, d.jpos); f(jidx, d.jidx); f(vrun, d.vrun); f(run_first, d.run_first);
    f(run_len, d.run_len); f(jj, d.jj); f(vfree, d.vfree); f(adj_ptr, d.adj_ptr); f(adj, d.adj); f(slot_rc, d.slot_rc);
    f(order, d.order);
  }
};

#pragma GCC visibility push(hidden)   // host functions that cross files (sbm_pgo_plan.hip has them); hidden, so that the
                                      // library's exported names stay the C ABI's
// Links in the caller's multimap order (keyed by `from`): what getConnectedGraph walks and the robust loop thins out.
struct PgoLinks {
  std::vector<int> from, to;
  std::vector<double> meas, info;
  size_t size() const { return from.size(); }
  void append(const PgoLinks& o, size_t k);   // link k of o
};
// host_arrays: poses, meas and info are host memory and are read; the device forms check ids and topology only
int pgo_check(const sbm_pgo_params* p, const sbm_pgo_graph* g, bool host_arrays = true);
// The partition of a checked graph; SBM_ERR_UNSUPPORTED (with P complete) beyond kPgoMaxJunctions junctions.
int pgo_make_plan(const sbm_pgo_params* p, const sbm_pgo_graph* g, PgoPlan& P);
void pgo_plan_info(const PgoPlan& P, sbm_pgo_plan_info* o);
// getConnectedGraph as written: the vertices reached from from_id with their propagated poses, and the kept links' indices.
void pgo_connected(int from_id, const std::map<int, Rt>& in, const PgoLinks& lin, std::map<int, Rt>& out, std::vector<int>& kept);
#pragma GCC visibility pop

}  // namespace sbm
