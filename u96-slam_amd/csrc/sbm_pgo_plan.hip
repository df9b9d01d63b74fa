// sbm_pgo_plan.hip -- the host half of the pose-graph optimiser: the checks, the partition into runs and junctions (PgoPlan),
// getConnectedGraph of Mapper.cpp for the robust loop, and the three entry points that never touch a device.
// Host only: no HIP header and no HIP call, so any C++17 compiler builds this file alone (tests/cpp/pgo_plan_main.cpp does, under
// the host sanitizers). sbm_pgo.hip has the kernels and everything that uses the handle.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <new>

#include "sbm_pgo.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace sbm {

int pgo_check(const sbm_pgo_params* p, const sbm_pgo_graph* g, bool host_arrays) {
  if (!p || !g) return SBM_ERR_NULL;
  if (p->num < 0) return SBM_ERR_SIZE;
  if (p->coupling != SBM_PGO_COUPLING_REFERENCE && p->coupling != SBM_PGO_COUPLING_SYMMETRIC) return SBM_ERR_UNSUPPORTED;
  if (p->run_max < 1 || p->run_max > 65536) return SBM_ERR_UNSUPPORTED;
  if (g->n_vertices <= 0 || g->n_edges < 0) return SBM_ERR_SIZE;              // an empty graph
  if (!g->ids || !g->poses || (g->n_edges > 0 && (!g->from || !g->to || !g->meas || !g->info))) return SBM_ERR_NULL;
  for (size_t i = 0; host_arrays && i < 12 * (size_t)g->n_vertices; i++)
    if (!std::isfinite(g->poses[i])) return SBM_ERR_UNSUPPORTED;
  for (size_t i = 0; host_arrays && i < 12 * (size_t)g->n_edges; i++)
    if (!std::isfinite(g->meas[i])) return SBM_ERR_UNSUPPORTED;
  for (size_t i = 0; host_arrays && i < 36 * (size_t)g->n_edges; i++)
    if (!std::isfinite(g->info[i])) return SBM_ERR_UNSUPPORTED;
  try {
    std::vector<int> ids(g->ids, g->ids + g->n_vertices);
    std::sort(ids.begin(), ids.end());
    if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return SBM_ERR_SIZE;   // a vertex id given twice
    if (!std::binary_search(ids.begin(), ids.end(), p->fixed_id)) return SBM_ERR_SIZE;  // an absent fixed_id
    for (int k = 0; k < g->n_edges; k++) {
      if (g->from[k] == g->to[k]) return SBM_ERR_UNSUPPORTED;
      if (!std::binary_search(ids.begin(), ids.end(), g->from[k]) || !std::binary_search(ids.begin(), ids.end(), g->to[k]))
        return SBM_ERR_SIZE;                                                            // an edge naming an absent vertex
    }
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return SBM_OK;
}

// Junctions: both ends of every coupling between Hessian indices that are not neighbours, and every (run_max + 1)-th vertex of a
// longer stretch. Runs: the maximal stretches of consecutive indices between junctions.
int pgo_make_plan(const sbm_pgo_params* p, const sbm_pgo_graph* g, PgoPlan& P) {
  try {
    const int nv = g->n_vertices, ne = g->n_edges;
    P.nv = nv; P.ne = ne;
    P.order.resize(nv);
    for (int i = 0; i < nv; i++) P.order[i] = i;
    std::sort(P.order.begin(), P.order.end(), [&](int a, int b) { return g->ids[a] < g->ids[b]; });
    P.ids.resize(nv); P.hidx.resize(nv);
    for (int i = 0; i < nv; i++) {
      P.ids[i] = g->ids[P.order[i]];
      P.hidx[i] = P.ids[i] == p->fixed_id ? -1 : P.nfree++;
      if (P.hidx[i] >= 0) P.vfree.push_back(i);
    }
    const int nf = P.nfree;
    P.vi.resize(ne); P.vj.resize(ne); P.couples.assign(ne, 0);
    std::vector<std::vector<int>> inc(nf);
    std::map<std::pair<int, int>, std::vector<int>> slots;
    for (int k = 0; k < ne; k++) {
      P.vi[k] = (int)(std::lower_bound(P.ids.begin(), P.ids.end(), g->from[k]) - P.ids.begin());
      P.vj[k] = (int)(std::lower_bound(P.ids.begin(), P.ids.end(), g->to[k]) - P.ids.begin());
      const int hi = P.hidx[P.vi[k]], hj = P.hidx[P.vj[k]];
      if (hi >= 0) inc[hi].push_back(2 * k);
      if (hj >= 0) inc[hj].push_back(2 * k + 1);
      // the one off-diagonal block, at (to, from): SimplicialLDLT reads it only from the lower triangle; where `to` is fixed
      // the reference forms a negative index, here the coupling is dropped
      const bool both = hi >= 0 && hj >= 0;
      if (both && (hj > hi || p->coupling == SBM_PGO_COUPLING_SYMMETRIC)) {
        P.couples[k] = 1;
        P.ncoupling++;
        if (hj > hi) slots[{hj, hi}].push_back(2 * k);        // m^T
        else slots[{hi, hj}].push_back(2 * k + 1);            // mirrored from the upper triangle: m
      }
    }
    P.inc_ptr.assign(nf + 1, 0);
    for (int h = 0; h < nf; h++) {
      P.inc_ptr[h + 1] = P.inc_ptr[h] + (int)inc[h].size();
      P.inc.insert(P.inc.end(), inc[h].begin(), inc[h].end());
    }
    P.sub.assign(nf, -1);
    P.jpos.assign(nf, -1);
    P.slot_ptr.push_back(0);
    for (const auto& s : slots) {
      const int r = s.first.first, c = s.first.second;
      if (r - c == 1) P.sub[r] = P.nslots;
      else P.jpos[r] = P.jpos[c] = 0;                          // marked; numbered below
      P.slot_rc.push_back(r); P.slot_rc.push_back(c);
      P.slot_edge.insert(P.slot_edge.end(), s.second.begin(), s.second.end());
      P.slot_ptr.push_back((int)P.slot_edge.size());
      P.nslots++;
    }
    int streak = 0;
    for (int h = 0; h < nf; h++) {
      if (P.jpos[h] >= 0) { streak = 0; continue; }
      if (++streak > p->run_max) { P.jpos[h] = 0; streak = 0; }
    }
    P.vrun.assign(nf, -1);
    for (int h = 0; h < nf; h++) {
      if (P.jpos[h] >= 0) { P.jpos[h] = P.nj++; P.jidx.push_back(h); continue; }
      if (h == 0 || P.jpos[h - 1] >= 0) { P.run_first.push_back(h); P.run_len.push_back(0); P.nruns++; }
      P.vrun[h] = P.nruns - 1;
      P.longest = std::max(P.longest, ++P.run_len.back());
    }
    std::vector<std::vector<int>> adj(nf);
    for (int s = 0; s < P.nslots; s++) {
      adj[P.slot_rc[2 * s]].push_back(2 * s);
      adj[P.slot_rc[2 * s + 1]].push_back(2 * s + 1);
    }
    P.adj_ptr.assign(nf + 1, 0);
    for (int h = 0; h < nf; h++) {
      P.adj_ptr[h + 1] = P.adj_ptr[h] + (int)adj[h].size();
      P.adj.insert(P.adj.end(), adj[h].begin(), adj[h].end());
    }
    for (int s = 0; s < P.nslots; s++) {
      const int r = P.slot_rc[2 * s], c = P.slot_rc[2 * s + 1];
      if (P.jpos[r] >= 0 && P.jpos[c] >= 0) { P.jj.push_back(s); P.jj.push_back(P.jpos[r]); P.jj.push_back(P.jpos[c]); }
    }
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return P.nj > kPgoMaxJunctions ? SBM_ERR_UNSUPPORTED : SBM_OK;
}

void pgo_plan_info(const PgoPlan& P, sbm_pgo_plan_info* o) {
  o->n_free = P.nfree; o->n_runs = P.nruns; o->n_junctions = P.nj; o->schur_size = 6 * P.nj; o->n_coupling = P.ncoupling;
  o->longest_run = P.longest; o->n_slots = P.nslots; o->max_junctions = kPgoMaxJunctions;
}

void PgoLinks::append(const PgoLinks& o, size_t k) {
  from.push_back(o.from[k]);
  to.push_back(o.to[k]);
  meas.insert(meas.end(), &o.meas[12 * k], &o.meas[12 * k] + 12);
  info.insert(info.end(), &o.info[36 * k], &o.info[36 * k] + 36);
}

// On links in the caller's multimap order (keyed by `from`). Propagation in double.
void pgo_connected(int from_id, const std::map<int, Rt>& in, const PgoLinks& lin, std::map<int, Rt>& out, std::vector<int>& kept) {
  out.clear(); kept.clear();
  std::multimap<int, int> bi, by_from;   // by_from: from -> link index, in order
  const int n = (int)lin.from.size();
  for (int k = 0; k < n; k++) {
    bi.insert({lin.from[k], lin.to[k]});
    bi.insert({lin.to[k], lin.from[k]});
    by_from.insert({lin.from[k], k});
  }
  auto find = [&](const std::multimap<int, int>& idx, int a, int b) {
    for (auto r = idx.equal_range(a); r.first != r.second; ++r.first)
      if (lin.to[r.first->second] == b) return r.first->second;
    for (auto r = idx.equal_range(b); r.first != r.second; ++r.first)
      if (lin.to[r.first->second] == a) return r.first->second;
    return -1;
  };
  std::multimap<int, int> kept_by_from;
  std::map<int, bool> pending;   // an ordered set
  pending[from_id] = true;
  while (!pending.empty()) {
    const int cur = pending.rbegin()->first;
    pending.erase(cur);
    if (out.empty()) out.insert({cur, in.find(cur)->second});
    for (auto r = bi.equal_range(cur); r.first != r.second; ++r.first) {
      const int to = r.first->second;
      const int k = find(by_from, cur, to);
      if (pending.count(to)) continue;
      if (!out.count(to)) {
        const Rt T = load_rt(&lin.meas[12 * (size_t)k]);
        out.insert({to, lin.from[k] == cur ? compose(out.at(cur), T) : compose(out.at(cur), inverse(T))});
        pending[to] = true;
      }
      if (find(kept_by_from, cur, to) < 0) kept_by_from.insert({lin.from[k], k});
    }
  }
  for (const auto& kv : kept_by_from) kept.push_back(kv.second);   // the out-multimap's order: by from, insertion order among equals
}

}  // namespace sbm

using namespace sbm;

extern "C" {

void sbm_pgo_params_default(sbm_pgo_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->num = 20;
  p->fixed_id = 1;
  p->coupling = SBM_PGO_COUPLING_REFERENCE;
  p->run_max = 64;
}

int sbm_pgo_params_check(const sbm_pgo_params* p, const sbm_pgo_graph* g) { return pgo_check(p, g); }

int sbm_pgo_plan(const sbm_pgo_params* p, const sbm_pgo_graph* g, sbm_pgo_plan_info* info, int32_t* vertex_run, int32_t* slot_rc,
                 uint8_t* edge_couples) {
  if (!info) return SBM_ERR_NULL;
  int st = pgo_check(p, g);
  if (st != SBM_OK) return st;
  PgoPlan P;
  st = pgo_make_plan(p, g, P);
  if (st != SBM_OK && st != SBM_ERR_UNSUPPORTED) return st;
  pgo_plan_info(P, info);
  if (vertex_run) std::copy(P.vrun.begin(), P.vrun.end(), vertex_run);
  if (slot_rc) std::copy(P.slot_rc.begin(), P.slot_rc.end(), slot_rc);
  if (edge_couples) std::copy(P.couples.begin(), P.couples.end(), edge_couples);
  return st;
}

}  // extern "C"
