// sbm_pgo.hpp -- header-only C++ adaptor for the reference's pose-graph optimiser (sbm.h, sbm_pgo_*), so that
//
//     runOptimizeRobust(poses, links, 20, &optimized_poses);                       // src/slam/src/core/main.cpp:328
//
// becomes
//
//     sbm::runOptimizeRobust(handle, poses, links, 20, &optimized_poses);
//
// with the caller's own map types. The functions are templates: PoseMap is a std::map<int, Transform>-like
// container whose mapped type has r11() .. r33(), o14(), o24(), o34() and a constructor from twelve doubles in that row-major
// order; LinkMap is a std::multimap<int, Link>-like container whose mapped type has from(), to(), transform() and infMatrix(),
// the latter with at<double>(row, col) (cv::Mat). The float-to-double conversion of addVertices / addEdges happens here, the
// conversion back in Transform's constructor, as in the reference. Links are taken in the container's iteration order.
// Failures throw sbm::Error. The removed links of the robust loop are available through the optional last argument.
#ifndef SBM_PGO_HPP_
#define SBM_PGO_HPP_

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "sbm_stereobm.hpp"   // sbm::Error

namespace sbm {

namespace pgo_detail {

struct Arrays {
  std::vector<int32_t> ids, from, to;
  std::vector<double> poses, meas, info;
  sbm_pgo_graph graph() const {
    return sbm_pgo_graph{(int32_t)ids.size(), ids.data(), poses.data(), (int32_t)from.size(), from.data(), to.data(), meas.data(),
                         info.data()};
  }
};

template <class Transform> void push_transform(std::vector<double>& v, const Transform& t) {
  const double m[12] = {(double)t.r11(), (double)t.r12(), (double)t.r13(), (double)t.o14(), (double)t.r21(), (double)t.r22(),
                        (double)t.r23(), (double)t.o24(), (double)t.r31(), (double)t.r32(), (double)t.r33(), (double)t.o34()};
  v.insert(v.end(), m, m + 12);
}

template <class PoseMap, class LinkMap> Arrays marshal(const PoseMap& poses, const LinkMap& links) {
  Arrays a;
  for (const auto& p : poses) {
    a.ids.push_back(p.first);
    push_transform(a.poses, p.second);
  }
  for (const auto& l : links) {
    a.from.push_back(l.second.from());
    a.to.push_back(l.second.to());
    push_transform(a.meas, l.second.transform());
    const auto& inf = l.second.infMatrix();
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 6; c++) a.info.push_back(inf.template at<double>(r, c));
  }
  return a;
}

template <class PoseMap> void unmarshal(const int32_t* ids, const double* poses, int n, PoseMap* out) {
  typedef typename PoseMap::mapped_type Transform;
  for (int i = 0; i < n; i++) {
    const double* m = poses + 12 * (size_t)i;
    out->insert(std::make_pair((int)ids[i], Transform(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11])));
  }
}

inline void check(int st) {
  if (st != SBM_OK) throw Error(st, sbm_strerror(st));
}

}  // namespace pgo_detail

// The reference's constants with `num` iterations; change coupling to SBM_PGO_COUPLING_SYMMETRIC for a correct optimiser.
inline sbm_pgo_params pgoParams(int num) {
  sbm_pgo_params p;
  sbm_pgo_params_default(&p);
  p.num = num;
  return p;
}

// runOptimize(poses, links, num, &optimized_poses): returns the final chi2; optimized_poses receives every vertex.
template <class PoseMap, class LinkMap>
double runOptimize(sbm_handle* h, const PoseMap& poses, const LinkMap& links, int num, PoseMap* optimized_poses,
                   const sbm_pgo_params* params = nullptr) {
  sbm_pgo_params p = params ? *params : pgoParams(num);
  p.num = num;
  const pgo_detail::Arrays a = pgo_detail::marshal(poses, links);
  const sbm_pgo_graph g = a.graph();
  std::vector<int32_t> ids(a.ids);
  std::vector<double> out(a.poses.size());
  double err = 0.0;
  pgo_detail::check(sbm_pgo_optimize(h, &p, &g, out.data(), &err));
  std::sort(ids.begin(), ids.end());   // the poses come back in ascending id order
  pgo_detail::unmarshal(ids.data(), out.data(), (int)ids.size(), optimized_poses);
  return err;
}

// runOptimizeRobust(poses, links, num, &optimized_poses): optimized_poses receives the vertices reached from the fixed one;
// removed (may be null) the (from, to) of the links dropped, in order.
template <class PoseMap, class LinkMap>
double runOptimizeRobust(sbm_handle* h, const PoseMap& poses, const LinkMap& links, int num, PoseMap* optimized_poses,
                         const sbm_pgo_params* params = nullptr, std::vector<std::pair<int, int> >* removed = nullptr) {
  sbm_pgo_params p = params ? *params : pgoParams(num);
  p.num = num;
  const pgo_detail::Arrays a = pgo_detail::marshal(poses, links);
  const sbm_pgo_graph g = a.graph();
  std::vector<int32_t> ids(a.ids.size()), rem(2 * a.from.size() + 2);
  std::vector<double> out(a.poses.size());
  int32_t n = 0, nrem = 0;
  double err = 0.0;
  pgo_detail::check(sbm_pgo_optimize_robust(h, &p, &g, &n, ids.data(), out.data(), &err, rem.data(), (int32_t)a.from.size(), &nrem));
  pgo_detail::unmarshal(ids.data(), out.data(), n, optimized_poses);
  if (removed) {
    removed->clear();
    for (int i = 0; i < nrem; i++) removed->push_back(std::make_pair((int)rem[2 * i], (int)rem[2 * i + 1]));
  }
  return err;
}

}  // namespace sbm

#endif  // SBM_PGO_HPP_
