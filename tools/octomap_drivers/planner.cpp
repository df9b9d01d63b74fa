// Driver of tools/make_occupancy_planner_fixtures.py: trees from recorded scans or key lists, then octomap's read side for planners --
// begin_leafs_bbx by keys and by points, getUnknownLeafCenters, getMetricMin / getMetricMax / volume, getRayIntersection -- and
// octomap's own time for the calls tools/bench_occupancy_planner.py times. This project's text; it calls octomap's API only.
//
// in:   int32 ntrees, per tree: head, int32 hits, int32 max_likelihood, hits | scans,
//         int32 nb, nb x {uint16 min[3], max[3], int32 max_depth}; int32 np, np x {float min[3], max[3], int32 max_depth};
//         int32 nu, nu x {float pmin[3], pmax[3], int32 depth}
//       double resolution, int32 nrays, nrays x {float origin[3], direction[3], centre[3], double delta}
//       int32 timing; if set: head, scans, uint16 min[3], max[3], float pmin[3], pmax[3], int32 repeat (of the rays above)
// out:  per tree: 12 doubles of the expanded tree (const min, max; calcMinMax min, max), 12 of the pruned one, double volume;
//         per box: leaves; per unknown case: uint32 n, float xyz[3 n]
//       per ray: int32 found, float xyz[3] (NaN where not found: `intersection` is set to NaN before each call)
//       timing: uint64 counts and double ms, in the order of main()
#include "driver.h"
#include <cmath>
#include <limits>

static void metric_out(octomap::OcTree& tree, FILE* out) {
  const octomap::OcTree& ct = tree;   // the const forms walk the leaves as long as calcMinMax has not run: they go first
  double v[12];
  ct.getMetricMin(v[0], v[1], v[2]);
  ct.getMetricMax(v[3], v[4], v[5]);
  tree.getMetricMin(v[6], v[7], v[8]);
  tree.getMetricMax(v[9], v[10], v[11]);
  fwrite(v, 8, 12, out);
}

template <class It> static void iter_out(It it, It end, FILE* out) {
  std::vector<uint16_t> k;
  std::vector<float> v;
  for (; it != end; ++it) {
    octomap::OcTreeKey key = it.getKey();
    k.push_back(key[0]), k.push_back(key[1]), k.push_back(key[2]), k.push_back((uint16_t)it.getDepth());
    v.push_back(it->getLogOdds());
  }
  wr(out, (uint32_t)v.size());
  for (size_t i = 0; i < v.size(); i++) {
    fwrite(&k[4 * i], 2, 4, out);
    wr(out, v[i]);
  }
}

struct Ray {
  float o[3], d[3], c[3];
  double delta;
};

int main(int argc, char** argv) {
  FILE *in, *out;
  if (!open_files(argc, argv, in, out)) return 2;
  int32_t ntrees;
  if (!rd(in, &ntrees, 1)) return 3;
  for (int t = 0; t < ntrees; t++) {
    double prob[5], resolution;
    int32_t hits, ml, n;
    if (!head_in(in, prob, &resolution) || !rd(in, &hits, 1) || !rd(in, &ml, 1)) return 3;
    octomap::OcTree tree(resolution);
    set_params(tree, prob);
    if (!(hits ? hits_in(in, tree) : scans_in(in, tree))) return 3;
    if (ml) tree.toMaxLikelihood();
    else tree.updateInnerOccupancy();
    {
      octomap::OcTree copy(tree);
      copy.expand();
      metric_out(copy, out);
    }
    tree.prune();
    metric_out(tree, out);
    wr(out, (double)tree.volume());
    if (!rd(in, &n, 1)) return 3;
    for (int i = 0; i < n; i++) {
      uint16_t k[6];
      int32_t depth;
      if (!rd(in, k, 6) || !rd(in, &depth, 1)) return 3;
      iter_out(tree.begin_leafs_bbx(octomap::OcTreeKey(k[0], k[1], k[2]), octomap::OcTreeKey(k[3], k[4], k[5]), (unsigned char)depth),
               tree.end_leafs_bbx(), out);
    }
    if (!rd(in, &n, 1)) return 3;
    for (int i = 0; i < n; i++) {
      float p[6];
      int32_t depth;
      if (!rd(in, p, 6) || !rd(in, &depth, 1)) return 3;
      iter_out(tree.begin_leafs_bbx(octomap::point3d(p[0], p[1], p[2]), octomap::point3d(p[3], p[4], p[5]), (unsigned char)depth),
               tree.end_leafs_bbx(), out);
    }
    if (!rd(in, &n, 1)) return 3;
    for (int i = 0; i < n; i++) {
      float p[6];
      int32_t depth;
      if (!rd(in, p, 6) || !rd(in, &depth, 1)) return 3;
      octomap::point3d_list centres;
      tree.getUnknownLeafCenters(centres, octomap::point3d(p[0], p[1], p[2]), octomap::point3d(p[3], p[4], p[5]), (unsigned)depth);
      wr(out, (uint32_t)centres.size());
      for (octomap::point3d_list::iterator it = centres.begin(); it != centres.end(); ++it) {
        float xyz[3] = {it->x(), it->y(), it->z()};
        fwrite(xyz, 4, 3, out);
      }
    }
  }
  double resolution;
  int32_t nrays;
  if (!rd(in, &resolution, 1) || !rd(in, &nrays, 1)) return 3;
  std::vector<Ray> rays(nrays);
  octomap::OcTree plain(resolution);
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (int i = 0; i < nrays; i++) {
    Ray& r = rays[i];
    if (!rd(in, r.o, 3) || !rd(in, r.d, 3) || !rd(in, r.c, 3) || !rd(in, &r.delta, 1)) return 3;
    octomap::point3d hit(nan, nan, nan);
    bool found = plain.getRayIntersection(octomap::point3d(r.o[0], r.o[1], r.o[2]), octomap::point3d(r.d[0], r.d[1], r.d[2]),
                                          octomap::point3d(r.c[0], r.c[1], r.c[2]), hit, r.delta);
    float xyz[3] = {hit.x(), hit.y(), hit.z()};
    wr(out, (int32_t)(found ? 1 : 0));
    fwrite(xyz, 4, 3, out);
  }
  int32_t timing;
  if (!rd(in, &timing, 1)) return 3;
  if (timing) {
    double prob[5];
    uint16_t k[6];
    float p[6];
    int32_t repeat;
    if (!head_in(in, prob, &resolution)) return 3;
    octomap::OcTree tree(resolution);
    set_params(tree, prob);
    if (!scans_in(in, tree) || !rd(in, k, 6) || !rd(in, p, 6) || !rd(in, &repeat, 1)) return 3;
    tree.updateInnerOccupancy();
    tree.prune();
    uint64_t count = 0;
    Clock::time_point t0 = Clock::now();
    for (octomap::OcTree::leaf_iterator it = tree.begin_leafs(), end = tree.end_leafs(); it != end; ++it) count++;
    double ms = ms_since(t0);
    wr(out, count);
    wr(out, ms);
    count = 0;
    t0 = Clock::now();
    for (octomap::OcTree::leaf_bbx_iterator it = tree.begin_leafs_bbx(octomap::OcTreeKey(k[0], k[1], k[2]), octomap::OcTreeKey(k[3], k[4], k[5])),
                                            end = tree.end_leafs_bbx(); it != end; ++it) count++;
    ms = ms_since(t0);
    wr(out, count);
    wr(out, ms);
    const unsigned depths[2] = {16, 14};
    for (unsigned depth : depths) {
      octomap::point3d_list centres;
      t0 = Clock::now();
      tree.getUnknownLeafCenters(centres, octomap::point3d(p[0], p[1], p[2]), octomap::point3d(p[3], p[4], p[5]), depth);
      ms = ms_since(t0);
      wr(out, (uint64_t)centres.size());
      wr(out, ms);
    }
    double v[6];
    const octomap::OcTree& ct = tree;
    t0 = Clock::now();
    ct.getMetricMin(v[0], v[1], v[2]);
    ct.getMetricMax(v[3], v[4], v[5]);
    ms = ms_since(t0);
    wr(out, (uint64_t)tree.getNumLeafNodes());
    wr(out, ms);
    count = 0;
    t0 = Clock::now();
    for (int r = 0; r < repeat; r++)
      for (int i = 0; i < nrays; i++) {
        const Ray& ray = rays[i];
        octomap::point3d hit;
        count += tree.getRayIntersection(octomap::point3d(ray.o[0], ray.o[1], ray.o[2]), octomap::point3d(ray.d[0], ray.d[1], ray.d[2]),
                                         octomap::point3d(ray.c[0], ray.c[1], ray.c[2]), hit, ray.delta) ? 1 : 0;
      }
    ms = ms_since(t0);
    wr(out, (uint64_t)repeat * (uint64_t)nrays);
    wr(out, ms);
    wr(out, count);
  }
  fclose(out);
  return 0;
}
