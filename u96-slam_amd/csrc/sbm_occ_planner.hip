// sbm_occ_planner.hip -- the occupancy map's read side for planners (include/sbm.h, "occupancy map: the read side for planners"):
// octomap's begin_leafs_bbx, getUnknownLeafCenters, getMetricMin / getMetricMax and getRayIntersection.  gfx950. Nothing here
// contracts a multiply-add. The first three read an sbm_occ_tree snapshot, the fourth needs the map's resolution only; all are
// read-only. Nothing waits on another workgroup: every step is a launch of its own, and the only atomics are integer counts and
// integer minima / maxima, one per wavefront.
//   occ_plan_bbx          occ_tree_select_kernel with singleIncrement's overlap test of the node itself, as a count pass (the
//                         host cannot know the count) and as the selection that the tree's sort and gather follow
//   occ_plan_unknown_*    one lane per cell of the step grid does search(p, depth) at the running float sums of the three axes;
//                         counts per tile of kOccTile cells, their scan, and the write in linear cell order
//   occ_plan_metric       the smallest and largest centre key per axis among the leaves of one depth
//   occ_plan_ray_entry    one lane per ray, the six planes in the order of the source
#include "sbm_occ.h"

namespace sbm {
#pragma clang fp contract(off)

struct OccKeyBox { unsigned lo[3], hi[3]; };

// adjustKeyAtDepth of a node's Morton prefix: the centre key per axis
__device__ __forceinline__ void occ_plan_centre(unsigned long long code, int depth, unsigned k[3]) {
  const int level = kOccDepth - depth;
  for (int a = 0; a < 3; a++) k[a] = level ? (occ_unspread(code >> a) << level) | (1u << (level - 1)) : occ_unspread(code >> a);
}
// a node of the pruned tree that begin_leafs(max_depth) stops at
__device__ __forceinline__ bool occ_plan_stop(unsigned info, int depth, int max_depth) {
  const unsigned top = (info >> kOccTopShift) & 31u;
  const bool pruned = top != kOccNoTop && top < (unsigned)depth;
  return !pruned && (depth == kOccDepth || (info & kOccCollapsed) || depth == max_depth);
}

// OcTreeIterator.hxx:445-447 for the node itself, in int as the source's promoted key_type sums are. A node's tested interval
// [c - off, c + off] lies inside its parent's, so a box that passes here passed at every ancestor: no lane needs another's answer.
// The root is never tested.
template <bool kCount>
__global__ void __launch_bounds__(256) occ_plan_bbx_kernel(OccLevel l, int depth, int max_depth, unsigned tag, uint32_t cap, OccKeyBox box,
                                                            unsigned long long* __restrict__ out_code, unsigned* __restrict__ out_at,
                                                            OccTreeStats* __restrict__ st) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool take = false;
  if (i < l.n && occ_plan_stop(l.info[i], depth, max_depth)) {
    take = true;
    if (depth) {
      unsigned c[3];
      occ_plan_centre(l.code[i], depth, c);
      const int off = 32768 >> depth;
      for (int a = 0; a < 3; a++) take = take && (int)box.lo[a] <= (int)c[a] + off && (int)box.hi[a] >= (int)c[a] - off;
    }
  }
  const uint32_t o = occ_wave_append(take, &st->cursor);   // every lane is here
  if (kCount || !take || o >= cap) return;
  out_code[o] = l.code[i] << (3 * (kOccDepth - depth));
  out_at[o] = tag + i;
}

struct OccUnknownGrid {
  const float *x, *y, *z;   // the running sums of the three axes
  uint32_t ny, nz, cells;
  int depth;
  double factor;
  OccLevel l;               // the asked depth
};
// cell i in push order (x outermost, z innermost): is search(p, depth) NULL there -- a point without a key, or no node
__device__ __forceinline__ bool occ_plan_unknown_cell(const OccUnknownGrid& g, uint32_t i, float p[3]) {
  const uint32_t iz = i % g.nz, iy = (i / g.nz) % g.ny, ix = i / g.nz / g.ny;
  p[0] = g.x[ix], p[1] = g.y[iy], p[2] = g.z[iz];
  unsigned k0, k1, k2;
  if (!(occ_axis(g.factor, p[0], &k0) && occ_axis(g.factor, p[1], &k1) && occ_axis(g.factor, p[2], &k2))) return true;
  const unsigned long long code = occ_code(k0, k1, k2) >> (3 * (kOccDepth - g.depth));
  uint32_t lo = 0, hi = g.l.n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (g.l.code[mid] < code) lo = mid + 1;
    else hi = mid;
  }
  return !(lo < g.l.n && g.l.code[lo] == code);
}

__global__ void __launch_bounds__(256) occ_plan_unknown_count_kernel(OccUnknownGrid g, unsigned* __restrict__ tile_count) {
  __shared__ unsigned wsum[4];
  float p[3];
  unsigned c = 0;
  for (int r = 0; r < kOccTile / 256; r++) {
    const uint32_t i = blockIdx.x * kOccTile + r * 256 + threadIdx.x;
    c += (i < g.cells && occ_plan_unknown_cell(g, i, p)) ? 1u : 0u;
  }
  for (int o = 32; o; o >>= 1) c += (unsigned)__shfl_xor((int)c, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive scan of the tile counts in place and their sum in v[tiles]; one workgroup, a run of tiles per thread
__global__ void __launch_bounds__(256) occ_plan_scan_kernel(unsigned* __restrict__ v, uint32_t tiles) {
  __shared__ unsigned part[256];
  const uint32_t per = (tiles + 255) / 256;
  const uint32_t lo = min(threadIdx.x * per, tiles), hi = min(lo + per, tiles);
  unsigned sum = 0;
  for (uint32_t t = lo; t < hi; t++) sum += v[t];
  part[threadIdx.x] = sum;
  __syncthreads();
  unsigned before = 0;
  for (int d = 0; d < (int)threadIdx.x; d++) before += part[d];
  for (uint32_t t = lo; t < hi; t++) {
    const unsigned x = v[t];
    v[t] = before;
    before += x;
  }
  if (threadIdx.x == 255) v[tiles] = before;   // the last thread's run ends at the last tile (or is empty behind it)
}

__global__ void __launch_bounds__(256) occ_plan_unknown_write_kernel(OccUnknownGrid g, const unsigned* __restrict__ tile_off, uint32_t cap,
                                                                      float* __restrict__ out) {
  __shared__ unsigned wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned running = tile_off[blockIdx.x];
  for (int r = 0; r < kOccTile / 256; r++) {   // the same trips for every thread: the barriers below are reached by all
    const uint32_t i = blockIdx.x * kOccTile + r * 256 + threadIdx.x;
    float p[3];
    const bool take = i < g.cells && occ_plan_unknown_cell(g, i, p);
    const unsigned long long taking = __ballot(take);
    if (lane == 0) wsum[wave] = __popcll(taking);
    __syncthreads();
    unsigned before = running;
    for (int w = 0; w < wave; w++) before += wsum[w];
    running += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    const uint32_t at = before + __popcll(taking & ((1ull << lane) - 1));
    if (!take || at >= cap) continue;
    out[3 * (size_t)at] = p[0];
    out[3 * (size_t)at + 1] = p[1];
    out[3 * (size_t)at + 2] = p[2];
  }
}

// out: min x y z (from ~0), max x y z (from 0) of the centre keys of this depth's leaves
__global__ void __launch_bounds__(256) occ_plan_metric_kernel(OccLevel l, int depth, unsigned* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  unsigned lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
  if (i < l.n && occ_plan_stop(l.info[i], depth, kOccDepth)) {
    unsigned c[3];
    occ_plan_centre(l.code[i], depth, c);
    for (int a = 0; a < 3; a++) lo[a] = hi[a] = c[a];
  }
  for (int a = 0; a < 3; a++) {   // every lane of the wavefront is here
    lo[a] = occ_wave_min(lo[a]);
    hi[a] = occ_wave_max(hi[a]);
  }
  if ((threadIdx.x & 63) == 0 && lo[0] != ~0u)
    for (int a = 0; a < 3; a++) {
      atomicMin(&out[a], lo[a]);
      atomicMax(&out[3 + a], hi[a]);
    }
}

// Vector3::dot: the products and sums in float, left to right, returned as double
__device__ __forceinline__ double occ_plan_dot(const float a[3], const float b[3]) {
#pragma clang fp contract(off)
  return (double)(a[0] * b[0] + a[1] * b[1] + a[2] * b[2]);
}

// getRayIntersection, OccupancyOcTreeBase.hxx:768-853, in the order of the source -> found, *hit (NaN where not)
__device__ __forceinline__ int occ_plan_ray(const float o[3], const float dir[3], const float c[3], double resolution, double delta,
                                            float hit[3]) {
#pragma clang fp contract(off)
  const float half = (float)(resolution / 2.0);
  const float neg[3] = {c[0] - half, c[1] - half, c[2] - half}, pos[3] = {c[0] + half, c[1] + half, c[2] + half};
  double out_d = 1.7976931348623157e308;   // std::numeric_limits<double>::max()
  bool found = false;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float normal[3] = {a == 0 ? 1.0f : 0.0f, a == 1 ? 1.0f : 0.0f, a == 2 ? 1.0f : 0.0f};
    const double line_dot_normal = occ_plan_dot(normal, dir);
    if (line_dot_normal != 0.0) {   // a NaN passes, as in the source
      const int u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2;
#pragma unroll
      for (int s = 0; s < 2; s++) {
        float point[3] = {c[0], c[1], c[2]};
        point[a] = s ? pos[a] : neg[a];
        const float diff[3] = {point[0] - o[0], point[1] - o[1], point[2] - o[2]};
        const double d = occ_plan_dot(diff, normal) / line_dot_normal;
        const float fd = (float)d;
        const float at[3] = {dir[0] * fd + o[0], dir[1] * fd + o[1], dir[2] * fd + o[2]};
        if (!((double)at[u] < (double)neg[u] - 1e-6 || (double)at[u] > (double)pos[u] + 1e-6 || (double)at[v] < (double)neg[v] - 1e-6 ||
              (double)at[v] > (double)pos[v] + 1e-6)) {
          out_d = d < out_d ? d : out_d;   // std::min(outD, d)
          found = true;
        }
      }
    }
  }
  const float t = (float)(out_d + delta);
  for (int a = 0; a < 3; a++) hit[a] = found ? dir[a] * t + o[a] : __uint_as_float(0x7FC00000u);
  return found ? 1 : 0;
}

struct OccRayOrigin { int shared; float origin[3]; };

__global__ void __launch_bounds__(256) occ_plan_ray_entry_kernel(const float* __restrict__ origins, const float* __restrict__ dirs,
                                                                  const float* __restrict__ centres, size_t n, OccRayOrigin ro, double resolution,
                                                                  double delta, float* __restrict__ xyz, int* __restrict__ found) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float o[3], hit[3];
  for (int a = 0; a < 3; a++) o[a] = ro.shared ? ro.origin[a] : origins[3 * i + a];
  const float d[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]}, c[3] = {centres[3 * i], centres[3 * i + 1], centres[3 * i + 2]};
  const int f = occ_plan_ray(o, d, c, resolution, delta, hit);
  for (int a = 0; a < 3; a++) xyz[3 * i + a] = hit[a];
  if (found) found[i] = f;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static bool occ_plan_empty(const sbm_occ_tree* t) { return !t->built || !t->count[kOccDepth]; }

template <bool kCount>
static int occ_plan_bbx_launch(sbm_occ_tree* t, const OccKeyBox& box, int max_depth, uint32_t cap, unsigned long long* keys, unsigned* at) {
  sbm_handle* h = t->h;
  OccTreeStats* stats = t->stats.as<OccTreeStats>();
  for (int d = 0; d <= max_depth; d++) {
    const OccLevel l = occ_tree_level(t, d);
    const unsigned tag = d == kOccDepth ? 0u : kOccInnerTag | (unsigned)t->off[d];
    hipLaunchKernelGGL(occ_plan_bbx_kernel<kCount>, dim3((l.n + 255) / 256), dim3(256), 0, h->stream, l, d, max_depth, tag, cap, box, keys, at, stats);
    HIPCHK(h, hipGetLastError());
  }
  return SBM_OK;
}

// How many entries the box iterator visits: the count pass and one read of the cursor. Waits for the stream.
static int occ_plan_bbx_count(sbm_occ_tree* t, const OccKeyBox& box, int max_depth, size_t* count) {
  sbm_handle* h = t->h;
  *count = 0;
  if (occ_plan_empty(t)) return SBM_OK;
  unsigned total = 0;
  const int st = occ_timed_run(h, kOccTreeQuery, true, 0, [&]() -> int {
    OccTreeStats* stats = t->stats.as<OccTreeStats>();
    HIPCHK(h, hipMemsetAsync(&stats->cursor, 0, sizeof(unsigned), h->stream));
    const int st = occ_plan_bbx_launch<true>(t, box, max_depth, 0, nullptr, nullptr);
    if (st != SBM_OK) return st;
    HIPCHK(h, hipMemcpyAsync(&total, &stats->cursor, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBM_OK;
  });
  *count = total;
  return st;
}

// The n entries a count pass found, into device arrays of n. Synchronous.
static int occ_plan_bbx_fill(sbm_occ_tree* t, const OccKeyBox& box, int max_depth, uint32_t n, unsigned long long* d_keys, int* d_depth,
                             unsigned* d_value) {
  return occ_timed_run(t->h, kOccTreeQuery, n > 0, 1, [&]() -> int {
    OccSelection s;
    int st = occ_tree_select_begin(t, n, d_keys, d_depth, &s);
    if (st != SBM_OK) return st;
    st = occ_plan_bbx_launch<false>(t, box, max_depth, n, s.kk[0], s.vv[0]);
    return st != SBM_OK ? st : occ_tree_select_end(t, s, d_value);
  });
}

static int occ_plan_bbx_check(const sbm_occ_tree* tree, const void* lo, const void* hi, int max_depth, const void* keys, const void* depth,
                              const void* value, size_t cap, const size_t* count, bool device) {
  if (!tree || !lo || !hi || !count || (cap > 0 && (!keys || !depth))) return SBM_ERR_NULL;
  if (max_depth < 0 || max_depth > kOccDepth) return SBM_ERR_SIZE;
  if (device && (((uintptr_t)keys & 7) || ((uintptr_t)depth & 3) || ((uintptr_t)value & 3))) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

static int occ_plan_bbx_device(sbm_occ_tree* tree, const OccKeyBox& box, int max_depth, void* d_keys, void* d_depth, void* d_value, size_t cap,
                               size_t* count) {
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  max_depth = max_depth ? max_depth : kOccDepth;
  const int st = occ_plan_bbx_count(tree, box, max_depth, count);
  if (st != SBM_OK) return st;
  if (*count > cap) return SBM_ERR_SIZE;
  return occ_plan_bbx_fill(tree, box, max_depth, (uint32_t)*count, (unsigned long long*)d_keys, (int*)d_depth, (unsigned*)d_value);
}

static int occ_plan_bbx_host(sbm_occ_tree* tree, const OccKeyBox& box, int max_depth, uint64_t* keys, int32_t* depth, float* value, size_t cap,
                             size_t* count) {
  sbm_handle* h = tree->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  max_depth = max_depth ? max_depth : kOccDepth;
  int st = occ_plan_bbx_count(tree, box, max_depth, count);
  if (st != SBM_OK) return st;
  const size_t n = *count;
  if (n > cap) return SBM_ERR_SIZE;
  if (!n) return SBM_OK;
  struct { unsigned long long* keys; int* depth; unsigned* value; } io;
  HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& c) { io = {c.take<unsigned long long>(n), c.take<int>(n), c.take<unsigned>(n)}; }, occ_pad));
  st = occ_plan_bbx_fill(tree, box, max_depth, (uint32_t)n, io.keys, io.depth, io.value);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpyAsync(keys, io.keys, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(depth, io.depth, n * 4, hipMemcpyDeviceToHost, h->stream));
  if (value) HIPCHK(h, hipMemcpyAsync(value, io.value, n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

static OccKeyBox occ_plan_key_box(const uint16_t lo[3], const uint16_t hi[3]) {
  OccKeyBox b;
  for (int a = 0; a < 3; a++) b.lo[a] = lo[a], b.hi[a] = hi[a];
  return b;
}
// coordToKeyChecked on both corners; false: the end iterator
static bool occ_plan_point_box(const sbm_occ_tree* t, const float lo[3], const float hi[3], OccKeyBox* b) {
  const double factor = 1. / t->resolution;
  for (int a = 0; a < 3; a++)
    if (!occ_axis_host(factor, lo[a], &b->lo[a]) || !occ_axis_host(factor, hi[a], &b->hi[a])) return false;
  return true;
}

// The unknown cells of a planned grid into d_xyz (cap triples). *count is the number found; beyond cap nothing is written.
static int occ_plan_unknown_run(sbm_occ_tree* t, const OccUnknownPlan& p, int depth, float* d_xyz, size_t cap, size_t* count) {
  sbm_handle* h = t->h;
  *count = 0;
  const size_t cells = (size_t)p.steps[0] * p.steps[1] * p.steps[2];
  if (!cells) return SBM_OK;
  std::vector<float> table;
  try {
    table.resize((size_t)p.steps[0] + p.steps[1] + p.steps[2]);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  float* axis[3] = {table.data(), table.data() + p.steps[0], table.data() + p.steps[0] + p.steps[1]};
  for (int a = 0; a < 3; a++) occ_unknown_axis(p.lo[a], p.step, p.steps[a], axis[a]);
  const uint32_t tiles = (uint32_t)((cells + kOccTile - 1) / kOccTile);
  struct { float* table; unsigned* tile; } d;
  HIPCHK(h, carve(h->occ.hist, h->stream, [&](Carve& c) { d = {c.take<float>(table.size()), c.take<unsigned>((size_t)tiles + 1)}; }, occ_pad));
  OccUnknownGrid g;
  memset(&g, 0, sizeof(g));
  g.x = d.table, g.y = d.table + p.steps[0], g.z = d.table + p.steps[0] + p.steps[1];
  g.ny = p.steps[1], g.nz = p.steps[2], g.cells = (uint32_t)cells;
  g.depth = depth;
  g.factor = 1. / t->resolution;
  g.l = occ_tree_level(t, depth);
  unsigned total = 0;
  int st = occ_timed_run(h, kOccTreeQuery, true, 0, [&]() -> int {
    HIPCHK(h, hipMemcpyAsync(d.table, table.data(), table.size() * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(occ_plan_unknown_count_kernel, dim3(tiles), dim3(256), 0, h->stream, g, d.tile);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(occ_plan_scan_kernel, dim3(1), dim3(256), 0, h->stream, d.tile, tiles);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(&total, d.tile + tiles, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the table has left the host vector as well
    return SBM_OK;
  });
  if (st != SBM_OK) return st;
  *count = total;
  if (total > cap) return SBM_ERR_SIZE;
  return occ_timed_run(h, kOccTreeQuery, total > 0, 1, [&]() -> int {
    hipLaunchKernelGGL(occ_plan_unknown_write_kernel, dim3(tiles), dim3(256), 0, h->stream, g, d.tile, (uint32_t)total, d_xyz);
    return SBM_OK;
  });
}

static int occ_plan_unknown_check(const sbm_occ_tree* tree, const float* pmin, const float* pmax, int depth, const void* xyz, size_t cap,
                                  const size_t* count, bool device, OccUnknownPlan* p) {
  if (!tree || !pmin || !pmax || !count || (cap > 0 && !xyz)) return SBM_ERR_NULL;
  if (depth < 0 || depth > kOccDepth) return SBM_ERR_SIZE;
  const int st = occ_unknown_plan(tree->resolution, pmin, pmax, depth, p);
  if (st == SBM_ERR_SIZE) return st;                       // a corner outside the key space
  if (device && ((uintptr_t)xyz & 3)) return SBM_ERR_UNSUPPORTED;
  return st;                                               // more than 2^30 cells
}

static int occ_plan_metric_run(sbm_occ_tree* t) {
  sbm_handle* h = t->h;
  if (t->have_metric) return SBM_OK;
  int st = occ_tree_stats(t);
  if (st != SBM_OK) return st;
  for (int a = 0; a < 6; a++) t->metric[a] = 0.0;          // an empty tree: six zeros, as octomap answers
  if (!occ_plan_empty(t)) {
    unsigned* d_keys;
    const size_t words = (size_t)(kOccDepth + 1) * 6;
    HIPCHK(h, carve(h->occ.hist, h->stream, [&](Carve& c) { d_keys = c.take<unsigned>(words); }, occ_pad));
    unsigned keys[(kOccDepth + 1) * 6];
    for (int d = 0; d <= kOccDepth; d++)
      for (int a = 0; a < 6; a++) keys[6 * d + a] = a < 3 ? ~0u : 0u;
    st = occ_timed_run(h, kOccTreeQuery, true, 0, [&]() -> int {
      HIPCHK(h, hipMemcpyAsync(d_keys, keys, sizeof(keys), hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));          // `keys` is read back into below
      for (int d = 0; d <= kOccDepth; d++) {
        if (!t->host.leaves_at[d]) continue;
        const OccLevel l = occ_tree_level(t, d);
        hipLaunchKernelGGL(occ_plan_metric_kernel, dim3((l.n + 255) / 256), dim3(256), 0, h->stream, l, d, d_keys + 6 * d);
        HIPCHK(h, hipGetLastError());
      }
      HIPCHK(h, hipMemcpyAsync(keys, d_keys, sizeof(keys), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      return SBM_OK;
    });
    if (st != SBM_OK) return st;
    double lo[3], hi[3];
    for (int a = 0; a < 3; a++) lo[a] = 1.7976931348623157e308, hi[a] = -1.7976931348623157e308;
    for (int d = 0; d <= kOccDepth; d++)
      if (t->host.leaves_at[d]) occ_metric_fold(d, keys + 6 * d, keys + 6 * d + 3, t->resolution, lo, hi);
    for (int a = 0; a < 3; a++) t->metric[a] = lo[a], t->metric[3 + a] = hi[a];
  }
  t->have_metric = true;
  return SBM_OK;
}

static int occ_plan_rays_run(sbm_occ_map* map, size_t n, const float* d_origins, const float* origin, const float* d_dirs, const float* d_centres,
                             double delta, float* d_xyz, int* d_found, int sync) {
  OccRayOrigin ro;
  memset(&ro, 0, sizeof(ro));
  ro.shared = origin != nullptr;
  if (origin) memcpy(ro.origin, origin, sizeof(ro.origin));
  return occ_timed_run(map->h, kOccCast, n > 0, sync, [&]() -> int {
    hipLaunchKernelGGL(occ_plan_ray_entry_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, map->h->stream, d_origins, d_dirs, d_centres, n,
                       ro, map->p.resolution, delta, d_xyz, d_found);
    return SBM_OK;
  });
}

static int occ_plan_rays_check(const sbm_occ_map* map, size_t n, const void* origins, const void* dirs, const void* centres, double delta,
                               const void* xyz) {
  if (!map || (n > 0 && (!origins || !dirs || !centres || !xyz))) return SBM_ERR_NULL;
  if (std::isnan(delta)) return SBM_ERR_SIZE;
  if (n > ((size_t)1 << 30)) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

}  // namespace sbm
using namespace sbm;

extern "C" {
int sbm_occ_bbx_leaves_device(sbm_occ_tree* tree, const uint16_t min_key[3], const uint16_t max_key[3], int max_depth, void* d_keys,
                              void* d_depth, void* d_value, size_t cap, size_t* count) {
  const int st = occ_plan_bbx_check(tree, min_key, max_key, max_depth, d_keys, d_depth, d_value, cap, count, true);
  if (st != SBM_OK) return st;
  return occ_plan_bbx_device(tree, occ_plan_key_box(min_key, max_key), max_depth, d_keys, d_depth, d_value, cap, count);
}

int sbm_occ_bbx_leaves(sbm_occ_tree* tree, const uint16_t min_key[3], const uint16_t max_key[3], int max_depth, uint64_t* keys,
                       int32_t* depth, float* value, size_t cap, size_t* count) {
  const int st = occ_plan_bbx_check(tree, min_key, max_key, max_depth, keys, depth, value, cap, count, false);
  if (st != SBM_OK) return st;
  return occ_plan_bbx_host(tree, occ_plan_key_box(min_key, max_key), max_depth, keys, depth, value, cap, count);
}

int sbm_occ_bbx_leaves_points_device(sbm_occ_tree* tree, const float min[3], const float max[3], int max_depth, void* d_keys, void* d_depth,
                                     void* d_value, size_t cap, size_t* count) {
  const int st = occ_plan_bbx_check(tree, min, max, max_depth, d_keys, d_depth, d_value, cap, count, true);
  if (st != SBM_OK) return st;
  OccKeyBox box;
  *count = 0;
  if (!occ_plan_point_box(tree, min, max, &box)) return SBM_OK;
  return occ_plan_bbx_device(tree, box, max_depth, d_keys, d_depth, d_value, cap, count);
}

int sbm_occ_bbx_leaves_points(sbm_occ_tree* tree, const float min[3], const float max[3], int max_depth, uint64_t* keys, int32_t* depth,
                              float* value, size_t cap, size_t* count) {
  const int st = occ_plan_bbx_check(tree, min, max, max_depth, keys, depth, value, cap, count, false);
  if (st != SBM_OK) return st;
  OccKeyBox box;
  *count = 0;
  if (!occ_plan_point_box(tree, min, max, &box)) return SBM_OK;
  return occ_plan_bbx_host(tree, box, max_depth, keys, depth, value, cap, count);
}

int sbm_occ_unknown_device(sbm_occ_tree* tree, const float pmin[3], const float pmax[3], int depth, void* d_xyz, size_t cap, size_t* count) {
  OccUnknownPlan p;
  const int st = occ_plan_unknown_check(tree, pmin, pmax, depth, d_xyz, cap, count, true, &p);
  if (st != SBM_OK) return st;
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  return occ_plan_unknown_run(tree, p, depth ? depth : kOccDepth, (float*)d_xyz, cap, count);
}

int sbm_occ_unknown(sbm_occ_tree* tree, const float pmin[3], const float pmax[3], int depth, float* xyz, size_t cap, size_t* count) {
  OccUnknownPlan p;
  int st = occ_plan_unknown_check(tree, pmin, pmax, depth, xyz, cap, count, false, &p);
  if (st != SBM_OK) return st;
  sbm_handle* h = tree->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  const size_t cells = (size_t)p.steps[0] * p.steps[1] * p.steps[2], room = cap < cells ? cap : cells;
  if (room) HIPCHK(h, h->occ.io.grow(room * 12, h->stream));
  st = occ_plan_unknown_run(tree, p, depth ? depth : kOccDepth, h->occ.io.as<float>(), room, count);
  if (st != SBM_OK) return st;
  if (*count) {
    HIPCHK(h, hipMemcpyAsync(xyz, h->occ.io.p, *count * 12, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return SBM_OK;
}

int sbm_occ_metric(sbm_occ_tree* tree, double min[3], double max[3]) {
  if (!tree || !min || !max) return SBM_ERR_NULL;
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  const int st = occ_plan_metric_run(tree);
  if (st != SBM_OK) return st;
  for (int a = 0; a < 3; a++) min[a] = tree->metric[a], max[a] = tree->metric[3 + a];
  return SBM_OK;
}

int sbm_occ_ray_intersections_device(sbm_occ_map* map, size_t n, const void* origins, int shared_origin, const void* d_dirs,
                                     const void* d_centres, double delta, void* d_xyz, void* d_found, int sync) {
  const int st = occ_plan_rays_check(map, n, origins, d_dirs, d_centres, delta, d_xyz);
  if (st != SBM_OK) return st;
  if ((!shared_origin && ((uintptr_t)origins & 3)) || ((uintptr_t)d_dirs & 3) || ((uintptr_t)d_centres & 3) || ((uintptr_t)d_xyz & 3) ||
      ((uintptr_t)d_found & 3))
    return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_plan_rays_run(map, n, shared_origin ? nullptr : (const float*)origins, shared_origin ? (const float*)origins : nullptr,
                           (const float*)d_dirs, (const float*)d_centres, delta, (float*)d_xyz, (int*)d_found, sync);
}

int sbm_occ_ray_intersections(sbm_occ_map* map, size_t n, const float* origins, int shared_origin, const float* dirs, const float* centres,
                              double delta, float* xyz, int32_t* found) {
  int st = occ_plan_rays_check(map, n, origins, dirs, centres, delta, xyz);
  if (st != SBM_OK) return st;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  struct { float *origins, *dirs, *centres, *xyz; int* found; } io = {};
  if (n) {
    HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& c) {
      io = {c.take<float>(shared_origin ? 0 : n * 3), c.take<float>(n * 3), c.take<float>(n * 3), c.take<float>(n * 3), c.take<int>(n)};
    }, occ_pad));
    HIPCHK(h, hipMemcpyAsync(io.dirs, dirs, n * 12, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(io.centres, centres, n * 12, hipMemcpyHostToDevice, h->stream));
    if (!shared_origin) HIPCHK(h, hipMemcpyAsync(io.origins, origins, n * 12, hipMemcpyHostToDevice, h->stream));
  }
  st = occ_plan_rays_run(map, n, shared_origin ? nullptr : io.origins, shared_origin ? origins : nullptr, io.dirs, io.centres, delta, io.xyz,
                         io.found, 0);
  if (st != SBM_OK) return st;
  if (n) {
    HIPCHK(h, hipMemcpyAsync(xyz, io.xyz, n * 12, hipMemcpyDeviceToHost, h->stream));
    if (found) HIPCHK(h, hipMemcpyAsync(found, io.found, n * 4, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}
}  // extern "C"
