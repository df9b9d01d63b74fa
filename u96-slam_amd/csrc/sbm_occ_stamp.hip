// sbm_occ_stamp.hip -- a time stamp per voxel of the log-odds map, octomap's OcTreeStamped (OcTreeStamped.h, OcTreeStamped.cpp):
// the map's clock, degradeOutdatedNodes, and the reads that return the stamp: search by points, the sorted fetch, a tree's leaf
// lists and its root (getLastUpdateTime).
// gfx950. include/sbm.h ("occupancy map: time stamps per voxel") states the contract; a map that never enables stamps allocates
// and launches nothing of this file. The stamping itself is a switch of the two APPLY kernels (sbm_occ_rays.hip, sbm_occ_edit.hip),
// the carry one of the table's move (sbm_occ.h, sbm_occ_grow.hip), the forget-by-age pass one of the delete family
// (sbm_occ_edit.hip). Nothing here contracts a multiply-add.
//
//   occ_stamp_degrade_kernel   one lane per slot: an occupied voxel whose stamp is more than time_thres behind the clock gets one
//                              miss update, clamped; its stamp stays. Plain stores by the lane that owns the slot.
//   occ_stamp_search_kernel    one lane per point: state, log-odds and stamp.
//   occ_stamp_slots_kernel / occ_stamp_gather_kernel   the fetch: occupied slots -> (key, slot) pairs, sorted by the map's radix
//                              sort, then log-odds and stamp of each slot in key order.
//   occ_stamp_tree_lookup_kernel   the stamp of each entry of a tree's leaves call, by a binary search over its depth's codes. The
//                              stamped pruned tree itself is built in sbm_occ_tree.hip (occ_tree_parents<kStamp>), its stream written and
//                              loaded in sbm_occ_ot.hip behind the other id.
#include "sbm_occ.h"

namespace sbm {
#pragma clang fp contract(off)

struct OccStampDegrade {
  const unsigned long long* keys;
  float* logodds;
  const unsigned* stamps;
  uint32_t slots, clock, time_thres;
  float miss, cmin, cmax, thres;
  unsigned long long* count;
};

// degradeOutdatedNodes (OcTreeStamped.cpp): isNodeOccupied(leaf) && (query_time - leaf.getTimestamp()) > time_thres, in unsigned
// int, then integrateMissNoTime: updateNodeLogOdds of the plain tree, which adds and clamps and does not stamp
__global__ void __launch_bounds__(256) occ_stamp_degrade_kernel(OccStampDegrade g) {
#pragma clang fp contract(off)
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool degraded = false;
  if (i < g.slots && g.keys[i] != kOccEmpty) {
    float v = g.logodds[i];
    if (v >= g.thres && (uint32_t)(g.clock - g.stamps[i]) > g.time_thres) {
      v = v + g.miss;
      if (v < g.cmin) v = g.cmin;
      else if (v > g.cmax) v = g.cmax;
      g.logodds[i] = v;
      degraded = true;
    }
  }
  occ_wave_count(degraded, g.count);   // every lane is here
}

struct OccStampRead {
  double factor;
  float thres;
  uint32_t mask, max_probe;
  const unsigned long long* keys;
  const unsigned* vals;
  const unsigned* stamps;   // null: a map without stamps, every voxel 0
};

__global__ void __launch_bounds__(256) occ_stamp_search_kernel(const float* __restrict__ xyz, size_t n, OccStampRead g, int* __restrict__ state,
                                                                unsigned* __restrict__ value, unsigned* __restrict__ stamp) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned k0, k1, k2, word = 0x7FC00000u, s = 0;
  int st = SBM_OCC_CELL_OUT;
  if (occ_axis(g.factor, xyz[3 * i], &k0) && occ_axis(g.factor, xyz[3 * i + 1], &k1) && occ_axis(g.factor, xyz[3 * i + 2], &k2)) {
    uint32_t slot;
    st = SBM_OCC_CELL_UNKNOWN;
    if (occ_find(g.keys, occ_pack(k0, k1, k2), g.mask, g.max_probe, &slot)) {
      word = g.vals[slot];
      st = __uint_as_float(word) >= g.thres ? SBM_OCC_CELL_OCCUPIED : SBM_OCC_CELL_FREE;   // isNodeOccupied
      if (g.stamps) s = g.stamps[slot];
    }
  }
  state[i] = st;
  if (value) value[i] = word;
  if (stamp) stamp[i] = s;
}

__global__ void __launch_bounds__(256) occ_stamp_slots_kernel(const unsigned long long* __restrict__ keys, uint32_t slots, uint32_t cap,
                                                               unsigned long long* __restrict__ out_keys, unsigned* __restrict__ out_slot,
                                                               OccCounters* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long k = i < slots ? keys[i] : kOccEmpty;
  const uint32_t o = occ_wave_append(k != kOccEmpty, &ctr->cursor);   // every lane is here
  if (k == kOccEmpty || o >= cap) return;   // the host sized the outputs from ctr->size
  out_keys[o] = k;
  out_slot[o] = i;
}

__global__ void __launch_bounds__(256) occ_stamp_gather_kernel(const unsigned* __restrict__ slot_of, uint32_t n, uint32_t slots,
                                                                const unsigned* __restrict__ vals, const unsigned* __restrict__ stamps,
                                                                unsigned* __restrict__ out_vals, unsigned* __restrict__ out_stamps) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint32_t slot = slot_of[j];
  if (slot >= slots) return;
  if (out_vals) out_vals[j] = vals[slot];
  if (out_stamps) out_stamps[j] = stamps ? stamps[slot] : 0u;
}

struct OccStampLevels {   // every depth of a built tree: its codes and its stamps
  const unsigned long long* code[kOccDepth + 1];
  const unsigned* stamp[kOccDepth + 1];   // null: a tree without stamps
  uint32_t n[kOccDepth + 1];
};

// the stamp of each entry of a leaves call: (centre key, depth) -> the node, by a binary search over its depth's codes
__global__ void __launch_bounds__(256) occ_stamp_tree_lookup_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ depth,
                                                                     uint32_t n, OccStampLevels t, unsigned* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  const int d = min(max(depth[i], 0), kOccDepth);
  const unsigned long long code = occ_code((unsigned)(key >> 32) & 0xFFFF, (unsigned)(key >> 16) & 0xFFFF, (unsigned)key & 0xFFFF) >> (3 * (kOccDepth - d));
  const unsigned long long* codes = t.code[d];
  uint32_t lo = 0, hi = t.n[d];
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (codes[mid] < code) lo = mid + 1;
    else hi = mid;
  }
  out[i] = (t.stamp[d] && lo < t.n[d] && codes[lo] == code) ? t.stamp[d][lo] : 0u;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
constexpr size_t kOccStampMax = (size_t)1 << 30;

static int occ_stamp_search_run(sbm_occ_map* map, size_t n, const float* d_xyz, float thres, int* d_state, unsigned* d_value,
                                unsigned* d_stamp, int sync) {
  sbm_handle* h = map->h;
  return occ_timed_run(h, kOccSearch, n > 0, sync, [&]() -> int {
    OccStampRead g;
    g.factor = 1. / map->p.resolution;
    g.thres = thres;
    occ_probe(map, &g.mask, &g.max_probe);
    g.keys = map->keys.as<unsigned long long>();
    g.vals = map->hits.as<unsigned>();
    g.stamps = map->stamp.as<unsigned>();
    hipLaunchKernelGGL(occ_stamp_search_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, d_xyz, n, g, d_state, d_value, d_stamp);
    return SBM_OK;
  });
}

// Sorted keys of the map into d_keys, with the log-odds and the stamp of each (either may be null)
static int occ_stamp_fetch_run(sbm_occ_map* map, unsigned long long* d_keys, unsigned* d_vals, unsigned* d_stamps, size_t cap, size_t* count) {
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  HIPCHK(h, occ_clock_start(h, kOccFetch, kOccFetch));
  OccCounters c;
  int st = occ_read_counters(map, &c);
  if (st != SBM_OK) return st;
  const uint32_t n = c.size;
  *count = n;
  if (n > cap) return SBM_ERR_SIZE;
  if (n) {
    const uint32_t tiles = (n + kOccTile - 1) / kOccTile;
    unsigned long long* kk[2] = {d_keys};
    unsigned* vv[2];
    HIPCHK(h, occ_sort_carve(h, n, &kk[1], &vv[1], &vv[0]));
    HIPCHK(h, h->occ.hist.grow((size_t)256 * tiles * 4, h->stream));
    HIPCHK(h, clk.mark(kOccBegin, h->stream));
    HIPCHK(h, hipMemsetAsync(&map->ctr.as<OccCounters>()->cursor, 0, sizeof(unsigned), h->stream));
    hipLaunchKernelGGL(occ_stamp_slots_kernel, dim3((map->slots + 255) / 256), dim3(256), 0, h->stream, map->keys.as<unsigned long long>(), map->slots,
                       n, kk[0], vv[0], map->ctr.as<OccCounters>());
    HIPCHK(h, hipGetLastError());
    st = occ_sort_run(h, kk, vv, n, h->occ.hist.as<unsigned>());
    if (st != SBM_OK) return st;
    hipLaunchKernelGGL(occ_stamp_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, vv[0], n, map->slots, map->hits.as<unsigned>(),
                       map->stamp.as<unsigned>(), d_vals, d_stamps);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, clk.mark(kOccEnd, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, clk.add(kOccFetch, kOccBegin, kOccEnd));
  }
  return c.overflow ? SBM_ERR_OCC_FULL : SBM_OK;
}

static int occ_stamp_leaves_run(sbm_occ_tree* t, const unsigned long long* d_keys, const int* d_depth, unsigned* d_stamp, uint32_t n) {
  sbm_handle* h = t->h;
  if (!n) return SBM_OK;
  OccStampLevels lv;
  memset(&lv, 0, sizeof(lv));
  unsigned *leaf = nullptr, *node = nullptr;
  if (t->built && t->stamped) occ_tree_stamps(t, &leaf, &node);
  for (int d = 0; d <= kOccDepth; d++) {
    const OccLevel l = occ_tree_level(t, d);
    lv.code[d] = l.code;
    lv.n[d] = l.n;
    lv.stamp[d] = !leaf ? nullptr : d == kOccDepth ? leaf : node + t->off[d];
  }
  hipLaunchKernelGGL(occ_stamp_tree_lookup_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, d_keys, d_depth, n, lv, d_stamp);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

}  // namespace sbm
using namespace sbm;

extern "C" {

int sbm_occ_stamp_enable(sbm_occ_map* map) {
  if (!map) return SBM_ERR_NULL;
  if (map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  if (map->color.p) return SBM_ERR_UNSUPPORTED;   // a map is one octomap class
  if (map->stamp.p) return SBM_OK;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  // The words first, into buffers of their own: a refused allocation frees what it got and leaves the map as it was.
  DevBuf words = {}, count = {};
  hipError_t e = words.grow((size_t)map->slots * 4, h->stream);
  if (e == hipSuccess) e = count.grow(sizeof(unsigned long long), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(words.p, 0, (size_t)map->slots * 4, h->stream);   // existing voxels have stamp 0, as after a load
  if (e != hipSuccess) {
    words.release();
    count.release();
    h->last_hip = (int)e;
    return e == hipErrorOutOfMemory ? SBM_ERR_NOMEM : SBM_ERR_HIP;
  }
  const int st = occ_logodds_alloc(map);   // enabling fixes the mode of a fresh map, as a colour call or an edit does
  if (st != SBM_OK) {   // what this may have allocated is what the first log-odds insert allocates: the map's content and mode are as they were
    words.release();
    count.release();
    return st;
  }
  std::swap(map->stamp, words);
  std::swap(map->stamp_count, count);
  map->mode = kOccModeLogOdds;
  return SBM_OK;
}

int sbm_occ_stamp_enabled(const sbm_occ_map* map, int* enabled) {
  if (!map || !enabled) return SBM_ERR_NULL;
  *enabled = map->stamp.p != nullptr;
  return SBM_OK;
}

int sbm_occ_stamp_set_time(sbm_occ_map* map, uint32_t clock) {
  if (!map) return SBM_ERR_NULL;
  map->clock = clock;
  return SBM_OK;
}

int sbm_occ_stamp_time(const sbm_occ_map* map, uint32_t* clock) {
  if (!map || !clock) return SBM_ERR_NULL;
  *clock = map->clock;
  return SBM_OK;
}

int sbm_occ_stamp_degrade(sbm_occ_map* map, uint32_t time_thres, const sbm_occ_ray_params* params, uint64_t* degraded) {
  if (!map || !params || !degraded) return SBM_ERR_NULL;
  const int st = occ_ray_params_check(params);
  if (st != SBM_OK) return st;
  if (!map->stamp.p || map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  OccStampDegrade g;
  g.keys = map->keys.as<unsigned long long>();
  g.logodds = map->hits.as<float>();
  g.stamps = map->stamp.as<unsigned>();
  g.slots = map->slots;
  g.clock = map->clock;
  g.time_thres = time_thres;
  g.miss = occ_logodds(params->prob_miss);
  g.cmin = occ_logodds(params->clamp_min);
  g.cmax = occ_logodds(params->clamp_max);
  g.thres = occ_logodds(params->occupancy_thres);
  g.count = map->stamp_count.as<unsigned long long>();
  HIPCHK(h, occ_clock_start(h, kOccRaysApply, kOccRaysApply));
  HIPCHK(h, hipMemsetAsync(g.count, 0, sizeof(unsigned long long), h->stream));
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  hipLaunchKernelGGL(occ_stamp_degrade_kernel, dim3((g.slots + 255) / 256), dim3(256), 0, h->stream, g);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  unsigned long long count = 0;
  HIPCHK(h, hipMemcpyAsync(&count, g.count, sizeof(count), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, clk.add(kOccRaysApply, kOccBegin, kOccEnd));
  *degraded = count;
  return SBM_OK;
}

int sbm_occ_stamp_leaves_device(sbm_occ_tree* tree, int max_depth, void* d_keys, void* d_depth, void* d_value, void* d_stamp, size_t cap,
                                size_t* count) {
  if (!tree || !count || (cap > 0 && (!d_keys || !d_depth))) return SBM_ERR_NULL;   // the order of sbm_occ_tree_leaves_device
  if (max_depth < 0 || max_depth > kOccDepth) return SBM_ERR_SIZE;
  if ((uintptr_t)d_stamp & 3) return SBM_ERR_UNSUPPORTED;
  const int st = sbm_occ_tree_leaves_device(tree, max_depth, d_keys, d_depth, d_value, cap, count);
  if (st != SBM_OK || !d_stamp) return st;
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  return occ_stamp_leaves_run(tree, (const unsigned long long*)d_keys, (const int*)d_depth, (unsigned*)d_stamp, (uint32_t)*count);
}

int sbm_occ_stamp_leaves(sbm_occ_tree* tree, int max_depth, uint64_t* keys, int32_t* depth, float* value, uint32_t* stamp, size_t cap,
                         size_t* count) {
  if (!tree || !count || (cap > 0 && (!keys || !depth || !stamp))) return SBM_ERR_NULL;
  sbm_handle* h = tree->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  size_t n = 0;
  int st = sbm_occ_tree_leaves_device(tree, max_depth, nullptr, nullptr, nullptr, 0, &n);   // the count alone
  if (st != SBM_OK && st != SBM_ERR_SIZE) return st;
  *count = n;
  if (n > cap) return SBM_ERR_SIZE;
  if (!n) return SBM_OK;
  struct { unsigned long long* keys; int* depth; unsigned *value, *stamp; } io;
  HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& c) {
    io = {c.take<unsigned long long>(n), c.take<int>(n), c.take<unsigned>(n), c.take<unsigned>(n)};
  }, occ_pad));
  st = sbm_occ_stamp_leaves_device(tree, max_depth, io.keys, io.depth, io.value, io.stamp, n, count);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpyAsync(keys, io.keys, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(depth, io.depth, n * 4, hipMemcpyDeviceToHost, h->stream));
  if (value) HIPCHK(h, hipMemcpyAsync(value, io.value, n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(stamp, io.stamp, n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

// getLastUpdateTime(): the root's stamp. 0 for a tree without stamps or without a voxel.
int sbm_occ_stamp_root(sbm_occ_tree* tree, uint32_t* stamp) {
  if (!tree || !stamp) return SBM_ERR_NULL;
  *stamp = 0;
  if (!tree->built || !tree->stamped || !tree->count[0]) return SBM_OK;
  sbm_handle* h = tree->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  unsigned *leaf, *node;
  occ_tree_stamps(tree, &leaf, &node);
  uint32_t v = 0;
  HIPCHK(h, hipMemcpyAsync(&v, node + tree->off[0], 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *stamp = v;
  return SBM_OK;
}

int sbm_occ_stamp_search_device(sbm_occ_map* map, size_t n, const void* d_xyz, float occupancy_thres_log, void* d_state, void* d_value,
                                void* d_stamp, int sync) {
  if (!map || (n > 0 && (!d_xyz || !d_state))) return SBM_ERR_NULL;
  if (std::isnan(occupancy_thres_log)) return SBM_ERR_SIZE;
  if (n > kOccStampMax || map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  if (((uintptr_t)d_xyz | (uintptr_t)d_state | (uintptr_t)d_value | (uintptr_t)d_stamp) & 3) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_stamp_search_run(map, n, (const float*)d_xyz, occupancy_thres_log, (int*)d_state, (unsigned*)d_value, (unsigned*)d_stamp, sync);
}

int sbm_occ_stamp_search(sbm_occ_map* map, size_t n, const float* xyz, float occupancy_thres_log, int32_t* state, void* value, uint32_t* stamp) {
  if (!map || (n > 0 && (!xyz || !state))) return SBM_ERR_NULL;
  if (std::isnan(occupancy_thres_log)) return SBM_ERR_SIZE;
  if (n > kOccStampMax || map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  // the stamps ride in the staging's fourth array, the one a tree's search uses for its depths
  return occ_search_host(h, n, xyz, true, state, value, (int32_t*)stamp, [&](float* d_xyz, int* d_state, unsigned* d_value, int* d_found) {
    return occ_stamp_search_run(map, n, d_xyz, occupancy_thres_log, d_state, d_value, (unsigned*)d_found, 0);
  });
}

int sbm_occ_stamp_fetch_device(sbm_occ_map* map, void* d_keys, void* d_logodds, void* d_stamps, size_t cap, size_t* count) {
  if (!map || !count || (cap > 0 && !d_keys)) return SBM_ERR_NULL;
  if (((uintptr_t)d_keys & 7) || (((uintptr_t)d_logodds | (uintptr_t)d_stamps) & 3) || map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_stamp_fetch_run(map, (unsigned long long*)d_keys, (unsigned*)d_logodds, (unsigned*)d_stamps, cap, count);
}

int sbm_occ_stamp_fetch(sbm_occ_map* map, uint64_t* keys, float* logodds, uint32_t* stamps, size_t cap, size_t* count) {
  if (!map || !count || (cap > 0 && !keys)) return SBM_ERR_NULL;
  if (map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  OccCounters c;
  int st = occ_read_counters(map, &c);
  if (st != SBM_OK) return st;
  *count = c.size;
  if (c.size > cap) return SBM_ERR_SIZE;
  if (!c.size) return c.overflow ? SBM_ERR_OCC_FULL : SBM_OK;
  unsigned long long* d_k;
  unsigned *d_v, *d_s;
  HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& cv) {
    d_k = cv.take<unsigned long long>(c.size), d_v = cv.take<unsigned>(c.size), d_s = cv.take<unsigned>(c.size);
  }, occ_pad));
  st = occ_stamp_fetch_run(map, d_k, d_v, d_s, c.size, count);
  if (st != SBM_OK && st != SBM_ERR_OCC_FULL) return st;
  HIPCHK(h, hipMemcpyAsync(keys, d_k, *count * 8, hipMemcpyDeviceToHost, h->stream));
  if (logodds) HIPCHK(h, hipMemcpyAsync(logodds, d_v, *count * 4, hipMemcpyDeviceToHost, h->stream));
  if (stamps) HIPCHK(h, hipMemcpyAsync(stamps, d_s, *count * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return st;
}

}  // extern "C"
