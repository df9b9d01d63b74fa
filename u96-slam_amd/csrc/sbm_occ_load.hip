// sbm_occ_load.hip -- a .bt stream into the occupancy map, octomap's readBinary (include/sbm.h, "occupancy map: load a .bt
// stream"): the host parses the pruned tree (occ_bt_parse, sbm_occ_bt.hip) and the device expands it.  gfx950.
//   occ_load_kernel     one lane per depth-16 voxel finds its leaf in the prefix array of the leaf volumes, de-interleaves its
//                       Morton code and claims its slot.
// A pruned leaf of depth d stands for 8^(16-d) voxels whose Morton codes are its first code OR'd with 0 .. 8^(16-d) - 1.
#include <stdio.h>
#include <stdlib.h>

#include "sbm_occ.h"

namespace sbm {

struct OccLoad {
  uint32_t leaves, total;        // total: the voxels of all leaves, at most 2^30
  uint32_t mask, max_probe;
  unsigned vmin, vmax;           // float bits of the clamp log-odds: a free leaf's value and an occupied leaf's
};
#ifndef SBM_OCC_LOAD_SHARED
#define SBM_OCC_LOAD_SHARED 0   // 1 builds the wavefront-shared leaf search, for tools/bench_occupancy_load.py to time
#endif
constexpr bool kOccLoadShared = SBM_OCC_LOAD_SHARED != 0;

// One output voxel per lane. leaf[j]: first code << 8 | depth << 1 | occupied; first[j]: the voxels of the leaves before j
// (strictly ascending, first[0] == 0). The voxels of one load are distinct, so a claimed slot has one writer: the value is a plain
// store, and the only atomics are the key's compare-and-swap and the integer counters, one add per wavefront.
__global__ void __launch_bounds__(256) occ_load_kernel(const unsigned long long* __restrict__ leaf, const unsigned* __restrict__ first,
                                                        OccLoad g, unsigned long long* __restrict__ keys, unsigned* __restrict__ vals,
                                                        OccCounters* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < g.total;
  bool claimed = false, lost = false;
  if (live) {
    uint32_t lo = 0, hi = g.leaves;   // the last leaf with first[leaf] <= i
    if (kOccLoadShared) {             // lane 0's leaf first: a leaf holds at least one voxel, so lane l's is at most l leaves on
      if ((threadIdx.x & 63) == 0)
        while (hi - lo > 1) {
          const uint32_t mid = lo + (hi - lo) / 2;
          if (first[mid] <= i) lo = mid;
          else hi = mid;
        }
      lo = __builtin_amdgcn_readfirstlane(lo);   // lane 0 is live wherever a lane of its wavefront is
      hi = min(lo + (threadIdx.x & 63) + 1, g.leaves);
    }
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (first[mid] <= i) lo = mid;
      else hi = mid;
    }
    const unsigned long long word = leaf[lo];
    const unsigned long long key = occ_key_of_code((word >> 8) | (unsigned long long)(i - first[lo]));
    uint32_t slot;
    lost = !occ_find_or_claim(keys, key, g.mask, g.max_probe, &slot, &claimed);
    if (!lost) vals[slot] = (word & 1) ? g.vmax : g.vmin;
  }
  const unsigned long long got = __ballot(claimed), over = __ballot(lost);
  if ((threadIdx.x & 63) == 0) {
    if (got) atomicAdd(&ctr->size, (unsigned)__popcll(got));
    if (over) atomicAdd(&ctr->overflow, (unsigned long long)__popcll(over));
  }
}

// ---- loading a .bt stream, host side ----------------------------------------------------------------------------------------
// readBinary into the map. Everything that can refuse the stream comes before the map is touched.
static int occ_load_run(sbm_occ_map* map, const uint8_t* bytes, size_t n, const sbm_occ_ray_params* p, int sync) {
  sbm_handle* h = map->h;
  sbm_occ_binary_header info;
  std::vector<OccBtLeaf> leaves;
  int st = occ_bt_parse(bytes, n, &info, &leaves, false);
  if (st != SBM_OK) return st;
  if (info.resolution != occ_printed_resolution(map->p.resolution)) return SBM_ERR_SIZE;
  if (info.voxels > map->capacity && !occ_can_reserve(map, info.voxels)) return SBM_ERR_OCC_FULL;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  StageClock& clk = h->occ.clock;
  HIPCHK(h, occ_clock_start(h, kOccLoad, kOccLoad));
  const size_t count = leaves.size();
  if (!count) {                           // size 0: clear() and nothing else
    st = occ_clear(map);
    if (st == SBM_OK && sync) HIPCHK(h, hipStreamSynchronize(h->stream));
    return st;
  }
  std::vector<unsigned> first;
  try {
    first.resize(count);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  uint64_t run = 0;
  for (size_t i = 0; i < count; i++) {
    first[i] = (unsigned)run;             // below the capacity, which is at most 2^30
    run += (uint64_t)1 << (3 * (16 - occ_bt_depth(leaves[i])));
  }
  st = occ_logodds_alloc(map);
  if (st != SBM_OK) return st;
  unsigned long long* d_word;
  unsigned* d_first;
  HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& c) { d_word = c.take<unsigned long long>(count); d_first = c.take<unsigned>(count); }, occ_pad));
  HIPCHK(h, hipMemcpyAsync(d_word, leaves.data(), count * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_first, first.data(), count * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // the host arrays end with this call
  OccLoad g;
  g.leaves = (uint32_t)count;
  g.total = (uint32_t)info.voxels;
  const float cmin = occ_logodds(p->clamp_min), cmax = occ_logodds(p->clamp_max);
  memcpy(&g.vmin, &cmin, 4);
  memcpy(&g.vmax, &cmax, 4);
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  st = occ_clear(map);
  if (st != SBM_OK) return st;
  map->mode = kOccModeLogOdds;
  if (info.voxels > map->capacity) {       // a growing map reserves the stream's voxels: the emptied table moves nothing
    st = occ_rehash(map, info.voxels);
    if (st != SBM_OK && st != SBM_ERR_NOMEM) return st;   // refused: the load goes on into the table it has and counts what it loses
    map->overflow_known = st == SBM_OK;
  }
  occ_probe(map, &g.mask, &g.max_probe);
  hipLaunchKernelGGL(occ_load_kernel, dim3((g.total + 255) / 256), dim3(256), 0, h->stream, d_word, d_first, g,
                     map->keys.as<unsigned long long>(), map->hits.as<unsigned>(), map->ctr.as<OccCounters>());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(kOccLoad, kOccBegin, kOccEnd));
  return occ_overflow_status(map, sync);
}

}  // namespace sbm
using namespace sbm;

extern "C" {
int sbm_occ_load_binary(sbm_occ_map* map, const void* bytes, size_t n, const sbm_occ_ray_params* params, int sync) {
  if (!map || !params || (n > 0 && !bytes)) return SBM_ERR_NULL;
  const int st = occ_ray_params_check(params);
  if (st != SBM_OK) return st;
  return occ_load_run(map, (const uint8_t*)bytes, n, params, sync);
}

int sbm_occ_read_binary(sbm_occ_map* map, const char* path, const sbm_occ_ray_params* params, int sync) {
  if (!map || !path || !params) return SBM_ERR_NULL;
  const int st = occ_ray_params_check(params);
  if (st != SBM_OK) return st;
  std::vector<uint8_t> data;
  const int rd = occ_read_file(path, &data);
  if (rd != SBM_OK) return rd;
  return occ_load_run(map, data.data(), data.size(), params, sync);
}
}  // extern "C"
