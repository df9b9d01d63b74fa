// sbm_occ_options.hip -- the switches of the occupancy map's log-odds mode that octomap keeps on the tree (include/sbm.h,
// "occupancy map: insert options"): the bounding box (setBBXMin / setBBXMax / useBBXLimit, OccupancyOcTreeBase.hxx:891-918) and
// change detection (enableChangeDetection / resetChangeDetection / changedKeys), whose per-slot states the apply kernel of
// sbm_occ_rays.hip steps and the fetch here reads.  gfx950. Nothing here contracts a multiply-add.
//
//   occ_change_count_kernel     slots with a change state, one atomic per wavefront
//   occ_change_compact_kernel   those slots -> dense (key, created) arrays for the map's radix sort
//   occ_change_flags_kernel     the sorted 32-bit payload -> one byte per key
#include "sbm_occ.h"

namespace sbm {
#pragma clang fp contract(off)

__global__ void __launch_bounds__(256) occ_change_count_kernel(const uint8_t* __restrict__ change, uint32_t slots, OccCounters* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  occ_wave_append(i < slots && change[i] != kOccChangeNone, &ctr->cursor);   // every lane is here
}

__global__ void __launch_bounds__(256) occ_change_compact_kernel(const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ change,
                                                                  uint32_t slots, uint32_t cap, unsigned long long* __restrict__ out_keys,
                                                                  unsigned* __restrict__ out_created, OccCounters* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint8_t s = i < slots ? change[i] : (uint8_t)kOccChangeNone;
  const uint32_t o = occ_wave_append(s != kOccChangeNone, &ctr->cursor);   // every lane is here
  if (s == kOccChangeNone || o >= cap) return;   // the host sized the outputs from the count pass
  out_keys[o] = keys[i];
  out_created[o] = s == kOccChangeCreated;
}

__global__ void __launch_bounds__(256) occ_change_flags_kernel(const unsigned* __restrict__ created, uint32_t n, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (uint8_t)created[i];
}

bool occ_axis_host(double factor, float coord, unsigned* k) {   // occ_axis of sbm_occ.h, the same statements
  const double f = floor(factor * (double)coord);
  if (!(f >= -32768.0 && f < 32768.0)) return false;
  *k = (unsigned)((int)f + 32768);
  return true;
}

// The slots with a change state, counted on the device and read back (a map that never enabled detection has none)
static int occ_change_count(sbm_occ_map* map, uint32_t* n) {
  sbm_handle* h = map->h;
  *n = 0;
  if (!map->change.p) return SBM_OK;
  HIPCHK(h, hipMemsetAsync(&map->ctr.as<OccCounters>()->cursor, 0, sizeof(unsigned), h->stream));
  hipLaunchKernelGGL(occ_change_count_kernel, dim3((map->slots + 255) / 256), dim3(256), 0, h->stream, map->change.as<uint8_t>(), map->slots,
                     map->ctr.as<OccCounters>());
  HIPCHK(h, hipGetLastError());
  OccCounters c;
  const int st = occ_read_counters(map, &c);
  if (st == SBM_OK) *n = c.cursor;
  return st;
}

// Sorted (key, created) of the changed voxels into d_keys / d_created (cap entries each; d_created may be null)
static int occ_changes_run(sbm_occ_map* map, unsigned long long* d_keys, uint8_t* d_created, size_t cap, size_t* count) {
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  HIPCHK(h, occ_clock_start(h, kOccFetch, kOccFetch));
  uint32_t n;
  int st = occ_change_count(map, &n);
  if (st != SBM_OK) return st;
  *count = n;
  if (n > cap) return SBM_ERR_SIZE;
  if (!n) return SBM_OK;
  const uint32_t tiles = (n + kOccTile - 1) / kOccTile;
  unsigned long long* kk[2] = {d_keys};
  unsigned* vv[2];
  HIPCHK(h, occ_sort_carve(h, n, &kk[1], &vv[1], &vv[0]));
  HIPCHK(h, h->occ.hist.grow((size_t)256 * tiles * 4, h->stream));
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  HIPCHK(h, hipMemsetAsync(&map->ctr.as<OccCounters>()->cursor, 0, sizeof(unsigned), h->stream));
  hipLaunchKernelGGL(occ_change_compact_kernel, dim3((map->slots + 255) / 256), dim3(256), 0, h->stream, map->keys.as<unsigned long long>(),
                     map->change.as<uint8_t>(), map->slots, n, kk[0], vv[0], map->ctr.as<OccCounters>());
  HIPCHK(h, hipGetLastError());
  st = occ_sort_run(h, kk, vv, n, h->occ.hist.as<unsigned>());
  if (st != SBM_OK) return st;
  if (d_created) {
    hipLaunchKernelGGL(occ_change_flags_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, vv[0], n, d_created);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, clk.add(kOccFetch, kOccBegin, kOccEnd));
  return SBM_OK;
}

}  // namespace sbm
using namespace sbm;

extern "C" {

int sbm_occ_set_bbx(sbm_occ_map* map, const float min[3], const float max[3]) {
  if (!map || !min || !max) return SBM_ERR_NULL;
  const double factor = 1. / map->p.resolution;
  unsigned kmin[3], kmax[3];
  for (int i = 0; i < 3; i++)
    if (!occ_axis_host(factor, min[i], &kmin[i]) || !occ_axis_host(factor, max[i], &kmax[i])) return SBM_ERR_SIZE;
  for (int i = 0; i < 3; i++) {
    map->bbx_min[i] = min[i], map->bbx_max[i] = max[i];
    map->bbx_min_key[i] = kmin[i], map->bbx_max_key[i] = kmax[i];
  }
  return SBM_OK;
}

int sbm_occ_use_bbx_limit(sbm_occ_map* map, int enable) {
  if (!map) return SBM_ERR_NULL;
  if (enable && map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  map->use_bbx = enable != 0;
  return SBM_OK;
}

int sbm_occ_get_bbx(sbm_occ_map* map, float min[3], float max[3], uint16_t min_key[3], uint16_t max_key[3], int* enabled) {
  if (!map) return SBM_ERR_NULL;
  for (int i = 0; i < 3; i++) {
    if (min) min[i] = map->bbx_min[i];
    if (max) max[i] = map->bbx_max[i];
    if (min_key) min_key[i] = (uint16_t)map->bbx_min_key[i];
    if (max_key) max_key[i] = (uint16_t)map->bbx_max_key[i];
  }
  if (enabled) *enabled = map->use_bbx ? 1 : 0;
  return SBM_OK;
}

int sbm_occ_enable_change_detection(sbm_occ_map* map, int enable) {
  if (!map) return SBM_ERR_NULL;
  if (enable && map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  if (enable && !map->change.p) {   // the first enable allocates the states: a map that never asks pays nothing
    sbm_handle* h = map->h;
    DeviceScope dscope(h->device);
    HIPCHK(h, dscope.enter());
    HIPCHK(h, map->change.grow(map->slots, h->stream));
    HIPCHK(h, hipMemsetAsync(map->change.p, 0, map->slots, h->stream));
  }
  map->detect = enable != 0;
  return SBM_OK;
}

int sbm_occ_change_detection_enabled(sbm_occ_map* map, int* enabled) {
  if (!map || !enabled) return SBM_ERR_NULL;
  *enabled = map->detect ? 1 : 0;
  return SBM_OK;
}

int sbm_occ_reset_change_detection(sbm_occ_map* map) {
  if (!map) return SBM_ERR_NULL;
  if (!map->change.p) return SBM_OK;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, hipMemsetAsync(map->change.p, 0, map->slots, h->stream));
  return SBM_OK;
}

int sbm_occ_num_changes(sbm_occ_map* map, size_t* count) {
  if (!map || !count) return SBM_ERR_NULL;
  if (map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  uint32_t n;
  const int st = occ_change_count(map, &n);
  if (st == SBM_OK) *count = n;
  return st;
}

int sbm_occ_fetch_changes_device(sbm_occ_map* map, void* d_keys, void* d_created, size_t cap, size_t* count) {
  if (!map || !count || (cap > 0 && !d_keys)) return SBM_ERR_NULL;
  if (((uintptr_t)d_keys & 7) || map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_changes_run(map, (unsigned long long*)d_keys, (uint8_t*)d_created, cap, count);
}

int sbm_occ_fetch_changes(sbm_occ_map* map, uint64_t* keys, uint8_t* created, size_t cap, size_t* count) {
  if (!map || !count || (cap > 0 && !keys)) return SBM_ERR_NULL;
  if (map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  uint32_t n;
  int st = occ_change_count(map, &n);
  if (st != SBM_OK) return st;
  *count = n;
  if (n > cap) return SBM_ERR_SIZE;
  if (!n) return SBM_OK;
  unsigned long long* d_k;
  uint8_t* d_c;
  HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& cv) { d_k = cv.take<unsigned long long>(n); d_c = cv.take<uint8_t>(n); }, occ_pad));
  st = occ_changes_run(map, d_k, d_c, n, count);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpyAsync(keys, d_k, *count * 8, hipMemcpyDeviceToHost, h->stream));
  if (created) HIPCHK(h, hipMemcpyAsync(created, d_c, *count, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

}  // extern "C"
