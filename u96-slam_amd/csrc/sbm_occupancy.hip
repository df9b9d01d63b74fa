// sbm_occupancy.hip -- the occupancy voxel map of the reference's buildOccupancyGridMap (src/slam/src/core/main.cpp:495-561)
// as a device-side set of octomap keys: the table, its hit-count insert, and the compaction and radix sort through which every
// ordered reading of the table goes (the fetches here; the tree's build and leaves in sbm_occ_tree.hip).  gfx950.
// include/sbm.h ("occupancy map: buildOccupancyGridMap") states the arithmetic; the point functions are those of
// sbm_consume.hip (sbm_consume_math.h). Nothing here contracts a multiply-add (the pragma below and -ffp-contract=off).
// The family's other files are sbm_occ_rays, _query, _tree, _bt and _load.hip; what two of them need is in sbm_occ.h, once.
//
//   occ_insert_kernel   one thread per pixel: disparity -> point -> two transforms -> gate -> key; the wavefront then reduces
//                       its 64 keys to distinct leaders with lane counts (ballot + readlane over the distinct values) and only
//                       the leaders touch the table: a 64-bit compare-and-swap on the key slot, an atomic add of the lane count.
//   occ_compact_kernel  occupied slots -> dense (key, hits) arrays, one atomic per wavefront.
//   occ_hist / occ_scan / occ_scatter   one 8-bit pass of an LSD radix sort: digit counts per tile, an exclusive scan of the
//                       digit-major count table, and a stable scatter (one wavefront per tile walks it 64 keys at a time and
//                       ranks equal digits by ballots).
#include "sbm_occ.h"

namespace sbm {
#pragma clang fp contract(off)

constexpr int kOccChunk = 64;        // planes per insert launch: their poses travel as kernel arguments (3 KiB)
constexpr size_t kOccMaxCapacity = (size_t)1 << 30;
struct OccPoses { float t[kOccChunk][12]; };

__global__ void __launch_bounds__(256) occ_insert_kernel(const int16_t* __restrict__ disp, OccGeom g, sbm_stereo_model m, OccPoses poses,
                                                          unsigned long long* __restrict__ keys, unsigned* __restrict__ hits,
                                                          OccCounters* __restrict__ ctr) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  unsigned long long key = kOccEmpty;
  const float* pose = poses.t[blockIdx.y];
  Pt3 p;
  if (i < g.W * g.H && occ_world_point(disp + (size_t)blockIdx.y * g.W * g.H, i, g, m, pose, &p)) {
    const float vx = p.x - pose[3], vy = p.y - pose[7], vz = p.z - pose[11];
    const float nsq = vx * vx + vy * vy + vz * vz;          // Vector3::norm_sq, a float expression
    unsigned k0, k1, k2;
    if (__dsqrt_rn((double)nsq) <= (double)g.range_max_sqrd && occ_axis(g.factor, p.x, &k0) && occ_axis(g.factor, p.y, &k1) &&
        occ_axis(g.factor, p.z, &k2))
      key = occ_pack(k0, k1, k2);
  }
  // the wavefront's distinct keys: the lowest lane of each value leads and learns how many lanes hold it
  const int lane = threadIdx.x & 63;
  const unsigned lo = (unsigned)key, hi = (unsigned)(key >> 32);
  unsigned long long todo = __ballot(key != kOccEmpty);
  unsigned count = 0;
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned llo = __builtin_amdgcn_readlane(lo, leader), lhi = __builtin_amdgcn_readlane(hi, leader);
    const unsigned long long same = __ballot(lo == llo && hi == lhi);   // the empty word has hi = 0xFFFFFFFF: no key matches it
    if (lane == leader) count = __popcll(same);
    todo &= ~same;
  }
  if (!count) return;
  uint32_t slot;
  bool claimed = false;
  const bool found = occ_find_or_claim(keys, key, g.mask, g.max_probe, &slot, &claimed);
  if (claimed) atomicAdd(&ctr->size, 1u);
  if (found) atomicAdd(&hits[slot], count);
  else atomicAdd(&ctr->overflow, (unsigned long long)count);
}

__global__ void __launch_bounds__(256) occ_compact_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ hits,
                                                           uint32_t slots, uint32_t cap, unsigned long long* __restrict__ out_keys,
                                                           unsigned* __restrict__ out_hits, OccCounters* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long k = i < slots ? keys[i] : kOccEmpty;
  const uint32_t o = occ_wave_append(k != kOccEmpty, &ctr->cursor);   // every lane is here
  if (k == kOccEmpty || o >= cap) return;   // the host sized the outputs from ctr->size; a slot claimed since then has no room
  out_keys[o] = k;
  out_hits[o] = hits[i];
}

// digit counts of one tile: hist[digit * tiles + tile]
__global__ void __launch_bounds__(256) occ_hist_kernel(const unsigned long long* __restrict__ keys, uint32_t n, int shift,
                                                        unsigned* __restrict__ hist, uint32_t tiles) {
  __shared__ unsigned cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * kOccTile;
  for (uint32_t j = threadIdx.x; j < kOccTile && base + j < n; j += 256) atomicAdd(&cnt[(keys[base + j] >> shift) & 255], 1u);
  __syncthreads();
  hist[threadIdx.x * tiles + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of the digit-major table in place; one workgroup, thread = digit
__global__ void __launch_bounds__(256) occ_scan_kernel(unsigned* __restrict__ hist, uint32_t tiles) {
  __shared__ unsigned total[256];
  unsigned* row = hist + (size_t)threadIdx.x * tiles;
  unsigned sum = 0;
  for (uint32_t t = 0; t < tiles; t++) {
    const unsigned v = row[t];
    row[t] = sum;
    sum += v;
  }
  total[threadIdx.x] = sum;
  __syncthreads();
  unsigned before = 0;
  for (int d = 0; d < (int)threadIdx.x; d++) before += total[d];
  for (uint32_t t = 0; t < tiles; t++) row[t] += before;
}

// stable scatter of one tile by one wavefront
__global__ void __launch_bounds__(64) occ_scatter_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                                                          uint32_t n, int shift, const unsigned* __restrict__ hist, uint32_t tiles,
                                                          unsigned long long* __restrict__ out_keys, unsigned* __restrict__ out_vals) {
  __shared__ unsigned offs[256];
  const int lane = threadIdx.x;
  for (int d = lane; d < 256; d += 64) offs[d] = hist[(size_t)d * tiles + blockIdx.x];
  __syncthreads();
  const uint32_t base = blockIdx.x * kOccTile;
  for (uint32_t j = 0; j < kOccTile && base + j < n; j += 64) {   // the condition is the same for every lane
    const uint32_t i = base + j + lane;
    const bool live = i < n;
    const unsigned long long k = live ? keys[i] : 0;
    const unsigned digit = (unsigned)(k >> shift) & 255;
    unsigned long long same = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const unsigned long long has = __ballot((digit >> b) & 1);
      same &= ((digit >> b) & 1) ? has : ~has;
    }
    const unsigned rank = __popcll(same & ((1ull << lane) - 1));
    const unsigned pos = live ? offs[digit] + rank : 0;
    __syncthreads();
    if (live && rank + 1 == (unsigned)__popcll(same)) offs[digit] = pos + 1;   // the last lane of a digit moves its offset on
    __syncthreads();
    if (live && pos < n) {
      out_keys[pos] = k;
      out_vals[pos] = vals[i];
    }
  }
}

int occ_read_counters(sbm_occ_map* map, OccCounters* c) {
  sbm_handle* h = map->h;
  HIPCHK(h, hipMemcpyAsync(c, map->ctr.p, sizeof(*c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int occ_clear(sbm_occ_map* map) {
  sbm_handle* h = map->h;
  HIPCHK(h, hipMemsetAsync(map->keys.p, 0xFF, (size_t)map->slots * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(map->hits.p, 0, (size_t)map->slots * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(map->ctr.p, 0, sizeof(OccCounters), h->stream));
  if (map->flags.p) HIPCHK(h, hipMemsetAsync(map->flags.p, 0, (size_t)map->slots * 4, h->stream));
  if (map->change.p) HIPCHK(h, hipMemsetAsync(map->change.p, 0, map->slots, h->stream));   // the switches and the box stay
  if (map->color.p) HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)map->color.p, (int)kOccWhite, map->slots, h->stream));   // every voxel white
  if (map->stamp.p) HIPCHK(h, hipMemsetAsync(map->stamp.p, 0, (size_t)map->slots * 4, h->stream));   // every stamp 0; the clock stays
  map->mode = kOccModeNone;
  map->scan = 0;
  map->size_bound = 0;
  map->overflow = 0;
  map->overflow_known = true;
  return SBM_OK;
}

void occ_probe(const sbm_occ_map* map, uint32_t* mask, uint32_t* max_probe) {
  *mask = map->slots - 1;
  *max_probe = std::min(map->slots, kOccMaxProbe);
}

int occ_check_insert(const sbm_occ_map* map, int n, const void* disp, int width, int height, int scale, const sbm_stereo_model* model,
                     const float* poses) {
  if (!map || !disp || !model || !poses) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width <= 0 || height <= 0 || scale <= 0) return SBM_ERR_SIZE;
  if ((size_t)width * height > ((size_t)1 << 30) || (size_t)width * scale > ((size_t)1 << 24) || (size_t)height * scale > ((size_t)1 << 24))
    return SBM_ERR_UNSUPPORTED;   // pixel coordinates stay exact in float, the pixel index in int
  return SBM_OK;
}

static const char* const kOccNames[] = {"occ_insert", "occ_fetch", "occ_rays_mark", "occ_rays_apply", "occ_search", "occ_cast",
                                        "occ_tree_build", "occ_tree_query", "occ_load"};
StageTable occ_stages() { return stage_table<kOccStageCount, kOccMarkCount>(kOccNames); }

hipError_t occ_clock_start(sbm_handle* h, int a, int b) {
  StageClock& clk = h->occ.clock;
  float keep[kOccStageCount];
  for (int i = 0; i < kOccStageCount; i++) keep[i] = clk.ms[i];
  const hipError_t e = clk.start(occ_stages(), h->profiling != 0);
  for (int i = 0; i < kOccStageCount; i++)
    if (clk.on && i != a && i != b) clk.ms[i] = keep[i];
  return e;
}

int occ_overflow_status(sbm_occ_map* map, int sync) {
  if (!sync && map->grow && map->overflow_known) return map->overflow ? SBM_ERR_OCC_FULL : SBM_OK;   // read inside the call
  if (!sync && !map->h->occ.clock.on) return SBM_OK;
  OccCounters c;
  const int st = occ_read_counters(map, &c);
  return st != SBM_OK ? st : c.overflow ? SBM_ERR_OCC_FULL : SBM_OK;
}

static int occ_insert_run(sbm_occ_map* map, int n, const int16_t* d_disp, int W, int H, int scale, const sbm_stereo_model* model,
                          const float* poses, int sync) {
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  HIPCHK(h, occ_clock_start(h, kOccInsert, kOccInsert));
  OccGeom g;
  g.W = W;
  g.H = H;
  g.scale = scale;
  g.range_max_sqrd = map->p.range_max * map->p.range_max;
  g.factor = 1. / map->p.resolution;
  occ_probe(map, &g.mask, &g.max_probe);
  const size_t plane = (size_t)W * H;
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  for (int c0 = 0; c0 < n; c0 += kOccChunk) {
    const int m = std::min(kOccChunk, n - c0);
    const size_t points = plane * m;
    if (map->grow && map->size_bound + points > map->capacity) {
      // The launch cannot be shown to fit and its counts cannot be added twice: a claim pass first, redone on a larger table
      // while it loses keys. After it the insert finds every key, unless the ceiling or an allocation stopped the growth:
      // then the insert itself counts what it loses, as on a map that does not grow.
      unsigned long long before;
      int st = occ_overflow_before(map, &before);
      OccCounters c = {};
      for (bool again = true; st == SBM_OK && again;) {
        occ_probe(map, &g.mask, &g.max_probe);
        st = occ_claim_launch(map, d_disp + plane * c0, g, model, poses + (size_t)12 * c0, m);
        if (st == SBM_OK) st = occ_grow_settle(map, before, &c, &again);
      }
      if (st == SBM_OK && c.overflow > before) st = occ_set_overflow(map, before);
      if (st != SBM_OK) return st;
      occ_probe(map, &g.mask, &g.max_probe);
      map->size_bound = c.size;
      map->overflow_known = c.overflow == before;   // an insert that loses points counts them on the device
    } else {
      map->size_bound = std::min(map->size_bound + points, (size_t)map->slots);
    }
    OccPoses ps;
    memset(&ps, 0, sizeof(ps));
    memcpy(ps.t, poses + (size_t)12 * c0, sizeof(float) * 12 * m);
    hipLaunchKernelGGL(occ_insert_kernel, dim3((unsigned)((plane + 255) / 256), m), dim3(256), 0, h->stream, d_disp + plane * c0, g,
                       *model, ps, map->keys.as<unsigned long long>(), map->hits.as<unsigned>(), map->ctr.as<OccCounters>());
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(kOccInsert, kOccBegin, kOccEnd));
  return occ_overflow_status(map, sync);
}

int occ_sort_run(sbm_handle* h, unsigned long long* const kk[2], unsigned* const vv[2], uint32_t n, unsigned* hist) {
  const uint32_t tiles = (n + kOccTile - 1) / kOccTile;
  for (int pass = 0; pass < 6; pass++) {
    const int a = pass & 1, b = a ^ 1;
    hipLaunchKernelGGL(occ_hist_kernel, dim3(tiles), dim3(256), 0, h->stream, kk[a], n, 8 * pass, hist, tiles);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(occ_scan_kernel, dim3(1), dim3(256), 0, h->stream, hist, tiles);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(occ_scatter_kernel, dim3(tiles), dim3(64), 0, h->stream, kk[a], vv[a], n, 8 * pass, hist, tiles, kk[b], vv[b]);
    HIPCHK(h, hipGetLastError());
  }
  return SBM_OK;
}

int occ_compact_run(sbm_occ_map* map, uint32_t n, unsigned long long* d_keys, unsigned* d_vals) {
  sbm_handle* h = map->h;
  HIPCHK(h, hipMemsetAsync(&map->ctr.as<OccCounters>()->cursor, 0, sizeof(unsigned), h->stream));
  hipLaunchKernelGGL(occ_compact_kernel, dim3((map->slots + 255) / 256), dim3(256), 0, h->stream, map->keys.as<unsigned long long>(),
                     map->hits.as<unsigned>(), map->slots, n, d_keys, d_vals, map->ctr.as<OccCounters>());
  HIPCHK(h, hipGetLastError());
  return SBM_OK;
}

// Sorted (key, hits) of the map into d_keys / d_hits (cap entries each; d_hits may be null: the counts then stay in scratch).
static int occ_fetch_run(sbm_occ_map* map, unsigned long long* d_keys, unsigned* d_hits, size_t cap, size_t* count) {
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
    // second key array, second count array, and a first count array for the caller who wants no counts
    unsigned long long* kk[2] = {d_keys};
    unsigned* vv[2];
    HIPCHK(h, occ_sort_carve(h, n, &kk[1], &vv[1], &vv[0]));
    if (d_hits) vv[0] = d_hits;
    HIPCHK(h, h->occ.hist.grow((size_t)256 * tiles * 4, h->stream));
    unsigned* hist = h->occ.hist.as<unsigned>();
    HIPCHK(h, clk.mark(kOccBegin, h->stream));
    st = occ_compact_run(map, n, kk[0], vv[0]);
    if (st == SBM_OK) st = occ_sort_run(h, kk, vv, n, hist);
    if (st != SBM_OK) return st;
    HIPCHK(h, clk.mark(kOccEnd, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, clk.add(kOccFetch, kOccBegin, kOccEnd));
  }
  return c.overflow ? SBM_ERR_OCC_FULL : SBM_OK;
}

}  // namespace sbm
using namespace sbm;

// Sorted (key, payload) of the map into host memory, through the handle's staging
static int occ_fetch_host(sbm_occ_map* map, uint64_t* keys, uint32_t* hits, size_t cap, size_t* count) {
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
  unsigned* d_v;
  HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& cv) { d_k = cv.take<unsigned long long>(c.size); d_v = cv.take<unsigned>(c.size); }, occ_pad));
  st = occ_fetch_run(map, d_k, d_v, c.size, count);
  if (st != SBM_OK && st != SBM_ERR_OCC_FULL) return st;
  HIPCHK(h, hipMemcpyAsync(keys, d_k, *count * 8, hipMemcpyDeviceToHost, h->stream));
  if (hits) HIPCHK(h, hipMemcpyAsync(hits, d_v, *count * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return st;
}

extern "C" {

void sbm_occ_params_default(sbm_occ_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->resolution = 0.1;
  p->range_max = 5.0f;
  p->tree_depth = 16;
}

int sbm_occ_params_validate(const sbm_occ_params* p) {
  if (!p) return SBM_ERR_NULL;
  if (!std::isfinite(p->resolution) || !(p->resolution > 0.) || !std::isfinite(1. / p->resolution)) return SBM_ERR_SIZE;
  if (std::isnan(p->range_max) || p->range_max < 0.f) return SBM_ERR_SIZE;
  if (p->tree_depth != 16) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

int sbm_occ_create(sbm_handle* h, const sbm_occ_params* p, size_t capacity, sbm_occ_map** out) {
  if (!h || !p || !out) return SBM_ERR_NULL;
  *out = nullptr;
  int st = sbm_occ_params_validate(p);
  if (st != SBM_OK) return st;
  if (capacity < 1) return SBM_ERR_SIZE;
  if (capacity > kOccMaxCapacity) return SBM_ERR_UNSUPPORTED;
  sbm_occ_map* map = new (std::nothrow) sbm_occ_map();
  if (!map) return SBM_ERR_NOMEM;
  memset(map, 0, sizeof(*map));
  map->h = h;
  map->p = *p;
  map->capacity = capacity;
  map->slots = 2;
  while ((size_t)map->slots < 2 * capacity) map->slots <<= 1;
  for (int i = 0; i < 3; i++) map->bbx_min_key[i] = map->bbx_max_key[i] = 32768;   // the keys of the box's two points, (0, 0, 0)
  DeviceScope dscope(h->device);
  hipError_t e = dscope.enter();
  if (e == hipSuccess) e = map->keys.grow((size_t)map->slots * 8, h->stream);
  if (e == hipSuccess) e = map->hits.grow((size_t)map->slots * 4, h->stream);
  if (e == hipSuccess) e = map->ctr.grow(sizeof(OccCounters), h->stream);
  st = SBM_OK;
  if (e != hipSuccess) {
    h->last_hip = (int)e;
    st = e == hipErrorOutOfMemory ? SBM_ERR_NOMEM : SBM_ERR_HIP;
  }
  if (st == SBM_OK) st = occ_clear(map);
  if (st != SBM_OK) {
    release_all(*map);
    delete map;
    return st;
  }
  *out = map;
  return SBM_OK;
}

void sbm_occ_destroy(sbm_occ_map* map) {
  if (!map) return;
  DeviceScope dscope(map->h->device);
  dscope.enter();
  hipStreamSynchronize(map->h->stream);
  release_all(*map);
  delete map;
}

int sbm_occ_reset(sbm_occ_map* map) {
  if (!map) return SBM_ERR_NULL;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_clear(map);
}

int sbm_occ_insert_device(sbm_occ_map* map, int n, const void* d_disp, int width, int height, int scale,
                          const sbm_stereo_model* model, const float* poses, int sync) {
  const int st = occ_check_insert(map, n, d_disp, width, height, scale, model, poses);
  if (st != SBM_OK) return st;
  if ((uintptr_t)d_disp & 1 || map->mode == kOccModeLogOdds || map->use_bbx || map->detect) return SBM_ERR_UNSUPPORTED;
  if (map->stamp.p) return SBM_ERR_UNSUPPORTED;   // stamp words belong to a log-odds map, also after sbm_occ_reset has cleared the mode
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  map->mode = kOccModeHits;
  return occ_insert_run(map, n, (const int16_t*)d_disp, width, height, scale, model, poses, sync);
}

int sbm_occ_insert(sbm_occ_map* map, int n, const int16_t* disp, int width, int height, int scale, const sbm_stereo_model* model,
                   const float* poses) {
  const int st = occ_check_insert(map, n, disp, width, height, scale, model, poses);
  if (st != SBM_OK) return st;
  if (map->mode == kOccModeLogOdds || map->use_bbx || map->detect) return SBM_ERR_UNSUPPORTED;
  if (map->stamp.p) return SBM_ERR_UNSUPPORTED;   // stamp words belong to a log-odds map, also after sbm_occ_reset has cleared the mode
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  const size_t bytes = (size_t)n * width * height * sizeof(int16_t);
  HIPCHK(h, h->occ.io.grow(bytes, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->occ.io.p, disp, bytes, hipMemcpyHostToDevice, h->stream));
  map->mode = kOccModeHits;
  return occ_insert_run(map, n, h->occ.io.as<int16_t>(), width, height, scale, model, poses, 1);
}

int sbm_occ_size(sbm_occ_map* map, size_t* size) {
  if (!map || !size) return SBM_ERR_NULL;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  OccCounters c;
  const int st = occ_read_counters(map, &c);
  if (st == SBM_OK) *size = c.size;
  return st;
}

int sbm_occ_overflow(sbm_occ_map* map, uint64_t* overflow) {
  if (!map || !overflow) return SBM_ERR_NULL;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  OccCounters c;
  const int st = occ_read_counters(map, &c);
  if (st == SBM_OK) *overflow = c.overflow;
  return st;
}

int sbm_occ_fetch_device(sbm_occ_map* map, void* d_keys, void* d_hits, size_t cap, size_t* count) {
  if (!map || !count || (cap > 0 && !d_keys)) return SBM_ERR_NULL;
  if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_hits & 3) || map->mode == kOccModeLogOdds) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_fetch_run(map, (unsigned long long*)d_keys, (unsigned*)d_hits, cap, count);
}

int sbm_occ_fetch(sbm_occ_map* map, uint64_t* keys, uint32_t* hits, size_t cap, size_t* count) {
  if (!map || !count || (cap > 0 && !keys)) return SBM_ERR_NULL;
  if (map->mode == kOccModeLogOdds) return SBM_ERR_UNSUPPORTED;
  return occ_fetch_host(map, keys, hits, cap, count);
}

int sbm_occ_fetch_logodds_device(sbm_occ_map* map, void* d_keys, void* d_logodds, size_t cap, size_t* count) {
  if (!map || !count || (cap > 0 && !d_keys)) return SBM_ERR_NULL;
  if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_logodds & 3)) return SBM_ERR_UNSUPPORTED;
  if (map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_fetch_run(map, (unsigned long long*)d_keys, (unsigned*)d_logodds, cap, count);   // the float's bits are the payload
}

int sbm_occ_fetch_logodds(sbm_occ_map* map, uint64_t* keys, float* logodds, size_t cap, size_t* count) {
  if (!map || !count || (cap > 0 && !keys)) return SBM_ERR_NULL;
  if (map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  return occ_fetch_host(map, keys, (uint32_t*)logodds, cap, count);
}

}  // extern "C"
