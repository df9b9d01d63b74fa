// sbm_occupancy.hip -- the occupancy voxel map of the reference's buildOccupancyGridMap (src/slam/src/core/main.cpp:495-561)
// as a device-side set of octomap keys, and the host writer of the octomap binary stream.  gfx950.
//
// include/sbm.h ("occupancy map: buildOccupancyGridMap") states the arithmetic; the point functions are those of
// sbm_consume.hip (sbm_consume_math.h). Nothing here contracts a multiply-add (the pragma below and -ffp-contract=off).
//
//   occ_insert_kernel   one thread per pixel: disparity -> point -> two transforms -> gate -> key; the wavefront then reduces
//                       its 64 keys to distinct leaders with lane counts (ballot + readlane over the distinct values) and only
//                       the leaders touch the table: a 64-bit compare-and-swap on the key slot, an atomic add of the lane count.
//   occ_rays_*_kernel   the log-odds mode, octomap's insertPointCloud per scan: one lane per ray walks computeRayKeys' 3-D DDA in
//                       registers and ORs "free" / "occupied this scan" into the flag word of every cell's slot; the lane whose OR
//                       found the word clear appends the slot to the scan's touched list. occ_rays_apply_kernel then gives every
//                       touched slot its ONE update (occupied wins) and clears the flags.
//   occ_search / occ_cast_rays / occ_cast_view   the read side, octomap's search and castRay: one lane per point, ray or pixel
//                       probes the table with plain loads and walks castRay's DDA in registers; the map is not written.
//   occ_load_kernel     readBinary: the host parses the pruned tree of a .bt stream, and one lane per depth-16 voxel finds its leaf
//                       in the prefix array of the leaf volumes, de-interleaves its Morton code and claims its slot.
//   occ_compact_kernel  occupied slots -> dense (key, hits) arrays, one atomic per wavefront.
//   occ_hist / occ_scan / occ_scatter   one 8-bit pass of an LSD radix sort: digit counts per tile, an exclusive scan of the
//                       digit-major count table, and a stable scatter (one wavefront per tile walks it 64 keys at a time and
//                       ranks equal digits by ballots).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "sbm_consume_math.h"
#include "sbm_handle.h"

struct sbm_occ_map {
  sbm_handle* h;
  sbm_occ_params p;
  size_t capacity;           // voxels the caller asked for
  uint32_t slots;            // power of two >= 2 * capacity
  unsigned scan;             // log-odds mode: scans applied since the last clear
  int mode;                  // fixed by the first insert after create or reset: kOccModeNone, kOccModeHits, kOccModeLogOdds
  sbm::DevBuf keys, hits;    // the table; in the log-odds mode a slot's `hits` word is its float log-odds
  sbm::DevBuf ctr;           // OccCounters
  sbm::DevBuf flags, touched;   // log-odds mode only, from its first insert: per slot the flag word of the running scan, and the
                                // slots that scan touched (4 B per slot each)
  template <class F> void each(F f) { f(keys); f(hits); f(ctr); f(flags); f(touched); }
};

namespace sbm {

#pragma clang fp contract(off)

constexpr unsigned long long kOccEmpty = ~0ull;
constexpr int kOccChunk = 64;        // planes per insert launch: their poses travel as kernel arguments (3 KiB)
constexpr uint32_t kOccMaxProbe = 1024;
constexpr int kOccTile = 1024;       // keys per workgroup of a radix pass
constexpr size_t kOccMaxCapacity = (size_t)1 << 30;

enum { kOccModeNone, kOccModeHits, kOccModeLogOdds };
constexpr int kOccMaxSteps = 3 * 65536;   // of one ray: each step moves one key by one on one axis
constexpr unsigned kOccFree = 1, kOccOccupied = 2;   // flag word of a slot within one scan

struct OccCounters {
  unsigned long long overflow;   // points (log-odds mode: cells) that found the table full
  unsigned size;                 // occupied slots
  unsigned cursor;               // compaction cursor of a fetch
  unsigned touched[2];           // log-odds mode: slots the running scan has touched, in [scan & 1]; the other is zero
};

struct OccPoses { float t[kOccChunk][12]; };

struct OccGeom {
  int W, H, scale;
  float range_max_sqrd;          // range_max * range_max, formed in float on the host as main.cpp:501 does
  double factor;                 // 1. / resolution
  uint32_t mask, max_probe;
};

__device__ __forceinline__ uint32_t occ_hash(unsigned long long key, uint32_t mask) {
  return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// OcTreeBaseImpl.hxx:310-321 on one axis: floor in double, then 0 <= floor + 32768 < 65536. NaN fails both comparisons, and so
// does every value whose floor fits no int (the reference's cast gives INT_MIN there, which its range test rejects).
__device__ __forceinline__ bool occ_axis(double factor, float coord, unsigned* k) {
#pragma clang fp contract(off)
  const double f = floor(factor * (double)coord);
  if (!(f >= -32768.0 && f < 32768.0)) return false;
  *k = (unsigned)((int)f + 32768);
  return true;
}

// main.cpp:529-539 on pixel i of a plane: false where the reference skips the pixel, else the point after both transforms
__device__ __forceinline__ bool occ_world_point(const int16_t* __restrict__ plane, int i, const OccGeom& g, const sbm_stereo_model& m,
                                                const float* pose, Pt3* out) {
#pragma clang fp contract(off)
  const int r = i / g.W, c = i % g.W;
  const float d = (float)plane[i] / 16.0f;       // main.cpp:529
  if (!(d > 0)) return false;
  Pt3 p = project_disparity((float)(c * g.scale), (float)(r * g.scale), d, m);
  if (!finite3(p)) return false;
  if (m.has_local) p = transform_point(p, m.local);
  *out = transform_point(p, pose);
  return true;
}

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
      key = (unsigned long long)k0 << 32 | (unsigned long long)k1 << 16 | k2;
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
  uint32_t slot = occ_hash(key, g.mask);
  for (uint32_t probe = 0; probe < g.max_probe; probe++, slot = (slot + 1) & g.mask) {
    unsigned long long cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kOccEmpty) {
      cur = atomicCAS(&keys[slot], kOccEmpty, key);
      if (cur == kOccEmpty) {
        atomicAdd(&ctr->size, 1u);
        cur = key;
      }
    }
    if (cur == key) {
      atomicAdd(&hits[slot], count);
      return;
    }
  }
  atomicAdd(&ctr->overflow, (unsigned long long)count);
}

// ---- log-odds mode: insertPointCloud (OccupancyOcTreeBase.hxx:86-102, computeUpdate :169-270) ------------------------------
struct OccRay {                 // one call's constants
  double max_range;             // < 0: no limit
  double resolution, factor;    // factor = 1. / resolution
  float hit, miss, cmin, cmax;  // log-odds
  uint32_t mask, max_probe, slots;
  uint32_t parity;              // which of OccCounters::touched counts this scan
};

struct OccPose { float t[12]; };     // the plane form's pose; the cloud form passes its origin in t[3], t[7], t[11]

struct OccTable {
  unsigned long long* keys;
  float* logodds;
  unsigned* flags;
  unsigned* touched;
  OccCounters* ctr;
};

// The whole wavefront calls this once per step (have: this lane has a cell). Finds or claims the cell's slot and ORs `bit` into
// its flag word -- after reading it: thousands of rays share their first cells, and a set bit needs no atomic. The lanes whose OR
// found the word clear append their slots to the scan's touched list, one atomic on the list's counter per wavefront. A cell
// that finds no slot within the probe bound is counted as overflow.
__device__ __forceinline__ void occ_mark_cell(unsigned long long key, unsigned bit, bool have, const OccRay& g, const OccTable& t) {
  bool fresh = false;
  uint32_t slot = 0;
  if (have) {
    bool found = false;
    slot = occ_hash(key, g.mask);
    for (uint32_t probe = 0; probe < g.max_probe; probe++, slot = (slot + 1) & g.mask) {
      unsigned long long cur = __hip_atomic_load(&t.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kOccEmpty) {
        cur = atomicCAS(&t.keys[slot], kOccEmpty, key);
        if (cur == kOccEmpty) {
          atomicAdd(&t.ctr->size, 1u);
          cur = key;
        }
      }
      if (cur == key) {
        found = true;
        break;
      }
    }
    if (found) {
      unsigned old = __hip_atomic_load(&t.flags[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (!(old & bit)) {
        old = atomicOr(&t.flags[slot], bit);
        fresh = old == 0;
      }
    } else {
      atomicAdd(&t.ctr->overflow, 1ull);
    }
  }
  const unsigned long long mine = __ballot(fresh);
  if (!mine) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mine) - 1;
  unsigned base = 0;
  if (lane == leader) base = atomicAdd(&t.ctr->touched[g.parity], (unsigned)__popcll(mine));
  base = __builtin_amdgcn_readlane(base, leader);
  if (!fresh) return;
  const uint32_t at = base + __popcll(mine & ((1ull << lane) - 1));
  if (at < g.slots) t.touched[at] = slot;   // a slot is appended once per scan: the list of `slots` entries always has room
}

// One axis of computeRayKeys' initialisation (OcTreeBaseImpl.hxx:577-596)
__device__ __forceinline__ void occ_ray_axis(float dir, unsigned key, float origin, double resolution, int* step, double* tmax,
                                             double* tdelta) {
#pragma clang fp contract(off)
  *step = dir > 0.0f ? 1 : dir < 0.0f ? -1 : 0;
  *tmax = *tdelta = 1.7976931348623157e308;   // std::numeric_limits<double>::max()
  if (*step) {
    double border = ((double)((int)key - 32768) + 0.5) * resolution;   // keyToCoord
    border += (double)(float)((double)*step * resolution * 0.5);
    *tmax = (border - (double)origin) / (double)dir;
    *tdelta = resolution / fabs((double)dir);
  }
}

// One ray of computeUpdate, by the whole wavefront (valid: this lane has a point): the range gate, the truncated end beyond it,
// computeRayKeys (OcTreeBaseImpl.hxx:542-648) with every cell marked free as the DDA reaches it, and the end point marked occupied.
__device__ __forceinline__ void occ_cast_ray(bool valid, Pt3 p, const float* o, const OccRay& g, const OccTable& t) {
#pragma clang fp contract(off)
  bool walking = false, ends = false;
  unsigned c0 = 0, c1 = 0, c2 = 0, e0 = 0, e1 = 0, e2 = 0;
  int s0 = 0, s1 = 0, s2 = 0;
  double t0 = 0., t1 = 0., t2 = 0., d0 = 0., d1 = 0., d2 = 0., length = 0.;
  if (valid && finite3(p)) {
    const float ox = o[0], oy = o[1], oz = o[2];
    float vx = p.x - ox, vy = p.y - oy, vz = p.z - oz;
    const double n = __dsqrt_rn((double)(vx * vx + vy * vy + vz * vz));   // Vector3::norm: the sum in float
    const bool within = g.max_range < 0.0 || n <= g.max_range;
    Pt3 end = p;
    if (!within) {                      // (p - origin).normalized() * (float)maxrange from the origin
      if (n > 0) {
        const float len = (float)n;
        vx /= len;
        vy /= len;
        vz /= len;
      }
      const float r = (float)g.max_range;
      end.x = ox + vx * r;
      end.y = oy + vy * r;
      end.z = oz + vz * r;
    }
    const bool end_ok = occ_axis(g.factor, end.x, &e0) && occ_axis(g.factor, end.y, &e1) && occ_axis(g.factor, end.z, &e2);
    ends = within && end_ok;
    if (end_ok && occ_axis(g.factor, ox, &c0) && occ_axis(g.factor, oy, &c1) && occ_axis(g.factor, oz, &c2) &&
        !(c0 == e0 && c1 == e1 && c2 == e2)) {
      walking = true;
      float dx = end.x - ox, dy = end.y - oy, dz = end.z - oz;
      const float len = (float)__dsqrt_rn((double)(dx * dx + dy * dy + dz * dz));
      dx /= len;
      dy /= len;
      dz /= len;
      length = (double)len;
      occ_ray_axis(dx, c0, ox, g.resolution, &s0, &t0, &d0);
      occ_ray_axis(dy, c1, oy, g.resolution, &s1, &t1, &d1);
      occ_ray_axis(dz, c2, oz, g.resolution, &s2, &t2, &d2);
    }
  }
  // The origin cell first, then one cell per step until the end cell's key or the ray's length is reached; the end cell is not
  // part of the ray. The step count is bounded whatever the input: the wavefront leaves the loop when its last lane has.
  int steps = 0;
  while (__ballot(walking)) {
    occ_mark_cell((unsigned long long)c0 << 32 | (unsigned long long)c1 << 16 | c2, kOccFree, walking, g, t);
    if (walking) {
      const int dim = t0 < t1 ? (t0 < t2 ? 0 : 2) : (t1 < t2 ? 1 : 2);   // the strict < of the reference: ties go to the later axis
      if (dim == 0) {
        c0 = (c0 + s0) & 0xFFFF;
        t0 += d0;
      } else if (dim == 1) {
        c1 = (c1 + s1) & 0xFFFF;
        t1 += d1;
      } else {
        c2 = (c2 + s2) & 0xFFFF;
        t2 += d2;
      }
      if ((c0 == e0 && c1 == e1 && c2 == e2) || fmin(fmin(t0, t1), t2) > length || ++steps >= kOccMaxSteps) walking = false;
    }
  }
  occ_mark_cell((unsigned long long)e0 << 32 | (unsigned long long)e1 << 16 | e2, kOccOccupied, ends, g, t);
}

// mark, cloud form: one lane per point of d_xyz
__global__ void __launch_bounds__(256) occ_rays_mark_cloud_kernel(const float* __restrict__ xyz, size_t n, OccPose origin, OccRay g,
                                                                   OccTable t) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  Pt3 p = nan3();
  if (i < n) p = Pt3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  const float o[3] = {origin.t[3], origin.t[7], origin.t[11]};
  occ_cast_ray(i < n, p, o, g, t);
}

// mark, plane form: one lane per pixel of one plane, through the front half of the hit insert; the origin is the pose's translation
__global__ void __launch_bounds__(256) occ_rays_mark_plane_kernel(const int16_t* __restrict__ plane, OccGeom pg, sbm_stereo_model m,
                                                                   OccPose pose, OccRay g, OccTable t) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  Pt3 p = nan3();
  const bool valid = i < pg.W * pg.H && occ_world_point(plane, i, pg, m, pose.t, &p);
  const float o[3] = {pose.t[3], pose.t[7], pose.t[11]};
  occ_cast_ray(valid, p, o, g, t);
}

// apply: every slot the scan touched gets its one update (updateNodeLogOdds, OccupancyOcTreeBase.hxx:1097-1106; an absent voxel
// starts at 0, which is what a fresh slot holds), occupied before free, and its flag word is cleared for the next scan. The
// early return of updateNode for a leaf at its clamp gives what the clamp gives. No atomics: a slot is in the list once. The
// two counts of OccCounters::touched take turns, so that no scan needs a memset between its two launches and the next scan's.
__global__ void __launch_bounds__(256) occ_rays_apply_kernel(OccRay g, OccTable t) {
#pragma clang fp contract(off)
  const uint32_t n = min(t.ctr->touched[g.parity], g.slots);
  if (blockIdx.x == 0 && threadIdx.x == 0) t.ctr->touched[g.parity ^ 1] = 0;   // the next scan's count; nobody reads it now
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t slot = t.touched[i];
    if (slot >= g.slots) continue;
    float v = t.logodds[slot] + ((t.flags[slot] & kOccOccupied) ? g.hit : g.miss);
    if (v < g.cmin) v = g.cmin;
    else if (v > g.cmax) v = g.cmax;
    t.logodds[slot] = v;
    t.flags[slot] = 0;
  }
}

__global__ void __launch_bounds__(256) occ_compact_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ hits,
                                                           uint32_t slots, uint32_t cap, unsigned long long* __restrict__ out_keys,
                                                           unsigned* __restrict__ out_hits, OccCounters* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long k = i < slots ? keys[i] : kOccEmpty;
  const unsigned long long live = __ballot(k != kOccEmpty);
  if (!live) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)live) - 1;
  unsigned base = 0;
  if (lane == leader) base = atomicAdd(&ctr->cursor, (unsigned)__popcll(live));
  base = __builtin_amdgcn_readlane(base, leader);
  if (k == kOccEmpty) return;
  const uint32_t o = base + __popcll(live & ((1ull << lane) - 1));
  if (o >= cap) return;   // the host sized the outputs from ctr->size; a slot claimed since then has no room
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

static int occ_read_counters(sbm_occ_map* map, OccCounters* c) {
  sbm_handle* h = map->h;
  HIPCHK(h, hipMemcpyAsync(c, map->ctr.p, sizeof(*c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

static int occ_clear(sbm_occ_map* map) {
  sbm_handle* h = map->h;
  HIPCHK(h, hipMemsetAsync(map->keys.p, 0xFF, (size_t)map->slots * 8, h->stream));
  HIPCHK(h, hipMemsetAsync(map->hits.p, 0, (size_t)map->slots * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(map->ctr.p, 0, sizeof(OccCounters), h->stream));
  if (map->flags.p) HIPCHK(h, hipMemsetAsync(map->flags.p, 0, (size_t)map->slots * 4, h->stream));
  map->mode = kOccModeNone;
  map->scan = 0;
  return SBM_OK;
}

static int occ_check_insert(const sbm_occ_map* map, int n, const void* disp, int width, int height, int scale,
                            const sbm_stereo_model* model, const float* poses) {
  if (!map || !disp || !model || !poses) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width <= 0 || height <= 0 || scale <= 0) return SBM_ERR_SIZE;
  if ((size_t)width * height > ((size_t)1 << 30) || (size_t)width * scale > ((size_t)1 << 24) || (size_t)height * scale > ((size_t)1 << 24))
    return SBM_ERR_UNSUPPORTED;   // pixel coordinates stay exact in float, the pixel index in int
  return SBM_OK;
}

// Stage times: an insert and a fetch are separate calls that share the clock's two marks, and each keeps the other's last time.
enum OccStage { kOccInsert, kOccFetch, kOccRaysMark, kOccRaysApply, kOccSearch, kOccCast, kOccTreeBuild, kOccTreeQuery, kOccLoad, kOccStageCount };
enum OccMark { kOccBegin, kOccEnd, kOccMid, kOccMarkCount };
static const char* const kOccNames[] = {"occ_insert", "occ_fetch", "occ_rays_mark", "occ_rays_apply", "occ_search", "occ_cast",
                                        "occ_tree_build", "occ_tree_query", "occ_load"};
StageTable occ_stages() { return stage_table<kOccStageCount, kOccMarkCount>(kOccNames); }

// A call begins: it times stages a and b (the same for one) from zero and keeps the last times of the family's other stages.
static hipError_t occ_clock_start(sbm_handle* h, int a, int b) {
  StageClock& clk = h->occ.clock;
  float keep[kOccStageCount];
  for (int i = 0; i < kOccStageCount; i++) keep[i] = clk.ms[i];
  const hipError_t e = clk.start(occ_stages(), h->profiling != 0);
  for (int i = 0; i < kOccStageCount; i++)
    if (clk.on && i != a && i != b) clk.ms[i] = keep[i];
  return e;
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
  g.mask = map->slots - 1;
  g.max_probe = std::min(map->slots, kOccMaxProbe);
  const size_t plane = (size_t)W * H;
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  for (int c0 = 0; c0 < n; c0 += kOccChunk) {
    const int m = std::min(kOccChunk, n - c0);
    OccPoses ps;
    memset(&ps, 0, sizeof(ps));
    memcpy(ps.t, poses + (size_t)12 * c0, sizeof(float) * 12 * m);
    hipLaunchKernelGGL(occ_insert_kernel, dim3((unsigned)((plane + 255) / 256), m), dim3(256), 0, h->stream, d_disp + plane * c0, g,
                       *model, ps, map->keys.as<unsigned long long>(), map->hits.as<unsigned>(), map->ctr.as<OccCounters>());
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(kOccInsert, kOccBegin, kOccEnd));
  if (!sync && !clk.on) return SBM_OK;
  OccCounters c;
  const int st = occ_read_counters(map, &c);
  if (st != SBM_OK) return st;
  return c.overflow ? SBM_ERR_OCC_FULL : SBM_OK;
}

// LSD radix sort of n (48-bit key, 32-bit payload) pairs, 8 bits per pass: from kk[0] / vv[0] through kk[1] / vv[1], and the
// even number of passes ends in kk[0] / vv[0]. hist: 256 counts per tile of kOccTile keys.
static int occ_sort_run(sbm_handle* h, unsigned long long* const kk[2], unsigned* const vv[2], uint32_t n, unsigned* hist) {
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
    // second key array, second count array, and a first count array when the caller wants no counts
    const size_t kb = ((size_t)n * 8 + 255) & ~(size_t)255, vb = ((size_t)n * 4 + 255) & ~(size_t)255;
    HIPCHK(h, h->occ.sort.grow(kb + 2 * vb, h->stream));
    HIPCHK(h, h->occ.hist.grow((size_t)256 * tiles * 4, h->stream));
    unsigned long long* kk[2] = {d_keys, h->occ.sort.as<unsigned long long>()};
    unsigned* vv[2] = {d_hits ? d_hits : (unsigned*)((char*)h->occ.sort.p + kb + vb), (unsigned*)((char*)h->occ.sort.p + kb)};
    unsigned* hist = h->occ.hist.as<unsigned>();
    HIPCHK(h, clk.mark(kOccBegin, h->stream));
    HIPCHK(h, hipMemsetAsync((char*)map->ctr.p + offsetof(OccCounters, cursor), 0, sizeof(unsigned), h->stream));
    hipLaunchKernelGGL(occ_compact_kernel, dim3((map->slots + 255) / 256), dim3(256), 0, h->stream, map->keys.as<unsigned long long>(),
                       map->hits.as<unsigned>(), map->slots, n, kk[0], vv[0], map->ctr.as<OccCounters>());
    HIPCHK(h, hipGetLastError());
    st = occ_sort_run(h, kk, vv, n, hist);
    if (st != SBM_OK) return st;
    HIPCHK(h, clk.mark(kOccEnd, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, clk.add(kOccFetch, kOccBegin, kOccEnd));
  }
  return c.overflow ? SBM_ERR_OCC_FULL : SBM_OK;
}

// ---- log-odds mode, host side ----------------------------------------------------------------------------------------------
static float occ_logodds(double p) { return (float)log(p / (1. - p)); }   // octomap_utils.h

static int occ_ray_params_check(const sbm_occ_ray_params* p) {
  if (!p) return SBM_ERR_NULL;
  const double prob[5] = {p->prob_hit, p->prob_miss, p->clamp_min, p->clamp_max, p->occupancy_thres};
  for (double v : prob)
    if (!(v > 0. && v < 1.)) return SBM_ERR_SIZE;   // NaN fails both
  if (p->prob_hit < 0.5 || p->prob_miss > 0.5 || !(p->clamp_min < p->clamp_max) || std::isnan(p->max_range)) return SBM_ERR_SIZE;
  return SBM_OK;
}

// What the log-odds mode keeps beside the table, 8 B per slot: the flag words, clear between scans, and the touched list
static int occ_logodds_alloc(sbm_occ_map* map) {
  sbm_handle* h = map->h;
  if (!map->flags.p) {
    HIPCHK(h, map->flags.grow((size_t)map->slots * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(map->flags.p, 0, (size_t)map->slots * 4, h->stream));
  }
  HIPCHK(h, map->touched.grow((size_t)map->slots * 4, h->stream));
  return SBM_OK;
}

// The first log-odds insert after create or reset allocates the flag words and the touched list and fixes the mode.
static int occ_rays_begin(sbm_occ_map* map, const sbm_occ_ray_params* p, OccRay* g, OccTable* t) {
  if (map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  const int st = occ_logodds_alloc(map);
  if (st != SBM_OK) return st;
  map->mode = kOccModeLogOdds;
  g->max_range = p->max_range;
  g->resolution = map->p.resolution;
  g->factor = 1. / map->p.resolution;
  g->hit = occ_logodds(p->prob_hit);
  g->miss = occ_logodds(p->prob_miss);
  g->cmin = occ_logodds(p->clamp_min);
  g->cmax = occ_logodds(p->clamp_max);
  g->mask = map->slots - 1;
  g->max_probe = std::min(map->slots, kOccMaxProbe);
  g->slots = map->slots;
  g->parity = 0;
  t->keys = map->keys.as<unsigned long long>();
  t->logodds = map->hits.as<float>();
  t->flags = map->flags.as<unsigned>();
  t->touched = map->touched.as<unsigned>();
  t->ctr = map->ctr.as<OccCounters>();
  return SBM_OK;
}

// One scan: `mark` launches its mark kernel; the apply launch follows in stream order.
template <class Mark> static int occ_rays_scan(sbm_occ_map* map, OccRay& g, const OccTable& t, Mark mark) {
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  g.parity = map->scan & 1;
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  mark();
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, clk.mark(kOccMid, h->stream));
  hipLaunchKernelGGL(occ_rays_apply_kernel, dim3(std::min((map->slots + 255) / 256, 1024u)), dim3(256), 0, h->stream, g, t);
  HIPCHK(h, hipGetLastError());
  map->scan++;
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(kOccRaysMark, kOccBegin, kOccMid));
  HIPCHK(h, clk.add(kOccRaysApply, kOccMid, kOccEnd));
  return SBM_OK;
}

static int occ_rays_end(sbm_occ_map* map, int sync) {
  if (!sync && !map->h->occ.clock.on) return SBM_OK;
  OccCounters c;
  const int st = occ_read_counters(map, &c);
  if (st != SBM_OK) return st;
  return c.overflow ? SBM_ERR_OCC_FULL : SBM_OK;
}

static int occ_check_cloud(const sbm_occ_map* map, size_t n, const void* xyz, const float* origin, const sbm_occ_ray_params* p) {
  if (!map || !origin || !p || (n > 0 && !xyz)) return SBM_ERR_NULL;
  const int st = occ_ray_params_check(p);
  if (st != SBM_OK) return st;
  if (n > ((size_t)1 << 30)) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

static int occ_cloud_run(sbm_occ_map* map, size_t n, const float* d_xyz, const float* origin, const sbm_occ_ray_params* p, int sync) {
  sbm_handle* h = map->h;
  OccRay g;
  OccTable t;
  int st = occ_rays_begin(map, p, &g, &t);
  if (st != SBM_OK) return st;
  HIPCHK(h, occ_clock_start(h, kOccRaysMark, kOccRaysApply));
  if (n) {
    OccPose o;
    memset(&o, 0, sizeof(o));
    o.t[3] = origin[0], o.t[7] = origin[1], o.t[11] = origin[2];
    st = occ_rays_scan(map, g, t, [&] {
      hipLaunchKernelGGL(occ_rays_mark_cloud_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, d_xyz, n, o, g, t);
    });
    if (st != SBM_OK) return st;
  }
  return occ_rays_end(map, sync);
}

static int occ_planes_run(sbm_occ_map* map, int n, const int16_t* d_disp, int W, int H, int scale, const sbm_stereo_model* model,
                          const float* poses, const sbm_occ_ray_params* p, int sync) {
  sbm_handle* h = map->h;
  OccRay g;
  OccTable t;
  int st = occ_rays_begin(map, p, &g, &t);
  if (st != SBM_OK) return st;
  HIPCHK(h, occ_clock_start(h, kOccRaysMark, kOccRaysApply));
  OccGeom pg;
  memset(&pg, 0, sizeof(pg));
  pg.W = W;
  pg.H = H;
  pg.scale = scale;
  const size_t plane = (size_t)W * H;
  for (int i = 0; i < n; i++) {   // plane i is scan i: its launches follow those of plane i - 1 in stream order
    OccPose pose;
    memcpy(pose.t, poses + (size_t)12 * i, sizeof(pose.t));
    st = occ_rays_scan(map, g, t, [&] {
      hipLaunchKernelGGL(occ_rays_mark_plane_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, h->stream, d_disp + plane * i,
                         pg, *model, pose, g, t);
    });
    if (st != SBM_OK) return st;
  }
  return occ_rays_end(map, sync);
}

// ---- queries: search and castRay (OcTreeBaseImpl.hxx:408-470, OccupancyOcTreeBase.hxx:645-765) ------------------------------
// Read-only and stream-ordered after the inserts: plain cached loads, no atomics. One lane per point, ray or pixel; a lane that
// has its answer leaves its loop, nothing needs the whole wavefront.
#ifndef SBM_OCC_VIEW_TILED
#define SBM_OCC_VIEW_TILED 1   // 0 builds the row order of the view kernel, for tools/bench_occupancy_query.py to time
#endif
constexpr bool kOccViewTiled = SBM_OCC_VIEW_TILED != 0;   // a wavefront covers an 8 x 8 pixel tile, not 64 pixels of a row

struct OccQuery {               // one call's constants
  double max_range;             // <= 0: no limit
  double resolution, factor;
  float thres;                  // log-odds mode: occupied iff logodds >= thres
  int ignore_unknown, mode;
  uint32_t mask, max_probe;
  const unsigned long long* keys;
  const unsigned* vals;
};

struct OccView {
  int W, H, scale, shared;      // shared (the ray form): every ray starts at origin
  float origin[3];
};

// The voxel's state and its slot's 32-bit word: a walk from the key's hash to the key, an empty slot or the probe bound
__device__ __forceinline__ int occ_lookup(unsigned long long key, const OccQuery& g, unsigned* value) {
  uint32_t slot = occ_hash(key, g.mask);
  for (uint32_t probe = 0; probe < g.max_probe; probe++, slot = (slot + 1) & g.mask) {
    const unsigned long long cur = g.keys[slot];
    if (cur == key) {
      const unsigned v = g.vals[slot];
      *value = v;
      if (g.mode == kOccModeHits) return SBM_OCC_CELL_OCCUPIED;
      return __uint_as_float(v) >= g.thres ? SBM_OCC_CELL_OCCUPIED : SBM_OCC_CELL_FREE;   // isNodeOccupied
    }
    if (cur == kOccEmpty) break;
  }
  *value = g.mode == kOccModeLogOdds ? 0x7FC00000u : 0u;
  return SBM_OCC_CELL_UNKNOWN;
}

__device__ __forceinline__ float occ_key_coord(unsigned key, double resolution) {   // keyToCoord, then point3d's float
#pragma clang fp contract(off)
  return (float)(((double)((int)key - 32768) + 0.5) * resolution);
}

// One axis of castRay's initialisation (OccupancyOcTreeBase.hxx:677-696): the border's half cell is added in DOUBLE here, where
// computeRayKeys (occ_ray_axis) rounds it to float first
__device__ __forceinline__ void occ_query_axis(float dir, unsigned key, float origin, double resolution, int* step, double* tmax,
                                               double* tdelta) {
#pragma clang fp contract(off)
  *step = dir > 0.0f ? 1 : dir < 0.0f ? -1 : 0;
  *tmax = *tdelta = 1.7976931348623157e308;
  if (*step) {
    double border = ((double)((int)key - 32768) + 0.5) * resolution;
    border += (double)*step * resolution * 0.5;
    *tmax = (border - (double)origin) / (double)dir;
    *tdelta = resolution / fabs((double)dir);
  }
}

// castRay, in the order of the source -> status, *end
__device__ __forceinline__ int occ_query_ray(Pt3 o, Pt3 d, const OccQuery& g, Pt3* end) {
#pragma clang fp contract(off)
  *end = nan3();
  unsigned c0, c1, c2, word;
  if (!(occ_axis(g.factor, o.x, &c0) && occ_axis(g.factor, o.y, &c1) && occ_axis(g.factor, o.z, &c2))) return SBM_OCC_RAY_NONE;
  int cell = occ_lookup((unsigned long long)c0 << 32 | (unsigned long long)c1 << 16 | c2, g, &word);
  if (cell == SBM_OCC_CELL_OCCUPIED || (cell == SBM_OCC_CELL_UNKNOWN && !g.ignore_unknown)) {
    *end = Pt3{occ_key_coord(c0, g.resolution), occ_key_coord(c1, g.resolution), occ_key_coord(c2, g.resolution)};
    return cell == SBM_OCC_CELL_OCCUPIED ? SBM_OCC_RAY_HIT : SBM_OCC_RAY_UNKNOWN;
  }
  const double len = __dsqrt_rn((double)(d.x * d.x + d.y * d.y + d.z * d.z));   // Vector3::normalized: the sum in float
  if (len > 0) {
    const float l = (float)len;
    d.x /= l;
    d.y /= l;
    d.z /= l;
  }
  int s0, s1, s2;
  double t0, t1, t2, d0, d1, d2;
  occ_query_axis(d.x, c0, o.x, g.resolution, &s0, &t0, &d0);
  occ_query_axis(d.y, c1, o.y, g.resolution, &s1, &t1, &d1);
  occ_query_axis(d.z, c2, o.z, g.resolution, &s2, &t2, &d2);
  if (!s0 && !s1 && !s2) return SBM_OCC_RAY_NONE;
  const bool ranged = g.max_range > 0.0;
  const double range_sq = g.max_range * g.max_range;
  for (int steps = 0; steps < kOccMaxSteps; steps++) {
    const int dim = t0 < t1 ? (t0 < t2 ? 0 : 2) : (t1 < t2 ? 1 : 2);
    const int s = dim == 0 ? s0 : dim == 1 ? s1 : s2;
    const unsigned c = dim == 0 ? c0 : dim == 1 ? c1 : c2;
    if ((s < 0 && c == 0) || (s > 0 && c == 65535)) break;   // the edge of the key space, tested before the advance
    if (dim == 0) {
      c0 += s0;
      t0 += d0;
    } else if (dim == 1) {
      c1 += s1;
      t1 += d1;
    } else {
      c2 += s2;
      t2 += d2;
    }
    const Pt3 e = Pt3{occ_key_coord(c0, g.resolution), occ_key_coord(c1, g.resolution), occ_key_coord(c2, g.resolution)};
    if (ranged) {
      const float ex = e.x - o.x, ey = e.y - o.y, ez = e.z - o.z;
      double dist = 0.0;
      dist += (double)(ex * ex);
      dist += (double)(ey * ey);
      dist += (double)(ez * ez);
      if (dist > range_sq) {
        *end = e;
        return SBM_OCC_RAY_RANGE;
      }
    }
    cell = occ_lookup((unsigned long long)c0 << 32 | (unsigned long long)c1 << 16 | c2, g, &word);
    if (cell == SBM_OCC_CELL_OCCUPIED || (cell == SBM_OCC_CELL_UNKNOWN && !g.ignore_unknown)) {
      *end = e;
      return cell == SBM_OCC_CELL_OCCUPIED ? SBM_OCC_RAY_HIT : SBM_OCC_RAY_UNKNOWN;
    }
  }
  *end = Pt3{occ_key_coord(c0, g.resolution), occ_key_coord(c1, g.resolution), occ_key_coord(c2, g.resolution)};
  return SBM_OCC_RAY_BOUNDS;
}

__global__ void __launch_bounds__(256) occ_search_kernel(const float* __restrict__ xyz, size_t n, OccQuery g, int* __restrict__ state,
                                                          unsigned* __restrict__ value) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned k0, k1, k2, word = g.mode == kOccModeLogOdds ? 0x7FC00000u : 0u;
  int st = SBM_OCC_CELL_OUT;
  if (occ_axis(g.factor, xyz[3 * i], &k0) && occ_axis(g.factor, xyz[3 * i + 1], &k1) && occ_axis(g.factor, xyz[3 * i + 2], &k2))
    st = occ_lookup((unsigned long long)k0 << 32 | (unsigned long long)k1 << 16 | k2, g, &word);
  state[i] = st;
  if (value) value[i] = word;
}

__global__ void __launch_bounds__(256) occ_cast_rays_kernel(const float* __restrict__ origins, const float* __restrict__ dirs, size_t n,
                                                             OccView v, OccQuery g, int* __restrict__ status, float* __restrict__ end) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Pt3 o = v.shared ? Pt3{v.origin[0], v.origin[1], v.origin[2]} : Pt3{origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]};
  Pt3 e;
  status[i] = occ_query_ray(o, Pt3{dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]}, g, &e);
  if (end) {
    end[3 * i] = e.x;
    end[3 * i + 1] = e.y;
    end[3 * i + 2] = e.z;
  }
}

// One ray per pixel of a virtual camera: a workgroup covers 32 x 8 pixels as four 8 x 8 tiles, one per wavefront (kOccViewTiled),
// or 256 consecutive pixels in row-major order.
__global__ void __launch_bounds__(256) occ_cast_view_kernel(OccView v, sbm_stereo_model m, OccPose pose, OccQuery g,
                                                             int* __restrict__ status, float* __restrict__ end) {
#pragma clang fp contract(off)
  int row, col;
  if (kOccViewTiled) {
    const int tiles_x = (v.W + 31) / 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    col = (int)(blockIdx.x % tiles_x) * 32 + wave * 8 + (lane & 7);
    row = (int)(blockIdx.x / tiles_x) * 8 + (lane >> 3);
    if (col >= v.W || row >= v.H) return;
  } else {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)v.W * v.H) return;
    row = (int)(i / v.W);
    col = (int)(i % v.W);
  }
  Pt3 q = Pt3{(float)(((double)(col * v.scale) - m.cx_l) / m.fx_l), (float)(((double)(row * v.scale) - m.cy_l) / m.fy_l), 1.0f};
  Pt3 o = Pt3{0.0f, 0.0f, 0.0f};
  if (m.has_local) {
    q = transform_point(q, m.local);
    o = transform_point(o, m.local);
  }
  q = transform_point(q, pose.t);
  o = transform_point(o, pose.t);
  Pt3 e;
  const size_t i = (size_t)row * v.W + col;
  status[i] = occ_query_ray(o, Pt3{q.x - o.x, q.y - o.y, q.z - o.z}, g, &e);
  if (end) {
    end[3 * i] = e.x;
    end[3 * i + 1] = e.y;
    end[3 * i + 2] = e.z;
  }
}

static void occ_query_begin(const sbm_occ_map* map, double max_range, float thres, int ignore_unknown, OccQuery* g) {
  g->max_range = max_range;
  g->resolution = map->p.resolution;
  g->factor = 1. / map->p.resolution;
  g->thres = thres;
  g->ignore_unknown = ignore_unknown != 0;
  g->mode = map->mode;
  g->mask = map->slots - 1;
  g->max_probe = std::min(map->slots, kOccMaxProbe);
  g->keys = map->keys.as<unsigned long long>();
  g->vals = map->hits.as<unsigned>();
}

// Times `stage` around `launch`; a query changes nothing and reports no overflow, so with sync it only waits for the stream.
template <class Launch> static int occ_query_run(sbm_occ_map* map, int stage, bool any, int sync, Launch launch) {
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  HIPCHK(h, occ_clock_start(h, stage, stage));
  if (any) {
    HIPCHK(h, clk.mark(kOccBegin, h->stream));
    launch();
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, clk.mark(kOccEnd, h->stream));
    HIPCHK(h, clk.add(stage, kOccBegin, kOccEnd));
  }
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

static int occ_search_run(sbm_occ_map* map, size_t n, const float* d_xyz, float thres, int* d_state, unsigned* d_value, int sync) {
  OccQuery g;
  occ_query_begin(map, -1., thres, 0, &g);
  return occ_query_run(map, kOccSearch, n > 0, sync, [&] {
    hipLaunchKernelGGL(occ_search_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, map->h->stream, d_xyz, n, g, d_state, d_value);
  });
}

static int occ_cast_run(sbm_occ_map* map, size_t n, const float* d_origins, const float* origin, const float* d_dirs,
                        const sbm_occ_query_params* p, int* d_status, float* d_end, int sync) {
  OccQuery g;
  occ_query_begin(map, p->max_range, p->occupancy_thres_log, p->ignore_unknown, &g);
  OccView v;
  memset(&v, 0, sizeof(v));
  v.shared = origin != nullptr;
  if (origin) memcpy(v.origin, origin, sizeof(v.origin));
  return occ_query_run(map, kOccCast, n > 0, sync, [&] {
    hipLaunchKernelGGL(occ_cast_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, map->h->stream, d_origins, d_dirs, n, v, g,
                       d_status, d_end);
  });
}

static int occ_query_params_check(const sbm_occ_query_params* p) {
  if (!p) return SBM_ERR_NULL;
  if (std::isnan(p->max_range) || std::isnan(p->occupancy_thres_log)) return SBM_ERR_SIZE;
  return SBM_OK;
}

static int occ_check_cast(const sbm_occ_map* map, size_t n, const void* origins, const void* dirs, const sbm_occ_query_params* p,
                          const void* status) {
  if (!map || !p || (n > 0 && (!origins || !dirs || !status))) return SBM_ERR_NULL;
  const int st = occ_query_params_check(p);
  if (st != SBM_OK) return st;
  if (n > ((size_t)1 << 30)) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

// ---- the .bt stream ------------------------------------------------------------------------------------------------------
// Morton code of a packed key: per bit, from the top, z y x -- a child index as computeChildIdx gives it
static uint64_t occ_morton(uint64_t key) {
  const uint64_t k0 = (key >> 32) & 0xFFFF, k1 = (key >> 16) & 0xFFFF, k2 = key & 0xFFFF;
  uint64_t m = 0;
  for (int b = 0; b < 16; b++) m |= ((k0 >> b & 1) | (k1 >> b & 1) << 1 | (k2 >> b & 1) << 2) << (3 * b);
  return m;
}

// A leaf of the stream: its Morton code above bit 0, and in bit 0 whether toMaxLikelihood makes it occupied. Sorting the words
// sorts the codes.
// The inner node that covers leaves [lo, hi) (sorted, distinct codes) with `level` key bits still undecided (16 at the root): its
// two bytes, then its inner children depth first. A child whose range holds all 8^(level-1) codes below it, all of one kind, is
// what prune() leaves as one leaf of that kind. Returns the nodes written, this one included.
static size_t occ_write_node(const uint64_t* lo, const uint64_t* hi, int level, std::vector<uint8_t>& body) {
  const int shift = 3 * (level - 1) + 1;
  const uint64_t full = (uint64_t)1 << (shift - 1);   // 8^(level-1)
  const uint64_t* edge[9];
  edge[0] = lo;
  for (int c = 0; c < 8; c++) {
    const uint64_t* e = edge[c];
    while (e < hi && ((*e >> shift) & 7) == (uint64_t)c) e++;
    edge[c + 1] = e;
  }
  uint8_t byte[2] = {0, 0};
  bool inner[8];
  size_t nodes = 1;
  for (int c = 0; c < 8; c++) {
    const uint64_t cnt = (uint64_t)(edge[c + 1] - edge[c]);
    inner[c] = false;
    if (!cnt) continue;
    const uint64_t kind = *edge[c] & 1;
    inner[c] = cnt != full;
    for (const uint64_t* e = edge[c]; !inner[c] && e < edge[c + 1]; e++) inner[c] = (*e & 1) != kind;
    // bits (2c, 2c+1): 0,1 occupied leaf; 1,0 free leaf; 1,1 inner
    byte[c / 4] |= (uint8_t)((inner[c] ? 3 : kind ? 2 : 1) << (2 * (c % 4)));
    if (!inner[c]) nodes++;
  }
  body.push_back(byte[0]);
  body.push_back(byte[1]);
  for (int c = 0; c < 8; c++)
    if (inner[c]) nodes += occ_write_node(edge[c], edge[c + 1], level - 1, body);
  return nodes;
}

// The .bt file: the header of AbstractOccupancyOcTree::writeBinaryConst, `res` as operator<<(double) prints it (%g), then the body
static int occ_write_file(const std::vector<uint8_t>& body, size_t nodes, double resolution, const char* path) {
  FILE* f = fopen(path, "wb");
  if (!f) return SBM_ERR_UNSUPPORTED;
  bool ok = fprintf(f,
                    "# Octomap OcTree binary file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
                    "id OcTree\nsize %zu\nres %g\ndata\n",
                    nodes, resolution) > 0;
  ok = ok && (body.empty() || fwrite(body.data(), 1, body.size(), f) == body.size());
  ok = (fclose(f) == 0) && ok;
  return ok ? SBM_OK : SBM_ERR_UNSUPPORTED;
}

// AbstractOccupancyOcTree::writeBinaryConst of the sorted leaves; `res` as operator<<(double) prints it (%g)
static int occ_write_stream(const std::vector<uint64_t>& leaf, double resolution, const char* path) {
  std::vector<uint8_t> body;
  size_t nodes = 0;
  try {
    if (!leaf.empty()) nodes = occ_write_node(leaf.data(), leaf.data() + leaf.size(), 16, body);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return occ_write_file(body, nodes, resolution, path);
}

// ---- reading a .bt stream (include/sbm.h, "occupancy map: load a .bt stream"): the host parser ------------------------------
__host__ __device__ unsigned occ_unspread(unsigned long long x);   // below, with the Morton codes of the tree

// A leaf as the parser hands it on and the device takes it: first Morton code of the cube << 8 | depth << 1 | occupied
typedef unsigned long long OccBtLeaf;
static uint64_t occ_bt_code(OccBtLeaf l) { return l >> 8; }
static int occ_bt_depth(OccBtLeaf l) { return (int)(l >> 1 & 31); }

struct OccBtParse {
  sbm_occ_binary_header info;
  std::vector<OccBtLeaf>* leaves;   // null: count only
  bool bounds;                      // key_min / key_max are wanted
  const uint8_t *at, *end;
};

// AbstractOcTree::readHeader on bytes [*pos, n): tokens up to the line `data`. SBM_ERR_SIZE where the stream ends first or a
// number does not parse (octomap's stream fails there and its loop ends without `data`).
static int occ_bt_header(const uint8_t* b, size_t n, size_t* pos, std::string* id, uint64_t* size, double* res) {
  size_t i = *pos;
  const auto space = [](uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); };
  const auto skip_line = [&] {
    while (i < n && b[i] != '\n') i++;
    if (i < n) i++;
  };
  const auto token = [&](std::string* t) {
    t->clear();
    while (i < n && space(b[i])) i++;
    while (i < n && !space(b[i])) t->push_back((char)b[i++]);
    return !t->empty();
  };
  std::string t;
  while (token(&t)) {
    if (t == "data") {
      skip_line();
      *pos = i;
      return SBM_OK;
    }
    if (t[0] == '#') {
      skip_line();
    } else if (t == "id") {
      if (!token(id)) return SBM_ERR_SIZE;
    } else if (t == "res" || t == "size") {
      while (i < n && space(b[i])) i++;
      char num[64];
      size_t len = 0;
      while (i + len < n && !space(b[i + len]) && len + 1 < sizeof(num)) num[len] = (char)b[i + len], len++;
      num[len] = 0;
      char* stop = num;
      if (t == "res") {
        *res = strtod(num, &stop);
      } else {
        if (num[0] < '0' || num[0] > '9') return SBM_ERR_SIZE;
        const unsigned long long v = strtoull(num, &stop, 10);
        if (v > 0xFFFFFFFFull) return SBM_ERR_SIZE;   // octomap's size is an unsigned
        *size = v;
      }
      if (stop == num) return SBM_ERR_SIZE;
      i += (size_t)(stop - num);   // what follows the number is the next token, as operator>> leaves it
    } else {
      skip_line();   // an unknown keyword: octomap warns and skips the line
    }
  }
  return SBM_ERR_SIZE;
}

// A leaf of the pruned tree: the node with Morton prefix `code` at `depth`
static int occ_bt_leaf(OccBtParse& p, uint64_t code, int depth, bool occupied) {
  sbm_occ_binary_header& o = p.info;
  const int level = 16 - depth;
  o.leaves++;
  o.leaves_at[depth]++;
  o.occupied += occupied ? 1 : 0;
  o.voxels += (uint64_t)1 << (3 * level);
  const uint64_t first = code << (3 * level);
  if (p.bounds) {
    const unsigned k[3] = {occ_unspread(first), occ_unspread(first >> 1), occ_unspread(first >> 2)};
    for (int a = 0; a < 3; a++) {
      o.key_min[a] = (uint16_t)std::min<unsigned>(o.key_min[a], k[a]);
      o.key_max[a] = (uint16_t)std::max<unsigned>(o.key_max[a], k[a] + (1u << level) - 1);
    }
  }
  if (p.leaves) p.leaves->push_back(first << 8 | (OccBtLeaf)depth << 1 | (occupied ? 1u : 0u));
  return SBM_OK;
}

// readBinaryNode of the node with Morton prefix `code` at `depth`, whose record is at p.at. Children in child order, depth first:
// the leaves arrive in Morton order.
static int occ_bt_node(OccBtParse& p, uint64_t code, int depth) {
  if (p.end - p.at < 2) return SBM_ERR_SIZE;   // the stream ends inside the tree
  const unsigned word = p.at[0] | (unsigned)p.at[1] << 8;
  p.at += 2;
  if (!word) return occ_bt_leaf(p, code, depth, true);   // a childless node keeps the clamp max readBinaryNode gave it
  for (int c = 0; c < 8; c++) {
    const unsigned kind = word >> (2 * c) & 3;
    if (!kind) continue;
    p.info.nodes++;
    int st;
    if (kind != 3) st = occ_bt_leaf(p, code << 3 | c, depth + 1, kind == 2);
    else if (depth + 1 >= 16) st = SBM_ERR_SIZE;             // a node below depth 16
    else st = occ_bt_node(p, code << 3 | c, depth + 1);
    if (st != SBM_OK) return st;
  }
  return SBM_OK;
}

// AbstractOccupancyOcTree::readBinary on n bytes -> the header's counts and, with `leaves`, the leaves in stream order
static int occ_bt_parse(const uint8_t* b, size_t n, sbm_occ_binary_header* info, std::vector<OccBtLeaf>* leaves, bool bounds = true) {
  static const char magic[] = "# Octomap OcTree binary file";
  OccBtParse p;
  memset(&p.info, 0, sizeof(p.info));
  for (int a = 0; a < 3; a++) p.info.key_min[a] = 0xFFFF;
  p.leaves = leaves;
  p.bounds = bounds && info != nullptr;
  int st = SBM_OK;
  size_t pos = 0;
  std::string id;
  try {
    if (n < sizeof(magic) - 1 || memcmp(b, magic, sizeof(magic) - 1) != 0) {
      st = SBM_ERR_UNSUPPORTED;   // the legacy header, or no .bt at all
    } else {
      while (pos < n && b[pos] != '\n') pos++;   // std::getline
      if (pos < n) pos++;
      st = occ_bt_header(b, n, &pos, &id, &p.info.size, &p.info.resolution);
    }
    if (st == SBM_OK && id != "OcTree" && id != "1") st = SBM_ERR_UNSUPPORTED;   // "1" is the id octomap itself renames
    if (st == SBM_OK && !(p.info.resolution > 0.)) st = SBM_ERR_SIZE;
    if (st == SBM_OK && p.info.size > 0) {
      if (leaves) leaves->reserve((size_t)std::min<uint64_t>(p.info.size, 4 * (uint64_t)(n - pos)));   // a record has 8 children at most
      p.at = b + pos;
      p.end = b + n;
      p.info.nodes = 1;
      st = occ_bt_node(p, 0, 0);
    }
  } catch (const std::bad_alloc&) {
    st = SBM_ERR_NOMEM;
  }
  if (st == SBM_OK && p.info.nodes != p.info.size) st = SBM_ERR_SIZE;   // calcNumNodes() against the header
  if (info) *info = p.info;
  return st;
}

// ---- the octree above the voxels (include/sbm.h, "occupancy map: the octree above the voxels") ------------------------------
// A snapshot: the map's voxels sorted by Morton code are depth 16, and sixteen bottom-up passes put the sixteen levels above
// them, each level its own ascending code array. Siblings are neighbours in that order, so a parent is made by the first of its
// children (its "head"); where a head lands is an exclusive scan over head flags. Nothing waits on another workgroup: every
// step is a launch of its own, and the only atomics are integer counts (per-depth node counts, key bounds, the cursor of a
// compaction that a sort follows).
//   occ_tree_code      packed key -> 48-bit Morton code in place; the MAXLIKELIHOOD reading of the value; key bounds
//   occ_tree_diverge   per voxel the depth at which its code leaves its left neighbour's: the prefix sums are the level sizes
//   occ_tree_heads / occ_tree_scan / occ_tree_parents   one level: heads per tile of 1024 children, the scan of the tile counts,
//                      and one write per head -- code, max, child mask, first child, collapsed, non-leaf nodes in the subtree
//   occ_tree_down      top-down, one launch per depth: the depth of the shallowest collapsed node at or above every node (which is
//                      membership in the pruned tree and search's found depth), the per-depth counts, the pre-order rank of every
//                      non-leaf node of the pruned tree
//   occ_tree_search / occ_tree_select + the radix sort + occ_tree_gather / occ_tree_binary   the queries
constexpr int kOccDepth = 16;
constexpr unsigned kOccCollapsed = 1u << 8;   // info word of a node: bits 0-7 child mask, bit 8 collapsed,
constexpr int kOccTopShift = 10;              // bits 10-14 the depth of the shallowest collapsed node at or above it, or
constexpr unsigned kOccNoTop = 31;            // kOccNoTop
constexpr unsigned kOccInnerTag = 1u << 31;   // payload of a selected node: its index among the leaves, or tag | index above them

struct OccTreeStats {
  unsigned long long diverge[kOccDepth + 1];                            // voxels by the depth at which they leave their left neighbour
  unsigned long long nodes_at[kOccDepth + 1], leaves_at[kOccDepth + 1]; // of the pruned tree
  unsigned kmin[3], kmax[3];
  unsigned cursor, pad;                                                 // compaction cursor of a leaves call
};

struct OccLevel {                 // one depth of a built tree
  unsigned long long* code;       // Morton prefixes (3 bits per depth), ascending
  unsigned* val;                  // float bits: the maximum over the voxels below
  unsigned* parent;               // index in the level above
  unsigned* info;
  unsigned *first, *inner, *rank; // above depth 16: the first child's index in the level below, the non-leaf nodes of the pruned
                                  // tree in the subtree (this one included), the pre-order rank among them
  uint32_t n;
};

// every third bit of a 16-bit key; unspread is its inverse
__host__ __device__ __forceinline__ unsigned long long occ_spread(unsigned long long x) {
  x &= 0xFFFFull;
  x = (x | x << 32) & 0x001F00000000FFFFull;
  x = (x | x << 16) & 0x001F0000FF0000FFull;
  x = (x | x << 8) & 0x100F00F00F00F00Full;
  x = (x | x << 4) & 0x10C30C30C30C30C3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

__host__ __device__ __forceinline__ unsigned occ_unspread(unsigned long long x) {
  x &= 0x1249249249249249ull;
  x = (x ^ x >> 2) & 0x10C30C30C30C30C3ull;
  x = (x ^ x >> 4) & 0x100F00F00F00F00Full;
  x = (x ^ x >> 8) & 0x001F0000FF0000FFull;
  x = (x ^ x >> 16) & 0x001F00000000FFFFull;
  x = (x ^ x >> 32) & 0xFFFFull;
  return (unsigned)x;
}

// computeChildIdx from the top bit down: x in bit 0, y in bit 1, z in bit 2 of every triple (occ_morton, on the host)
__host__ __device__ __forceinline__ unsigned long long occ_code(unsigned k0, unsigned k1, unsigned k2) {
  return occ_spread(k0) | occ_spread(k1) << 1 | occ_spread(k2) << 2;
}

// ---- loading a .bt stream: the expansion -----------------------------------------------------------------------------------
// A pruned leaf of depth d stands for 8^(16-d) voxels whose Morton codes are its first code OR'd with 0 .. 8^(16-d) - 1.
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
    const unsigned long long code = (word >> 8) | (unsigned long long)(i - first[lo]);
    const unsigned long long key = (unsigned long long)occ_unspread(code) << 32 | (unsigned long long)occ_unspread(code >> 1) << 16 |
                                   occ_unspread(code >> 2);
    lost = true;
    uint32_t slot = occ_hash(key, g.mask);
    for (uint32_t probe = 0; probe < g.max_probe; probe++, slot = (slot + 1) & g.mask) {
      unsigned long long cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kOccEmpty) {
        cur = atomicCAS(&keys[slot], kOccEmpty, key);
        if (cur == kOccEmpty) {
          claimed = true;
          cur = key;
        }
      }
      if (cur == key) {
        vals[slot] = (word & 1) ? g.vmax : g.vmin;
        lost = false;
        break;
      }
    }
  }
  const unsigned long long got = __ballot(claimed), over = __ballot(lost);
  if ((threadIdx.x & 63) == 0) {
    if (got) atomicAdd(&ctr->size, (unsigned)__popcll(got));
    if (over) atomicAdd(&ctr->overflow, (unsigned long long)__popcll(over));
  }
}

__device__ __forceinline__ unsigned occ_wave_min(unsigned v) {
  for (int o = 32; o; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ unsigned occ_wave_max(unsigned v) {
  for (int o = 32; o; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
  return v;
}

struct OccReading {   // how a stored word becomes a leaf's value
  int max_likelihood, hits;
  float thres;
  unsigned cmin, cmax;   // float bits
};

__global__ void __launch_bounds__(256) occ_tree_code_kernel(unsigned long long* __restrict__ keys, unsigned* __restrict__ vals, uint32_t n,
                                                             OccReading r, OccTreeStats* __restrict__ st) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  unsigned lo[3] = {~0u, ~0u, ~0u}, hi[3] = {0u, 0u, 0u};
  if (i < n) {
    const unsigned long long key = keys[i];
    const unsigned k[3] = {(unsigned)(key >> 32) & 0xFFFF, (unsigned)(key >> 16) & 0xFFFF, (unsigned)key & 0xFFFF};
    keys[i] = occ_code(k[0], k[1], k[2]);
    if (r.max_likelihood) vals[i] = (r.hits || __uint_as_float(vals[i]) >= r.thres) ? r.cmax : r.cmin;   // toMaxLikelihood
    for (int a = 0; a < 3; a++) lo[a] = hi[a] = k[a];
  }
  for (int a = 0; a < 3; a++) {   // every lane of the wavefront is here
    lo[a] = occ_wave_min(lo[a]);
    hi[a] = occ_wave_max(hi[a]);
  }
  if ((threadIdx.x & 63) == 0 && lo[0] != ~0u)
    for (int a = 0; a < 3; a++) {
      atomicMin(&st->kmin[a], lo[a]);
      atomicMax(&st->kmax[a], hi[a]);
    }
}

__global__ void __launch_bounds__(256) occ_tree_diverge_kernel(const unsigned long long* __restrict__ code, uint32_t n,
                                                                OccTreeStats* __restrict__ st) {
  __shared__ unsigned cnt[kOccDepth + 1];
  if (threadIdx.x <= kOccDepth) cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    int d = 0;   // the first voxel opens a node at every depth
    if (i) {
      const unsigned long long x = code[i] ^ code[i - 1];
      d = x ? kOccDepth - (63 - __clzll((long long)x)) / 3 : kOccDepth;   // the codes are distinct: x is never 0
    }
    atomicAdd(&cnt[min(max(d, 0), kOccDepth)], 1u);
  }
  __syncthreads();
  if (threadIdx.x <= kOccDepth && cnt[threadIdx.x]) atomicAdd(&st->diverge[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

__device__ __forceinline__ bool occ_tree_head(const unsigned long long* code, uint32_t i) {
  return i == 0 || (code[i] >> 3) != (code[i - 1] >> 3);
}

// heads among one tile of kOccTile children
__global__ void __launch_bounds__(256) occ_tree_heads_kernel(const unsigned long long* __restrict__ code, uint32_t n,
                                                              unsigned* __restrict__ tile_heads) {
  __shared__ unsigned wsum[4];
  const uint32_t base = blockIdx.x * kOccTile;
  unsigned c = 0;
  for (uint32_t j = threadIdx.x; j < kOccTile; j += 256) c += (base + j < n && occ_tree_head(code, base + j)) ? 1u : 0u;
  for (int o = 32; o; o >>= 1) c += (unsigned)__shfl_xor((int)c, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_heads[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive scan of the tile counts in place; one workgroup, a run of tiles per thread
__global__ void __launch_bounds__(256) occ_tree_scan_kernel(unsigned* __restrict__ v, uint32_t tiles) {
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
}

// One level: every head writes its parent and tells its (at most eight) children where it is. tile_off: the scanned tile counts,
// or null for a level of one tile. leaves: the children are depth 16.
__global__ void __launch_bounds__(256) occ_tree_parents_kernel(OccLevel c, OccLevel p, const unsigned* __restrict__ tile_off, int leaves) {
  __shared__ unsigned wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned running = tile_off ? tile_off[blockIdx.x] : 0;
  for (int r = 0; r < kOccTile / 256; r++) {   // the same trips for every thread: the barriers below are reached by all
    const uint32_t i = blockIdx.x * kOccTile + r * 256 + threadIdx.x;
    const bool head = i < c.n && occ_tree_head(c.code, i);
    const unsigned long long heads = __ballot(head);
    if (lane == 0) wsum[wave] = __popcll(heads);
    __syncthreads();
    unsigned before = running;
    for (int w = 0; w < wave; w++) before += wsum[w];
    running += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    const uint32_t at = before + __popcll(heads & ((1ull << lane) - 1));
    if (!head || at >= p.n) continue;   // the level sizes are exact: no head lands beyond
    const unsigned long long code = c.code[i] >> 3;
    const unsigned v0 = c.val[i];
    unsigned best = v0, mask = 0, inner = 0;
    bool all_leaves = true, equal = true;
    for (uint32_t j = i; j < c.n && j - i < 8 && (c.code[j] >> 3) == code; j++) {
      const unsigned v = c.val[j];
      if (__uint_as_float(v) > __uint_as_float(best)) best = v;              // updateOccupancyChildren: the maximum
      equal = equal && __uint_as_float(v) == __uint_as_float(v0);            // isNodeCollapsible: float ==
      mask |= 1u << (unsigned)(c.code[j] & 7);
      if (!leaves) {
        all_leaves = all_leaves && (c.info[j] & kOccCollapsed);
        inner += c.inner[j];
      }
      c.parent[j] = at;
    }
    const bool collapsed = mask == 0xFF && all_leaves && equal;
    p.code[at] = code;
    p.val[at] = best;
    p.first[at] = i;
    p.info[at] = mask | (collapsed ? kOccCollapsed : 0u);
    p.inner[at] = collapsed ? 0u : 1u + inner;
  }
}

// Top-down, depth by depth (the level above is finished: an earlier launch). A node is in the pruned tree iff nothing above it is
// collapsed; in it, it is a leaf iff it is depth 16 or collapsed. The rank of a non-leaf node among such nodes in pre-order is its
// parent's, plus one, plus the non-leaf nodes under its earlier siblings.
__global__ void __launch_bounds__(256) occ_tree_down_kernel(OccLevel l, OccLevel up, int depth, OccTreeStats* __restrict__ st) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool node = false, leaf = false;
  if (i < l.n) {
    const unsigned mine = depth < kOccDepth ? l.info[i] & (kOccCollapsed | 0xFFu) : 0u;
    const bool collapsed = (mine & kOccCollapsed) != 0;
    unsigned p = 0, top = kOccNoTop;
    if (depth) {
      p = l.parent[i];
      top = (up.info[p] >> kOccTopShift) & 31u;
    }
    const bool pruned = top != kOccNoTop;
    if (!pruned && collapsed) top = (unsigned)depth;
    l.info[i] = mine | top << kOccTopShift;
    if (depth < kOccDepth) {
      unsigned rank = 0;
      if (!pruned && !collapsed && depth) {
        rank = up.rank[p] + 1;
        for (uint32_t s = up.first[p]; s < i; s++) rank += l.inner[s];
      }
      l.rank[i] = rank;
    }
    node = !pruned;
    leaf = node && (depth == kOccDepth || collapsed);
  }
  const unsigned long long nodes = __ballot(node), leaves = __ballot(leaf);
  if ((threadIdx.x & 63) == 0) {
    if (nodes) atomicAdd(&st->nodes_at[depth], (unsigned long long)__popcll(nodes));
    if (leaves) atomicAdd(&st->leaves_at[depth], (unsigned long long)__popcll(leaves));
  }
}

// search(point, depth): one lane per point, a binary search over the codes of the asked depth with plain loads
__global__ void __launch_bounds__(256) occ_tree_search_kernel(const float* __restrict__ xyz, size_t n, double factor, OccLevel l, int depth,
                                                               float thres, int* __restrict__ state, unsigned* __restrict__ value,
                                                               int* __restrict__ found) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned k0, k1, k2, word = 0x7FC00000u;
  int st = SBM_OCC_CELL_OUT, fd = -1;
  if (occ_axis(factor, xyz[3 * i], &k0) && occ_axis(factor, xyz[3 * i + 1], &k1) && occ_axis(factor, xyz[3 * i + 2], &k2)) {
    const unsigned long long code = occ_code(k0, k1, k2) >> (3 * (kOccDepth - depth));
    uint32_t lo = 0, hi = l.n;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (l.code[mid] < code) lo = mid + 1;
      else hi = mid;
    }
    st = SBM_OCC_CELL_UNKNOWN;
    if (lo < l.n && l.code[lo] == code) {
      word = l.val[lo];
      st = __uint_as_float(word) >= thres ? SBM_OCC_CELL_OCCUPIED : SBM_OCC_CELL_FREE;
      const unsigned top = (l.info[lo] >> kOccTopShift) & 31u;
      fd = top != kOccNoTop ? (int)top : depth;
    }
  }
  state[i] = st;
  if (value) value[i] = word;
  if (found) found[i] = fd;
}

// begin_leafs(max_depth) of one depth: the leaves of the pruned tree, and at max_depth every node of it, as (first Morton code of
// the cube, where the node is). The cubes are disjoint, so the sort that follows puts them in octomap's order whatever the
// order of arrival here.
__global__ void __launch_bounds__(256) occ_tree_select_kernel(OccLevel l, int depth, int max_depth, unsigned tag, uint32_t cap,
                                                               unsigned long long* __restrict__ out_code, unsigned* __restrict__ out_at,
                                                               OccTreeStats* __restrict__ st) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool take = false;
  if (i < l.n) {
    const unsigned info = l.info[i], top = (info >> kOccTopShift) & 31u;
    const bool pruned = top != kOccNoTop && top < (unsigned)depth;
    take = !pruned && (depth == kOccDepth || (info & kOccCollapsed) || depth == max_depth);
  }
  const unsigned long long taken = __ballot(take);
  if (!taken) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)taken) - 1;
  unsigned base = 0;
  if (lane == leader) base = atomicAdd(&st->cursor, (unsigned)__popcll(taken));
  base = __builtin_amdgcn_readlane(base, leader);
  if (!take) return;
  const uint32_t o = base + __popcll(taken & ((1ull << lane) - 1));
  if (o >= cap) return;
  out_code[o] = l.code[i] << (3 * (kOccDepth - depth));
  out_at[o] = tag + i;
}

struct OccTreeRef {   // where a selected node's value and depth are
  const unsigned *leaf_val, *node_val;
  uint32_t off[kOccDepth];   // of depth d among the nodes above the leaves
};

// the sorted selection in place: first code -> centre key (adjustKeyAtDepth), where -> depth, and the value
__global__ void __launch_bounds__(256) occ_tree_gather_kernel(unsigned long long* __restrict__ keys, int* __restrict__ depth_io,
                                                               unsigned* __restrict__ value, uint32_t n, OccTreeRef t) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned at = (unsigned)depth_io[i];
  int depth = kOccDepth;
  unsigned v;
  if (at & kOccInnerTag) {
    const unsigned g = at & ~kOccInnerTag;
    depth = kOccDepth - 1;
    while (depth > 0 && t.off[depth] > g) depth--;
    v = t.node_val[g];
  } else {
    v = t.leaf_val[at];
  }
  const unsigned long long code = keys[i];
  const unsigned half = depth < kOccDepth ? 1u << (kOccDepth - depth - 1) : 0u;   // the low bits of the first code are zero
  keys[i] = (unsigned long long)(occ_unspread(code) | half) << 32 | (unsigned long long)(occ_unspread(code >> 1) | half) << 16 |
            (occ_unspread(code >> 2) | half);
  depth_io[i] = depth;
  if (value) value[i] = v;
}

// writeBinaryNode: every non-leaf node of the pruned tree writes its two bytes at twice its rank. Per child two bits, the first
// of the pair lower: 00 none, 01 occupied leaf, 10 free leaf, 11 inner; a leaf is occupied iff it holds clamp max.
__global__ void __launch_bounds__(256) occ_tree_binary_kernel(OccLevel l, OccLevel below, int depth, unsigned cmax, uint8_t* __restrict__ out,
                                                               size_t cap) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= l.n) return;
  const unsigned info = l.info[i];
  if (((info >> kOccTopShift) & 31u) != kOccNoTop) return;   // collapsed, or below a collapsed node
  uint32_t child = l.first[i];
  unsigned word = 0;
  for (int c = 0; c < 8; c++) {
    if (!(info >> c & 1u)) continue;
    unsigned kind = 3;
    if (child < below.n && (depth + 1 == kOccDepth || (below.info[child] & kOccCollapsed))) kind = below.val[child] == cmax ? 2 : 1;
    word |= kind << (2 * c);
    child++;
  }
  const size_t o = 2 * (size_t)l.rank[i];
  if (o + 1 < cap) {
    out[o] = (uint8_t)(word & 0xFF);
    out[o + 1] = (uint8_t)(word >> 8);
  }
}

}  // namespace sbm

struct sbm_occ_tree {
  sbm_handle* h;
  sbm_occ_map* map;            // read by a build only
  bool built, have_stats;      // levels are valid; `host` holds the last build's counts
  int reading;
  double resolution;
  unsigned cmax;               // float bits of clamp max, what .bt calls occupied
  uint32_t count[17];          // nodes per depth, pruned or not; count[16] is the voxels
  size_t off[16], inner_total; // where depth d begins among the nodes above the leaves, and how many those are
  sbm::OccTreeStats host;
  sbm::DevBuf leaf, node;      // depth 16: code, value, parent, info (20 B per voxel); above: code, value, parent, info, first
                               // child, subtree count, rank (32 B per node)
  sbm::DevBuf stats, tiles;    // OccTreeStats; head counts per tile of the level being built
  template <class F> void each(F f) { f(leaf); f(node); f(stats); f(tiles); }
};

namespace sbm {

// ---- the tree, host side -------------------------------------------------------------------------------------------------
static size_t occ_pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// Depth d of a built tree; a tree that was never built, or whose build failed, has empty levels.
static OccLevel occ_tree_level(const sbm_occ_tree* t, int d) {
  OccLevel l;
  memset(&l, 0, sizeof(l));
  if (!t->built) return l;
  l.n = t->count[d];
  if (d == kOccDepth) {   // leaf: codes, values, parents, info words
    char* b = t->leaf.as<char>();
    const size_t n = l.n;
    l.code = (unsigned long long*)b;
    l.val = (unsigned*)(b + occ_pad(8 * n));
    l.parent = (unsigned*)(b + occ_pad(8 * n) + occ_pad(4 * n));
    l.info = (unsigned*)(b + occ_pad(8 * n) + 2 * occ_pad(4 * n));
    return l;
  }
  char* b = t->node.as<char>();   // node: seven arrays over all the depths above 16, depth 0 first
  const size_t all = t->inner_total, w = occ_pad(4 * all), o = t->off[d];
  unsigned* word = (unsigned*)(b + occ_pad(8 * all));
  l.code = (unsigned long long*)b + o;
  l.val = word + o;
  l.parent = (unsigned*)((char*)word + w) + o;
  l.info = (unsigned*)((char*)word + 2 * w) + o;
  l.first = (unsigned*)((char*)word + 3 * w) + o;
  l.inner = (unsigned*)((char*)word + 4 * w) + o;
  l.rank = (unsigned*)((char*)word + 5 * w) + o;
  return l;
}

static int occ_tree_build_run(sbm_occ_tree* t, int reading, const sbm_occ_ray_params* rp, int sync) {
  sbm_occ_map* map = t->map;
  sbm_handle* h = t->h;
  StageClock& clk = h->occ.clock;
  HIPCHK(h, occ_clock_start(h, kOccTreeBuild, kOccTreeBuild));
  t->built = false;
  t->have_stats = false;
  t->reading = reading;
  t->resolution = map->p.resolution;
  memset(t->count, 0, sizeof(t->count));
  memset(t->off, 0, sizeof(t->off));
  t->inner_total = 0;
  OccReading r;
  memset(&r, 0, sizeof(r));
  if (rp) {
    const float cmin = occ_logodds(rp->clamp_min), cmax = occ_logodds(rp->clamp_max);
    r.thres = occ_logodds(rp->occupancy_thres);
    memcpy(&r.cmin, &cmin, 4);
    memcpy(&r.cmax, &cmax, 4);
  }
  r.max_likelihood = reading == SBM_OCC_TREE_MAXLIKELIHOOD;
  r.hits = map->mode == kOccModeHits;
  t->cmax = r.cmax;
  OccCounters c;
  int st = occ_read_counters(map, &c);
  if (st != SBM_OK) return st;
  const uint32_t n = c.size;
  HIPCHK(h, t->stats.grow(sizeof(OccTreeStats), h->stream));
  OccTreeStats* stats = t->stats.as<OccTreeStats>();
  HIPCHK(h, hipMemsetAsync(stats, 0, sizeof(OccTreeStats), h->stream));
  HIPCHK(h, hipMemsetAsync(stats->kmin, 0xFF, sizeof(stats->kmin), h->stream));
  if (!n) {
    t->built = true;
    if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
    return SBM_OK;
  }
  const uint32_t tiles = (n + kOccTile - 1) / kOccTile, blocks = (n + 255) / 256;
  const size_t kb = occ_pad((size_t)n * 8), vb = occ_pad((size_t)n * 4);
  HIPCHK(h, t->leaf.grow(kb + 3 * vb, h->stream));
  HIPCHK(h, h->occ.sort.grow(kb + vb, h->stream));
  HIPCHK(h, h->occ.hist.grow((size_t)256 * tiles * 4, h->stream));
  unsigned long long* kk[2] = {t->leaf.as<unsigned long long>(), h->occ.sort.as<unsigned long long>()};
  unsigned* vv[2] = {(unsigned*)(t->leaf.as<char>() + kb), (unsigned*)(h->occ.sort.as<char>() + kb)};
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  HIPCHK(h, hipMemsetAsync((char*)map->ctr.p + offsetof(OccCounters, cursor), 0, sizeof(unsigned), h->stream));
  hipLaunchKernelGGL(occ_compact_kernel, dim3((map->slots + 255) / 256), dim3(256), 0, h->stream, map->keys.as<unsigned long long>(),
                     map->hits.as<unsigned>(), map->slots, n, kk[0], vv[0], map->ctr.as<OccCounters>());
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(occ_tree_code_kernel, dim3(blocks), dim3(256), 0, h->stream, kk[0], vv[0], n, r, stats);
  HIPCHK(h, hipGetLastError());
  st = occ_sort_run(h, kk, vv, n, h->occ.hist.as<unsigned>());
  if (st != SBM_OK) return st;
  hipLaunchKernelGGL(occ_tree_diverge_kernel, dim3(blocks), dim3(256), 0, h->stream, kk[0], n, stats);
  HIPCHK(h, hipGetLastError());
  // the level sizes: a node of depth d begins at every voxel that leaves its left neighbour at depth d or above
  unsigned long long diverge[kOccDepth + 1];
  HIPCHK(h, hipMemcpyAsync(diverge, stats->diverge, sizeof(diverge), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  unsigned long long run = 0, inner_total = 0;
  for (int d = 0; d <= kOccDepth; d++) {
    run += diverge[d];
    if (run > n) return SBM_ERR_HIP;   // cannot happen: every voxel is counted once
    t->count[d] = (uint32_t)run;
    if (d < kOccDepth) {
      t->off[d] = (size_t)inner_total;
      inner_total += run;
    }
  }
  if (t->count[kOccDepth] != n) return SBM_ERR_HIP;
  if (inner_total >= ((unsigned long long)1 << 31)) return SBM_ERR_UNSUPPORTED;   // ranks and subtree counts are 32-bit
  t->inner_total = (size_t)inner_total;
  HIPCHK(h, t->node.grow(occ_pad(8 * t->inner_total) + 6 * occ_pad(4 * t->inner_total), h->stream));
  HIPCHK(h, t->tiles.grow((size_t)tiles * 4, h->stream));
  t->built = true;   // occ_tree_level answers from here on; a failure below takes it back
  st = [&]() -> int {
    for (int d = kOccDepth - 1; d >= 0; d--) {   // bottom-up: the parents of depth d + 1
      const OccLevel child = occ_tree_level(t, d + 1), parent = occ_tree_level(t, d);
      const uint32_t ct = (child.n + kOccTile - 1) / kOccTile;
      unsigned* tile_off = nullptr;
      if (ct > 1) {
        tile_off = t->tiles.as<unsigned>();
        hipLaunchKernelGGL(occ_tree_heads_kernel, dim3(ct), dim3(256), 0, h->stream, child.code, child.n, tile_off);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL(occ_tree_scan_kernel, dim3(1), dim3(256), 0, h->stream, tile_off, ct);
        HIPCHK(h, hipGetLastError());
      }
      hipLaunchKernelGGL(occ_tree_parents_kernel, dim3(ct), dim3(256), 0, h->stream, child, parent, tile_off, d + 1 == kOccDepth ? 1 : 0);
      HIPCHK(h, hipGetLastError());
    }
    for (int d = 0; d <= kOccDepth; d++) {       // top-down
      const OccLevel l = occ_tree_level(t, d), up = occ_tree_level(t, d ? d - 1 : 0);
      hipLaunchKernelGGL(occ_tree_down_kernel, dim3((l.n + 255) / 256), dim3(256), 0, h->stream, l, up, d, stats);
      HIPCHK(h, hipGetLastError());
    }
    return SBM_OK;
  }();
  if (st != SBM_OK) {
    t->built = false;
    return st;
  }
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(kOccTreeBuild, kOccBegin, kOccEnd));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

// The counts of the last build, read once
static int occ_tree_stats(sbm_occ_tree* t) {
  sbm_handle* h = t->h;
  if (t->have_stats) return SBM_OK;
  memset(&t->host, 0, sizeof(t->host));
  for (int a = 0; a < 3; a++) t->host.kmin[a] = 0xFFFF;
  if (t->built && t->count[kOccDepth]) {
    HIPCHK(h, hipMemcpyAsync(&t->host, t->stats.p, sizeof(OccTreeStats), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  t->have_stats = true;
  return SBM_OK;
}

// Times `launch` as the stage occ_tree_query
template <class Launch> static int occ_tree_query_run(sbm_occ_tree* t, bool any, int sync, Launch launch) {
  sbm_handle* h = t->h;
  StageClock& clk = h->occ.clock;
  HIPCHK(h, occ_clock_start(h, kOccTreeQuery, kOccTreeQuery));
  if (any) {
    HIPCHK(h, clk.mark(kOccBegin, h->stream));
    const int st = launch();
    if (st != SBM_OK) return st;
    HIPCHK(h, clk.mark(kOccEnd, h->stream));
    HIPCHK(h, clk.add(kOccTreeQuery, kOccBegin, kOccEnd));
  }
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

static int occ_tree_search_run(sbm_occ_tree* t, size_t n, const float* d_xyz, int depth, float thres, int* d_state, unsigned* d_value,
                               int* d_found, int sync) {
  sbm_handle* h = t->h;
  const OccLevel l = occ_tree_level(t, depth);
  return occ_tree_query_run(t, n > 0, sync, [&]() -> int {
    hipLaunchKernelGGL(occ_tree_search_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, d_xyz, n, 1. / t->resolution, l,
                       depth, thres, d_state, d_value, d_found);
    HIPCHK(h, hipGetLastError());
    return SBM_OK;
  });
}

// The entries begin_leafs(max_depth) visits: the leaves down to max_depth and the other nodes of that depth
static size_t occ_tree_leaf_count(const sbm_occ_tree* t, int max_depth) {
  unsigned long long n = t->host.nodes_at[max_depth] - t->host.leaves_at[max_depth];
  for (int d = 0; d <= max_depth; d++) n += t->host.leaves_at[d];
  return (size_t)n;
}

static int occ_tree_leaves_run(sbm_occ_tree* t, int max_depth, unsigned long long* d_keys, int* d_depth, unsigned* d_value, size_t cap,
                               size_t* count) {
  sbm_handle* h = t->h;
  int st = occ_tree_stats(t);
  if (st != SBM_OK) return st;
  const size_t total = occ_tree_leaf_count(t, max_depth);
  *count = total;
  if (total > cap) return SBM_ERR_SIZE;
  const uint32_t n = (uint32_t)total;
  return occ_tree_query_run(t, n > 0, 1, [&]() -> int {
    const uint32_t tiles = (n + kOccTile - 1) / kOccTile;
    const size_t kb = occ_pad((size_t)n * 8);
    HIPCHK(h, h->occ.sort.grow(kb + occ_pad((size_t)n * 4), h->stream));
    HIPCHK(h, h->occ.hist.grow((size_t)256 * tiles * 4, h->stream));
    OccTreeStats* stats = t->stats.as<OccTreeStats>();
    HIPCHK(h, hipMemsetAsync(&stats->cursor, 0, sizeof(unsigned), h->stream));
    unsigned long long* kk[2] = {d_keys, h->occ.sort.as<unsigned long long>()};
    unsigned* vv[2] = {(unsigned*)d_depth, (unsigned*)(h->occ.sort.as<char>() + kb)};
    OccTreeRef ref;
    memset(&ref, 0, sizeof(ref));
    ref.leaf_val = occ_tree_level(t, kOccDepth).val;
    ref.node_val = occ_tree_level(t, 0).val;
    for (int d = 0; d < kOccDepth; d++) ref.off[d] = (uint32_t)t->off[d];
    for (int d = 0; d <= max_depth; d++) {
      const OccLevel l = occ_tree_level(t, d);
      const unsigned tag = d == kOccDepth ? 0u : kOccInnerTag | (unsigned)t->off[d];
      hipLaunchKernelGGL(occ_tree_select_kernel, dim3((l.n + 255) / 256), dim3(256), 0, h->stream, l, d, max_depth, tag, n, kk[0], vv[0], stats);
      HIPCHK(h, hipGetLastError());
    }
    const int st = occ_sort_run(h, kk, vv, n, h->occ.hist.as<unsigned>());
    if (st != SBM_OK) return st;
    hipLaunchKernelGGL(occ_tree_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, d_keys, d_depth, d_value, n, ref);
    HIPCHK(h, hipGetLastError());
    return SBM_OK;
  });
}

static int occ_tree_binary_run(sbm_occ_tree* t, uint8_t* d_bytes, size_t cap, size_t* nbytes) {
  sbm_handle* h = t->h;
  int st = occ_tree_stats(t);
  if (st != SBM_OK) return st;
  unsigned long long inner = 0;
  for (int d = 0; d < kOccDepth; d++) inner += t->host.nodes_at[d] - t->host.leaves_at[d];
  *nbytes = (size_t)(2 * inner);
  if (*nbytes > cap) return SBM_ERR_SIZE;
  return occ_tree_query_run(t, inner > 0, 1, [&]() -> int {
    for (int d = 0; d < kOccDepth; d++) {
      const OccLevel l = occ_tree_level(t, d), below = occ_tree_level(t, d + 1);
      hipLaunchKernelGGL(occ_tree_binary_kernel, dim3((l.n + 255) / 256), dim3(256), 0, h->stream, l, below, d, t->cmax, d_bytes, *nbytes);
      HIPCHK(h, hipGetLastError());
    }
    return SBM_OK;
  });
}

// ---- loading a .bt stream, host side ----------------------------------------------------------------------------------------
// What sbm_occ_write_binary* print for a resolution (%g), read back
static double occ_printed_resolution(double resolution) {
  char text[64];
  snprintf(text, sizeof(text), "%g", resolution);
  return strtod(text, nullptr);
}

// readBinary into the map. Everything that can refuse the stream comes before the map is touched.
static int occ_load_run(sbm_occ_map* map, const uint8_t* bytes, size_t n, const sbm_occ_ray_params* p, int sync) {
  sbm_handle* h = map->h;
  sbm_occ_binary_header info;
  std::vector<OccBtLeaf> leaves;
  int st = occ_bt_parse(bytes, n, &info, &leaves, false);
  if (st != SBM_OK) return st;
  if (info.resolution != occ_printed_resolution(map->p.resolution)) return SBM_ERR_SIZE;
  if (info.voxels > map->capacity) return SBM_ERR_OCC_FULL;
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
  const size_t wb = occ_pad(count * 8);
  HIPCHK(h, h->occ.io.grow(wb + count * 4, h->stream));
  unsigned long long* d_word = h->occ.io.as<unsigned long long>();
  unsigned* d_first = (unsigned*)(h->occ.io.as<char>() + wb);
  HIPCHK(h, hipMemcpyAsync(d_word, leaves.data(), count * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_first, first.data(), count * 4, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // the host arrays end with this call
  OccLoad g;
  g.leaves = (uint32_t)count;
  g.total = (uint32_t)info.voxels;
  g.mask = map->slots - 1;
  g.max_probe = std::min(map->slots, kOccMaxProbe);
  const float cmin = occ_logodds(p->clamp_min), cmax = occ_logodds(p->clamp_max);
  memcpy(&g.vmin, &cmin, 4);
  memcpy(&g.vmax, &cmax, 4);
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  st = occ_clear(map);
  if (st != SBM_OK) return st;
  map->mode = kOccModeLogOdds;
  hipLaunchKernelGGL(occ_load_kernel, dim3((g.total + 255) / 256), dim3(256), 0, h->stream, d_word, d_first, g,
                     map->keys.as<unsigned long long>(), map->hits.as<unsigned>(), map->ctr.as<OccCounters>());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(kOccLoad, kOccBegin, kOccEnd));
  return occ_rays_end(map, sync);
}

static int occ_tree_depth_check(int depth) { return depth < 0 || depth > kOccDepth ? SBM_ERR_SIZE : SBM_OK; }

}  // namespace sbm

// ---- entry points --------------------------------------------------------------------------------------------------------
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
  const size_t kb = ((size_t)c.size * 8 + 255) & ~(size_t)255;
  HIPCHK(h, h->occ.io.grow(kb + (size_t)c.size * 4, h->stream));
  unsigned long long* d_k = h->occ.io.as<unsigned long long>();
  unsigned* d_v = (unsigned*)((char*)h->occ.io.p + kb);
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
  if ((uintptr_t)d_disp & 1 || map->mode == kOccModeLogOdds) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  map->mode = kOccModeHits;
  return occ_insert_run(map, n, (const int16_t*)d_disp, width, height, scale, model, poses, sync);
}

int sbm_occ_insert(sbm_occ_map* map, int n, const int16_t* disp, int width, int height, int scale, const sbm_stereo_model* model,
                   const float* poses) {
  const int st = occ_check_insert(map, n, disp, width, height, scale, model, poses);
  if (st != SBM_OK) return st;
  if (map->mode == kOccModeLogOdds) return SBM_ERR_UNSUPPORTED;
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

int sbm_occ_write_binary(const uint64_t* keys, size_t n, double resolution, const char* path) {
  if (!path || (n > 0 && !keys)) return SBM_ERR_NULL;
  if (!std::isfinite(resolution) || !(resolution > 0.)) return SBM_ERR_SIZE;
  std::vector<uint64_t> leaf;
  try {
    leaf.reserve(n);
    for (size_t i = 0; i < n; i++) {
      if (keys[i] >> 48) return SBM_ERR_SIZE;
      leaf.push_back(occ_morton(keys[i]) << 1 | 1);
    }
    std::sort(leaf.begin(), leaf.end());
    leaf.erase(std::unique(leaf.begin(), leaf.end()), leaf.end());
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return occ_write_stream(leaf, resolution, path);
}

int sbm_occ_write_binary_logodds(const uint64_t* keys, const float* logodds, size_t n, double resolution, float occupancy_thres_log,
                                 const char* path) {
  if (!path || (n > 0 && (!keys || !logodds))) return SBM_ERR_NULL;
  if (!std::isfinite(resolution) || !(resolution > 0.) || std::isnan(occupancy_thres_log)) return SBM_ERR_SIZE;
  std::vector<uint64_t> leaf;
  try {
    leaf.reserve(n);
    for (size_t i = 0; i < n; i++) {
      if (keys[i] >> 48 || std::isnan(logodds[i])) return SBM_ERR_SIZE;
      leaf.push_back(occ_morton(keys[i]) << 1 | (logodds[i] >= occupancy_thres_log ? 1 : 0));   // isNodeOccupied
    }
    std::sort(leaf.begin(), leaf.end());
    for (size_t i = 1; i < leaf.size(); i++)
      if (leaf[i] >> 1 == leaf[i - 1] >> 1) return SBM_ERR_SIZE;   // one value per voxel
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  return occ_write_stream(leaf, resolution, path);
}

void sbm_occ_ray_params_default(sbm_occ_ray_params* p) {
  if (!p) return;
  p->prob_hit = 0.7;
  p->prob_miss = 0.4;
  p->clamp_min = 0.1192;
  p->clamp_max = 0.971;
  p->occupancy_thres = 0.5;
  p->max_range = -1.;
}

int sbm_occ_ray_params_validate(const sbm_occ_ray_params* p) { return occ_ray_params_check(p); }

int sbm_occ_ray_logodds(const sbm_occ_ray_params* p, float logodds[5]) {
  if (!logodds) return SBM_ERR_NULL;
  const int st = occ_ray_params_check(p);
  if (st != SBM_OK) return st;
  const double prob[5] = {p->prob_hit, p->prob_miss, p->clamp_min, p->clamp_max, p->occupancy_thres};
  for (int i = 0; i < 5; i++) logodds[i] = occ_logodds(prob[i]);
  return SBM_OK;
}

int sbm_occ_insert_cloud_device(sbm_occ_map* map, size_t n_points, const void* d_xyz, const float* origin,
                                const sbm_occ_ray_params* params, int sync) {
  const int st = occ_check_cloud(map, n_points, d_xyz, origin, params);
  if (st != SBM_OK) return st;
  if ((uintptr_t)d_xyz & 3) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_cloud_run(map, n_points, (const float*)d_xyz, origin, params, sync);
}

int sbm_occ_insert_cloud(sbm_occ_map* map, size_t n_points, const float* xyz, const float* origin, const sbm_occ_ray_params* params) {
  const int st = occ_check_cloud(map, n_points, xyz, origin, params);
  if (st != SBM_OK) return st;
  if (map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  if (n_points) {
    HIPCHK(h, h->occ.io.grow(n_points * 12, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->occ.io.p, xyz, n_points * 12, hipMemcpyHostToDevice, h->stream));
  }
  return occ_cloud_run(map, n_points, h->occ.io.as<float>(), origin, params, 1);
}

int sbm_occ_insert_rays_device(sbm_occ_map* map, int n, const void* d_disp, int width, int height, int scale,
                               const sbm_stereo_model* model, const float* poses, const sbm_occ_ray_params* params, int sync) {
  int st = occ_check_insert(map, n, d_disp, width, height, scale, model, poses);
  if (st == SBM_OK) st = occ_ray_params_check(params);
  if (st != SBM_OK) return st;
  if ((uintptr_t)d_disp & 1) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_planes_run(map, n, (const int16_t*)d_disp, width, height, scale, model, poses, params, sync);
}

int sbm_occ_insert_rays(sbm_occ_map* map, int n, const int16_t* disp, int width, int height, int scale, const sbm_stereo_model* model,
                        const float* poses, const sbm_occ_ray_params* params) {
  int st = occ_check_insert(map, n, disp, width, height, scale, model, poses);
  if (st == SBM_OK) st = occ_ray_params_check(params);
  if (st != SBM_OK) return st;
  if (map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  const size_t bytes = (size_t)n * width * height * sizeof(int16_t);
  HIPCHK(h, h->occ.io.grow(bytes, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->occ.io.p, disp, bytes, hipMemcpyHostToDevice, h->stream));
  return occ_planes_run(map, n, h->occ.io.as<int16_t>(), width, height, scale, model, poses, params, 1);
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

void sbm_occ_query_params_default(sbm_occ_query_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->max_range = -1.;
  p->occupancy_thres_log = 0.0f;
  p->ignore_unknown = 0;
}

int sbm_occ_query_params_validate(const sbm_occ_query_params* p) { return occ_query_params_check(p); }

int sbm_occ_search_device(sbm_occ_map* map, size_t n, const void* d_xyz, float occupancy_thres_log, void* d_state, void* d_value,
                          int sync) {
  if (!map || (n > 0 && (!d_xyz || !d_state))) return SBM_ERR_NULL;
  if (std::isnan(occupancy_thres_log)) return SBM_ERR_SIZE;
  if (n > ((size_t)1 << 30) || ((uintptr_t)d_xyz & 3) || ((uintptr_t)d_state & 3) || ((uintptr_t)d_value & 3)) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_search_run(map, n, (const float*)d_xyz, occupancy_thres_log, (int*)d_state, (unsigned*)d_value, sync);
}

int sbm_occ_search(sbm_occ_map* map, size_t n, const float* xyz, float occupancy_thres_log, int32_t* state, void* value) {
  if (!map || (n > 0 && (!xyz || !state))) return SBM_ERR_NULL;
  if (std::isnan(occupancy_thres_log)) return SBM_ERR_SIZE;
  if (n > ((size_t)1 << 30)) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  if (n) {   // io: n triples, n states, n values
    HIPCHK(h, h->occ.io.grow(n * 20, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->occ.io.p, xyz, n * 12, hipMemcpyHostToDevice, h->stream));
  }
  char* io = h->occ.io.as<char>();
  const int st = occ_search_run(map, n, (const float*)io, occupancy_thres_log, (int*)(io + n * 12), (unsigned*)(io + n * 16), 0);
  if (st != SBM_OK) return st;
  if (n) {
    HIPCHK(h, hipMemcpyAsync(state, io + n * 12, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (value) HIPCHK(h, hipMemcpyAsync(value, io + n * 16, n * 4, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_occ_cast_rays_device(sbm_occ_map* map, size_t n, const void* origins, int shared_origin, const void* d_dirs,
                             const sbm_occ_query_params* params, void* d_status, void* d_end, int sync) {
  const int st = occ_check_cast(map, n, origins, d_dirs, params, d_status);
  if (st != SBM_OK) return st;
  if ((!shared_origin && ((uintptr_t)origins & 3)) || ((uintptr_t)d_dirs & 3) || ((uintptr_t)d_status & 3) || ((uintptr_t)d_end & 3))
    return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_cast_run(map, n, shared_origin ? nullptr : (const float*)origins, shared_origin ? (const float*)origins : nullptr,
                      (const float*)d_dirs, params, (int*)d_status, (float*)d_end, sync);
}

int sbm_occ_cast_rays(sbm_occ_map* map, size_t n, const float* origins, int shared_origin, const float* dirs,
                      const sbm_occ_query_params* params, int32_t* status, float* end) {
  int st = occ_check_cast(map, n, origins, dirs, params, status);
  if (st != SBM_OK) return st;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  char* io = nullptr;
  if (n) {   // io: n directions, n origins, n statuses, n ends
    HIPCHK(h, h->occ.io.grow(n * 40, h->stream));
    io = h->occ.io.as<char>();
    HIPCHK(h, hipMemcpyAsync(io, dirs, n * 12, hipMemcpyHostToDevice, h->stream));
    if (!shared_origin) HIPCHK(h, hipMemcpyAsync(io + n * 12, origins, n * 12, hipMemcpyHostToDevice, h->stream));
  }
  st = occ_cast_run(map, n, shared_origin ? nullptr : (const float*)(io + n * 12), shared_origin ? origins : nullptr, (const float*)io,
                    params, (int*)(io + n * 24), (float*)(io + n * 28), 0);
  if (st != SBM_OK) return st;
  if (n) {
    HIPCHK(h, hipMemcpyAsync(status, io + n * 24, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (end) HIPCHK(h, hipMemcpyAsync(end, io + n * 28, n * 12, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_occ_cast_view_device(sbm_occ_map* map, int width, int height, int scale, const sbm_stereo_model* model, const float* pose,
                             const sbm_occ_query_params* params, void* d_status, void* d_end, int sync) {
  if (!map || !model || !pose || !params || !d_status) return SBM_ERR_NULL;
  if (width <= 0 || height <= 0 || scale <= 0) return SBM_ERR_SIZE;
  const int st = occ_query_params_check(params);
  if (st != SBM_OK) return st;
  if ((size_t)width * height > ((size_t)1 << 30) || (size_t)width * scale > ((size_t)1 << 24) || (size_t)height * scale > ((size_t)1 << 24) ||
      ((uintptr_t)d_status & 3) || ((uintptr_t)d_end & 3))
    return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  OccQuery g;
  occ_query_begin(map, params->max_range, params->occupancy_thres_log, params->ignore_unknown, &g);
  OccView v;
  memset(&v, 0, sizeof(v));
  v.W = width;
  v.H = height;
  v.scale = scale;
  OccPose t;
  memcpy(t.t, pose, sizeof(t.t));
  const unsigned blocks = kOccViewTiled ? (unsigned)(((width + 31) / 32) * (size_t)((height + 7) / 8))
                                        : (unsigned)(((size_t)width * height + 255) / 256);
  return occ_query_run(map, kOccCast, true, sync, [&] {
    hipLaunchKernelGGL(occ_cast_view_kernel, dim3(blocks), dim3(256), 0, h->stream, v, *model, t, g, (int*)d_status, (float*)d_end);
  });
}

// ---- loading a .bt stream ---------------------------------------------------------------------------------------------------
int sbm_occ_binary_info(const void* bytes, size_t n, sbm_occ_binary_header* out) {
  if (!out || (n > 0 && !bytes)) return SBM_ERR_NULL;
  return occ_bt_parse((const uint8_t*)bytes, n, out, nullptr);
}

int sbm_occ_binary_leaves(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, uint8_t* occupied, size_t cap, size_t* count) {
  if (!count || (n > 0 && !bytes) || (cap > 0 && (!first_key || !depth || !occupied))) return SBM_ERR_NULL;
  std::vector<OccBtLeaf> leaves;
  const int st = occ_bt_parse((const uint8_t*)bytes, n, nullptr, &leaves);
  if (st != SBM_OK) return st;
  *count = leaves.size();
  if (leaves.size() > cap) return SBM_ERR_SIZE;
  for (size_t i = 0; i < leaves.size(); i++) {
    const uint64_t c = occ_bt_code(leaves[i]);
    first_key[i] = (uint64_t)occ_unspread(c) << 32 | (uint64_t)occ_unspread(c >> 1) << 16 | occ_unspread(c >> 2);
    depth[i] = occ_bt_depth(leaves[i]);
    occupied[i] = (uint8_t)(leaves[i] & 1);
  }
  return SBM_OK;
}

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
  FILE* f = fopen(path, "rb");
  if (!f) return SBM_ERR_UNSUPPORTED;
  std::vector<uint8_t> data;
  bool ok = true;
  try {
    uint8_t chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) data.insert(data.end(), chunk, chunk + got);
    ok = !ferror(f);
  } catch (const std::bad_alloc&) {
    fclose(f);
    return SBM_ERR_NOMEM;
  }
  fclose(f);
  if (!ok) return SBM_ERR_UNSUPPORTED;
  return occ_load_run(map, data.data(), data.size(), params, sync);
}

// ---- the octree above the voxels ----------------------------------------------------------------------------------------
int sbm_occ_tree_create(sbm_occ_map* map, sbm_occ_tree** out) {
  if (!map || !out) return SBM_ERR_NULL;
  *out = nullptr;
  sbm_occ_tree* t = new (std::nothrow) sbm_occ_tree();
  if (!t) return SBM_ERR_NOMEM;
  memset(t, 0, sizeof(*t));
  t->h = map->h;
  t->map = map;
  t->reading = SBM_OCC_TREE_LOGODDS;
  t->resolution = map->p.resolution;
  *out = t;
  return SBM_OK;
}

void sbm_occ_tree_destroy(sbm_occ_tree* tree) {
  if (!tree) return;
  DeviceScope dscope(tree->h->device);
  dscope.enter();
  hipStreamSynchronize(tree->h->stream);
  release_all(*tree);
  delete tree;
}

int sbm_occ_tree_build(sbm_occ_tree* tree, int reading, const sbm_occ_ray_params* params, int sync) {
  if (!tree || (reading == SBM_OCC_TREE_MAXLIKELIHOOD && !params)) return SBM_ERR_NULL;
  if (reading != SBM_OCC_TREE_LOGODDS && reading != SBM_OCC_TREE_MAXLIKELIHOOD) return SBM_ERR_SIZE;
  if (params) {
    const int st = occ_ray_params_check(params);
    if (st != SBM_OK) return st;
  }
  if (reading == SBM_OCC_TREE_LOGODDS && tree->map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  return occ_tree_build_run(tree, reading, params, sync);
}

int sbm_occ_tree_info(sbm_occ_tree* tree, sbm_occ_tree_counts* info) {
  if (!tree || !info) return SBM_ERR_NULL;
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  const int st = occ_tree_stats(tree);
  if (st != SBM_OK) return st;
  memset(info, 0, sizeof(*info));
  info->voxels = tree->built ? tree->count[kOccDepth] : 0;
  for (int d = 0; d <= kOccDepth; d++) {
    info->nodes_at[d] = tree->host.nodes_at[d];
    info->leaves_at[d] = tree->host.leaves_at[d];
    info->nodes += info->nodes_at[d];
    info->leaves += info->leaves_at[d];
  }
  for (int a = 0; a < 3; a++) {
    info->key_min[a] = (uint16_t)tree->host.kmin[a];
    info->key_max[a] = (uint16_t)tree->host.kmax[a];
  }
  return SBM_OK;
}

int sbm_occ_tree_search_device(sbm_occ_tree* tree, size_t n, const void* d_xyz, int depth, float occupancy_thres_log, void* d_state,
                               void* d_value, void* d_found_depth, int sync) {
  if (!tree || (n > 0 && (!d_xyz || !d_state))) return SBM_ERR_NULL;
  if (occ_tree_depth_check(depth) != SBM_OK || std::isnan(occupancy_thres_log)) return SBM_ERR_SIZE;
  if (n > ((size_t)1 << 30) || ((uintptr_t)d_xyz & 3) || ((uintptr_t)d_state & 3) || ((uintptr_t)d_value & 3) || ((uintptr_t)d_found_depth & 3))
    return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  return occ_tree_search_run(tree, n, (const float*)d_xyz, depth ? depth : kOccDepth, occupancy_thres_log, (int*)d_state,
                             (unsigned*)d_value, (int*)d_found_depth, sync);
}

int sbm_occ_tree_search(sbm_occ_tree* tree, size_t n, const float* xyz, int depth, float occupancy_thres_log, int32_t* state, void* value,
                        int32_t* found_depth) {
  if (!tree || (n > 0 && (!xyz || !state))) return SBM_ERR_NULL;
  if (occ_tree_depth_check(depth) != SBM_OK || std::isnan(occupancy_thres_log)) return SBM_ERR_SIZE;
  if (n > ((size_t)1 << 30)) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = tree->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  if (n) {   // io: n triples, n states, n values, n depths
    HIPCHK(h, h->occ.io.grow(n * 24, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->occ.io.p, xyz, n * 12, hipMemcpyHostToDevice, h->stream));
  }
  char* io = h->occ.io.as<char>();
  const int st = occ_tree_search_run(tree, n, (const float*)io, depth ? depth : kOccDepth, occupancy_thres_log, (int*)(io + n * 12),
                                     (unsigned*)(io + n * 16), (int*)(io + n * 20), 0);
  if (st != SBM_OK) return st;
  if (n) {
    HIPCHK(h, hipMemcpyAsync(state, io + n * 12, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (value) HIPCHK(h, hipMemcpyAsync(value, io + n * 16, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (found_depth) HIPCHK(h, hipMemcpyAsync(found_depth, io + n * 20, n * 4, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_occ_tree_leaves_device(sbm_occ_tree* tree, int max_depth, void* d_keys, void* d_depth, void* d_value, size_t cap, size_t* count) {
  if (!tree || !count || (cap > 0 && (!d_keys || !d_depth))) return SBM_ERR_NULL;
  if (occ_tree_depth_check(max_depth) != SBM_OK) return SBM_ERR_SIZE;
  if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_depth & 3) || ((uintptr_t)d_value & 3)) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  return occ_tree_leaves_run(tree, max_depth ? max_depth : kOccDepth, (unsigned long long*)d_keys, (int*)d_depth, (unsigned*)d_value, cap,
                             count);
}

int sbm_occ_tree_leaves(sbm_occ_tree* tree, int max_depth, uint64_t* keys, int32_t* depth, float* value, size_t cap, size_t* count) {
  if (!tree || !count || (cap > 0 && (!keys || !depth))) return SBM_ERR_NULL;
  if (occ_tree_depth_check(max_depth) != SBM_OK) return SBM_ERR_SIZE;
  sbm_handle* h = tree->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  max_depth = max_depth ? max_depth : kOccDepth;
  int st = occ_tree_stats(tree);
  if (st != SBM_OK) return st;
  const size_t n = occ_tree_leaf_count(tree, max_depth);
  *count = n;
  if (n > cap) return SBM_ERR_SIZE;
  if (!n) return SBM_OK;
  const size_t kb = occ_pad(n * 8), vb = occ_pad(n * 4);
  HIPCHK(h, h->occ.io.grow(kb + 2 * vb, h->stream));
  char* io = h->occ.io.as<char>();
  st = occ_tree_leaves_run(tree, max_depth, (unsigned long long*)io, (int*)(io + kb), (unsigned*)(io + kb + vb), n, count);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpyAsync(keys, io, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(depth, io + kb, n * 4, hipMemcpyDeviceToHost, h->stream));
  if (value) HIPCHK(h, hipMemcpyAsync(value, io + kb + vb, n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_occ_tree_binary_device(sbm_occ_tree* tree, void* d_bytes, size_t cap, size_t* nbytes) {
  if (!tree || !nbytes || (cap > 0 && !d_bytes)) return SBM_ERR_NULL;
  if (tree->reading != SBM_OCC_TREE_MAXLIKELIHOOD && tree->built) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  return occ_tree_binary_run(tree, (uint8_t*)d_bytes, cap, nbytes);
}

int sbm_occ_tree_write_binary(sbm_occ_tree* tree, const char* path) {
  if (!tree || !path) return SBM_ERR_NULL;
  if (tree->reading != SBM_OCC_TREE_MAXLIKELIHOOD && tree->built) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = tree->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  int st = occ_tree_stats(tree);
  if (st != SBM_OK) return st;
  unsigned long long nodes = 0, leaves = 0;
  for (int d = 0; d <= kOccDepth; d++) nodes += tree->host.nodes_at[d], leaves += tree->host.leaves_at[d];
  const size_t bytes = (size_t)(2 * (nodes - leaves));
  std::vector<uint8_t> body;
  try {
    body.resize(bytes);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  if (bytes) {
    size_t got = 0;
    HIPCHK(h, h->occ.io.grow(bytes, h->stream));
    st = occ_tree_binary_run(tree, h->occ.io.as<uint8_t>(), bytes, &got);
    if (st != SBM_OK) return st;
    HIPCHK(h, hipMemcpyAsync(body.data(), h->occ.io.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  return occ_write_file(body, (size_t)nodes, tree->resolution, path);
}

}  // extern "C"
