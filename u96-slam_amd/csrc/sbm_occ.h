// sbm_occ.h -- what more than one file of the occupancy family (sbm_occupancy.hip, sbm_occ_*.hip) needs, each thing once. Internal.
// The first part is plain C++, for the host-only sbm_occ_bt.hip and sbm_occ_ot_host.hip; the rest needs HIP (gfx950 only). Nothing here contracts a
// multiply-add: every helper with float or double steps carries the pragma.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/sbm.h"
#ifdef __HIP__
#include <algorithm>
#include <new>
#include "sbm_consume_math.h"
#include "sbm_handle.h"
#define SBM_OCC_HD __host__ __device__ __forceinline__
#else
#define SBM_OCC_HD inline
#endif

namespace sbm {
// every third bit of a 16-bit key; unspread is its inverse
SBM_OCC_HD unsigned long long occ_spread(unsigned long long x) {
  x &= 0xFFFFull;
  x = (x | x << 32) & 0x001F00000000FFFFull;
  x = (x | x << 16) & 0x001F0000FF0000FFull;
  x = (x | x << 8) & 0x100F00F00F00F00Full;
  x = (x | x << 4) & 0x10C30C30C30C30C3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
SBM_OCC_HD unsigned occ_unspread(unsigned long long x) {
  x &= 0x1249249249249249ull;
  x = (x ^ x >> 2) & 0x10C30C30C30C30C3ull;
  x = (x ^ x >> 4) & 0x100F00F00F00F00Full;
  x = (x ^ x >> 8) & 0x001F0000FF0000FFull;
  x = (x ^ x >> 16) & 0x001F00000000FFFFull;
  x = (x ^ x >> 32) & 0xFFFFull;
  return (unsigned)x;
}

SBM_OCC_HD unsigned long long occ_pack(unsigned k0, unsigned k1, unsigned k2) {
  return (unsigned long long)k0 << 32 | (unsigned long long)k1 << 16 | k2;   // a packed key
}
// its Morton code, computeChildIdx from the top bit down: x in bit 0, y in bit 1, z in bit 2 of every triple; and the key of a code
SBM_OCC_HD unsigned long long occ_code(unsigned k0, unsigned k1, unsigned k2) {
  return occ_spread(k0) | occ_spread(k1) << 1 | occ_spread(k2) << 2;
}
SBM_OCC_HD unsigned long long occ_key_of_code(unsigned long long code) {
  return occ_pack(occ_unspread(code), occ_unspread(code >> 1), occ_unspread(code >> 2));
}

// A leaf as the .bt parser hands it on and the device takes it: first Morton code of the cube << 8 | depth << 1 | occupied
typedef unsigned long long OccBtLeaf;
inline uint64_t occ_bt_code(OccBtLeaf l) { return l >> 8; }
inline int occ_bt_depth(OccBtLeaf l) { return (int)(l >> 1 & 31); }
#pragma GCC visibility push(hidden)   // sbm_occ_bt.hip: the parser (leaves in stream order) and the file of a written body
int occ_bt_parse(const uint8_t* b, size_t n, sbm_occ_binary_header* info, std::vector<OccBtLeaf>* leaves, bool bounds = true);
int occ_write_file(const std::vector<uint8_t>& body, size_t nodes, double resolution, const char* path);
int occ_read_file(const char* path, std::vector<uint8_t>* data);
int occ_bt_header(const uint8_t* b, size_t n, size_t* pos, std::string* id, uint64_t* size, double* res);   // readHeader
// sbm_occ_ot_host.hip, the .ot stream: its header alone (-> where the body begins), the whole host parse (leaf words without the occupied bit, and the
// leaves' float bits), and the file. want_res > 0: what the file's res must equal
int occ_ot_head(const uint8_t* b, size_t n, double want_res, sbm_occ_ot_header* info, size_t* body, bool stamped = false);   // stamped: the id has to be OcTreeStamped
int occ_ot_parse(const uint8_t* b, size_t n, double want_res, sbm_occ_ot_header* info, std::vector<OccBtLeaf>* words,
                 std::vector<uint32_t>* values, bool bounds, bool stamped = false);
int occ_ot_write_file(const std::vector<uint8_t>& body, size_t nodes, double resolution, const char* path, const char* id = "OcTree");
double occ_printed_resolution(double resolution);   // what the writers print for a resolution (%g), read back
// sbm_occ_color_host.hip, the ColorOcTree stream: as the three above with eight bytes per node and the leaves' colour words
int occ_color_ot_parse(const uint8_t* b, size_t n, double want_res, sbm_occ_ot_header* info, std::vector<OccBtLeaf>* words,
                       std::vector<uint32_t>* values, std::vector<uint32_t>* colors, bool bounds);
int occ_color_ot_write_file(const std::vector<uint8_t>& body, size_t nodes, double resolution, const char* path);
#pragma GCC visibility pop
// The edits' host arithmetic (sbm_occ_edit.hip; tools/occupancy_edit_sanitize.cpp runs it under the sanitizers). A batch of n items
// goes through in chunks of SBM_OCC_EDIT_CHUNK, in item order: how many, and the items [*begin, *begin + *count) of chunk c
inline size_t occ_edit_chunks(size_t n) { return n / SBM_OCC_EDIT_CHUNK + (n % SBM_OCC_EDIT_CHUNK != 0); }
inline void occ_edit_chunk(size_t n, size_t c, size_t* begin, size_t* count) {
  *begin = c * (size_t)SBM_OCC_EDIT_CHUNK;
  *count = *begin >= n ? 0 : n - *begin < (size_t)SBM_OCC_EDIT_CHUNK ? n - *begin : (size_t)SBM_OCC_EDIT_CHUNK;
}
// deleteNode's depth (0 means 16) -> the bits of a packed key in which a voxel has to agree with the given key: the top `depth`
// bits of each component. false: a depth outside 0..16
inline bool occ_depth_mask(int depth, uint64_t* mask) {
  if (depth < 0 || depth > 16) return false;
  const uint64_t m = (0xFFFFull << (16 - (depth ? depth : 16))) & 0xFFFFull;
  *mask = m << 32 | m << 16 | m;
  return true;
}
// a key box as the box delete's kernel takes it: is the packed key inside (both ends inclusive; min > max on an axis: nothing is)
SBM_OCC_HD bool occ_key_in_box(unsigned long long key, const unsigned kmin[3], const unsigned kmax[3]) {
  const unsigned k0 = (unsigned)(key >> 32) & 0xFFFF, k1 = (unsigned)(key >> 16) & 0xFFFF, k2 = (unsigned)key & 0xFFFF;
  return k0 >= kmin[0] && k0 <= kmax[0] && k1 >= kmin[1] && k1 <= kmax[1] && k2 >= kmin[2] && k2 <= kmax[2];
}

// The planners' host arithmetic (sbm_occ_planner.hip; tools/occupancy_planner_sanitize.cpp runs it under the sanitizers), octomap's
// own statements in double and float. A translation unit that uses it is built without contraction.
constexpr size_t kOccUnknownMaxCells = (size_t)1 << 30;
// keyToCoord(key, depth), OcTreeBaseImpl.hxx:394-405: the root, the voxels, between
inline double occ_key_to_coord(unsigned key, int depth, double resolution) {
  if (depth == 0) return 0.0;
  if (depth == 16) return ((double)((int)key - 32768) + 0.5) * resolution;
  const double span = (double)(1 << (16 - depth));
  return (__builtin_floor(((double)key - 32768.0) / span) + 0.5) * (resolution * span);   // getNodeSize(depth) is resolution * span
}
// The UNCHECKED coordToKey(coordinate, depth) of OcTreeBaseImpl.hxx:297-306 before its cast to 16 bits, which wraps there. false
// where the key leaves 0..65535 (a NaN among them): the divergence include/sbm.h states
inline bool occ_coord_to_key_at(double factor, float coord, int depth, unsigned* key) {
  const double f = __builtin_floor(factor * (double)coord);
  if (!(f >= -32768.0 && f < 32768.0)) return false;
  const int diff = 16 - depth, keyval = (int)f;
  const int k = diff ? (keyval & ~((1 << diff) - 1)) + (1 << (diff - 1)) + 32768 : keyval + 32768;   // (keyval >> diff) << diff
  if (k < 0 || k > 65535) return false;
  *key = (unsigned)k;
  return true;
}
// getUnknownLeafCenters up to its loops (OcTreeBaseImpl.hxx:1046-1062): the clamped lower corner, the step and the step counts.
// A count that is negative or NaN (pmax below pmin on an axis; octomap's cast to unsigned is undefined there) is 0.
struct OccUnknownPlan {
  float lo[3], step;
  uint32_t steps[3];
};
inline int occ_unknown_plan(double resolution, const float pmin[3], const float pmax[3], int depth, OccUnknownPlan* p) {
  if (depth < 0 || depth > 16) return SBM_ERR_SIZE;
  depth = depth ? depth : 16;
  const double factor = 1. / resolution;
  p->step = (float)(resolution * (double)(1 << (16 - depth)));   // resolution * pow(2, tree_depth - depth)
  size_t cells = 1;
  float hi[3];
  for (int a = 0; a < 3; a++) {
    unsigned klo, khi;
    if (!occ_coord_to_key_at(factor, pmin[a], depth, &klo) || !occ_coord_to_key_at(factor, pmax[a], depth, &khi)) return SBM_ERR_SIZE;
    p->lo[a] = (float)occ_key_to_coord(klo, depth, resolution);
    hi[a] = (float)occ_key_to_coord(khi, depth, resolution);
  }
  for (int a = 0; a < 3; a++) {
    const float diff = hi[a] - p->lo[a];
    const float n = __builtin_floorf(diff / p->step);
    p->steps[a] = n >= 1.0f && n <= 65536.0f ? (uint32_t)n : 0u;   // two keys of 0..65535 are never further apart
    cells *= p->steps[a];                                          // at most 2^48
  }
  return cells > kOccUnknownMaxCells ? SBM_ERR_UNSUPPORTED : SBM_OK;
}
// One axis of its loops: out[i] is the running float sum after i + 1 increments, which is what the loop asks and reports
inline void occ_unknown_axis(float start, float step, uint32_t n, float* out) {
  volatile float p = start;   // every sum is rounded to float before the next
  for (uint32_t i = 0; i < n; i++) {
    p = p + step;
    out[i] = p;
  }
}
// getMetricMin / getMetricMax (the const forms, OcTreeBaseImpl.hxx:959-1013) from the smallest and largest centre key among the
// leaves of one depth: keyToCoord is non-decreasing in the key, and so are its rounded sums with the depth's half size, so the
// extreme keys of a depth give that depth's extreme bounds, bit for bit. lo / hi come in with what the depths so far gave.
inline void occ_metric_fold(int depth, const unsigned kmin[3], const unsigned kmax[3], double resolution, double lo[3], double hi[3]) {
  const double half = (resolution * (double)(1 << (16 - depth))) / 2.0;
  for (int a = 0; a < 3; a++) {
    const double x = occ_key_to_coord(kmin[a], depth, resolution) - half, y = occ_key_to_coord(kmax[a], depth, resolution) + half;
    if (x < lo[a]) lo[a] = x;
    if (y > hi[a]) hi[a] = y;
  }
}

#ifdef __HIP__
constexpr unsigned long long kOccEmpty = ~0ull;
constexpr uint32_t kOccMaxProbe = 1024;
constexpr int kOccTile = 1024;       // keys per workgroup of a radix pass, children per workgroup of a tree level
constexpr int kOccDepth = 16;
enum { kOccModeNone, kOccModeHits, kOccModeLogOdds };
constexpr int kOccMaxSteps = 3 * 65536;   // of one ray: each step moves one key by one on one axis
constexpr unsigned kOccFree = 1, kOccOccupied = 2;   // flag word of a slot within one scan
constexpr unsigned kOccCreated = 4;                  // ... under change detection: the scan claimed the slot
enum : uint8_t { kOccChangeNone, kOccChangeCreated, kOccChangeFlipped };   // change state of a slot (octomap's changed_keys: true, false)
constexpr unsigned kOccCollapsed = 1u << 8;   // info word of a tree node: bits 0-7 child mask, bit 8 collapsed,
constexpr int kOccTopShift = 10;              // bits 10-14 the depth of the shallowest collapsed node at or above it, or
constexpr unsigned kOccNoTop = 31;            // kOccNoTop
constexpr unsigned kOccInnerTag = 1u << 31;   // payload of a selected node: its index among the leaves, or tag | index above them
constexpr unsigned kOccWhite = 0x00FFFFFFu;   // colour word of a slot (r | g << 8 | b << 16): octomap's "no colour set"

struct OccCounters {
  unsigned long long overflow;   // points (log-odds mode: cells) that found the table full
  unsigned size;                 // occupied slots
  unsigned cursor;               // compaction cursor of a fetch
  unsigned touched[2];           // log-odds mode: slots the running scan has touched, in [scan & 1]; the other is zero
};
struct OccPose { float t[12]; };     // one plane's pose; the cloud form passes its origin in t[3], t[7], t[11]
struct OccGeom {                     // the planes of an insert
  int W, H, scale;
  float range_max_sqrd;          // range_max * range_max, formed in float on the host as main.cpp:501 does
  double factor;                 // 1. / resolution
  uint32_t mask, max_probe;
};
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

// Stage times: the family's calls share the clock's marks, and each keeps the other stages' last times (occ_clock_start).
enum OccStage { kOccInsert, kOccFetch, kOccRaysMark, kOccRaysApply, kOccSearch, kOccCast, kOccTreeBuild, kOccTreeQuery, kOccLoad, kOccStageCount };
enum OccMark { kOccBegin, kOccEnd, kOccMid, kOccMarkCount };

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
__device__ __forceinline__ float occ_key_coord(unsigned key, double resolution) {   // keyToCoord, then point3d's float
#pragma clang fp contract(off)
  return (float)(((double)((int)key - 32768) + 0.5) * resolution);
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

// One axis of a 3-D DDA's initialisation. The one difference between its two sources: the border's half cell is rounded to
// float before it is added (kHalfInFloat: computeRayKeys) or added in double (castRay).
template <bool kHalfInFloat>
__device__ __forceinline__ void occ_dda_axis(float dir, unsigned key, float origin, double resolution, int* step, double* tmax,
                                             double* tdelta) {
#pragma clang fp contract(off)
  *step = dir > 0.0f ? 1 : dir < 0.0f ? -1 : 0;
  *tmax = *tdelta = 1.7976931348623157e308;   // std::numeric_limits<double>::max()
  if (*step) {
    double border = ((double)((int)key - 32768) + 0.5) * resolution;   // keyToCoord
    if (kHalfInFloat) border += (double)(float)((double)*step * resolution * 0.5);
    else border += (double)*step * resolution * 0.5;
    *tmax = (border - (double)origin) / (double)dir;
    *tdelta = resolution / fabs((double)dir);
  }
}

// The UNCHECKED coordToKey of computeDiscreteUpdate on one axis (OcTreeBaseImpl.h:357-359): the sum wraps modulo 65536. false
// where the coordinate is not finite or its floor fits no int, where the reference's cast is undefined.
__device__ __forceinline__ bool occ_axis_wrapped(double factor, float coord, unsigned* k) {
#pragma clang fp contract(off)
  const double f = floor(factor * (double)coord);
  if (!(f >= -2147483648.0 && f < 2147483648.0)) return false;
  *k = ((unsigned)(int)f + 32768u) & 0xFFFFu;
  return true;
}

// Finds the key's slot or claims an empty one: a walk of at most max_probe slots from the key's hash, a relaxed load of each, a
// 64-bit compare-and-swap on an empty one. false: no slot. It counts nothing: a caller told `claimed` owes OccCounters::size one.
__device__ __forceinline__ bool occ_find_or_claim(unsigned long long* keys, unsigned long long key, uint32_t mask, uint32_t max_probe,
                                                  uint32_t* at, bool* claimed) {
  uint32_t slot = occ_hash(key, mask);
  for (uint32_t probe = 0; probe < max_probe; probe++, slot = (slot + 1) & mask) {
    unsigned long long cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kOccEmpty) {
      cur = atomicCAS(&keys[slot], kOccEmpty, key);
      if (cur == kOccEmpty) {
        *claimed = true;
        cur = key;
      }
    }
    if (cur == key) {
      *at = slot;
      return true;
    }
  }
  return false;
}

// What the batches by key share (sbm_occ_edit.hip, sbm_occ_color.hip)
constexpr unsigned long long kOccKeyBits = (1ull << 48) - 1;   // a packed key; the radix sort orders these bits
constexpr uint32_t kOccNoSlot = ~0u;
// The key's slot, without claiming: the walk of occ_find_or_claim, which ends at the first empty slot.
__device__ __forceinline__ bool occ_find(const unsigned long long* keys, unsigned long long key, uint32_t mask, uint32_t max_probe,
                                         uint32_t* at) {
  uint32_t slot = occ_hash(key, mask);
  for (uint32_t probe = 0; probe < max_probe; probe++, slot = (slot + 1) & mask) {
    const unsigned long long cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == key) {
      *at = slot;
      return true;
    }
    if (cur == kOccEmpty) return false;
  }
  return false;
}

// `count` lanes of the wavefront add one each: one atomic by the first lane. EVERY lane has to reach this call.
template <class T> __device__ __forceinline__ void occ_wave_count(bool count, T* counter) {
  const unsigned long long counting = __ballot(count);
  if (counting && (threadIdx.x & 63) == 0) atomicAdd(counter, (T)__popcll(counting));
}

// The wavefront's append to a list: one atomic add on the list's counter for all the lanes with `take`, each of which gets its
// index (the others' means nothing). EVERY lane of the wavefront has to reach this call: it ballots and reads a lane.
__device__ __forceinline__ unsigned occ_wave_append(bool take, unsigned* counter) {
  const unsigned long long taking = __ballot(take);
  if (!taking) return 0;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)taking) - 1;
  unsigned base = 0;
  if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(taking));
  base = __builtin_amdgcn_readlane(base, leader);
  return base + __popcll(taking & ((1ull << lane) - 1));
}

// The wavefront's minimum / maximum in every lane. EVERY lane of the wavefront has to reach the call.
__device__ __forceinline__ unsigned occ_wave_min(unsigned v) {
  for (int o = 32; o; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ unsigned occ_wave_max(unsigned v) {
  for (int o = 32; o; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
  return v;
}

// A move of the table (sbm_occ_grow.hip: into a larger one; sbm_occ_edit.hip: into one of the same size without the removed slots)
struct OccRehash {
  const unsigned long long* old_keys;
  const unsigned* old_vals;
  const unsigned* old_flags;       // null in hit mode
  const uint8_t* old_change;       // null where detection was never enabled
  const unsigned* old_colors;      // null on a map without colours (sbm_occ_color.hip)
  uint32_t old_slots;
  unsigned long long* keys;
  unsigned* vals;
  unsigned* flags;
  uint8_t* change;
  unsigned* colors;
  unsigned* touched;
  uint32_t mask, max_probe, slots;
  uint32_t parity;                 // which of OccCounters::touched the running scan counts in
  OccCounters* ctr;
};
// One lane of a move, old slot i with `key` (kOccEmpty: nothing to move). EVERY lane of the wavefront has to reach this call.
// old_stamps / stamps: the stamp words of a stamped map (sbm_occ_stamp.hip), which the stamped forms of the two move kernels pass;
// they are arguments of their own, so that the kernels of a map without stamps are what they were.
__device__ __forceinline__ void occ_move_lane(const OccRehash& r, uint32_t i, unsigned long long key, const unsigned* old_stamps = nullptr,
                                              unsigned* stamps = nullptr) {
  bool listed = false;
  uint32_t slot = 0;
  if (key != kOccEmpty) {
    bool claimed = false;
    if (occ_find_or_claim(r.keys, key, r.mask, r.max_probe, &slot, &claimed)) {
      r.vals[slot] = r.old_vals[i];
      const unsigned f = r.old_flags ? r.old_flags[i] : 0;
      if (f) {
        r.flags[slot] = f;
        listed = true;
      }
      if (r.old_change) {
        const uint8_t s = r.old_change[i];
        if (s != kOccChangeNone) r.change[slot] = s;
      }
      if (r.old_colors) r.colors[slot] = r.old_colors[i];
      if (old_stamps) stamps[slot] = old_stamps[i];
    } else {   // a probe walk of the new table that ends without a slot: the voxel is lost, and counted as lost
      atomicAdd(&r.ctr->overflow, 1ull);
      atomicSub(&r.ctr->size, 1u);
    }
  }
  const uint32_t at = occ_wave_append(listed, &r.ctr->touched[r.parity]);   // every lane is here
  if (listed && at < r.slots) r.touched[at] = slot;
}

constexpr size_t occ_pad = 256;   // the family's alignment: arrays that share a buffer begin on it (Carve, sbm_carve.h)
#pragma GCC visibility push(hidden)   // host functions that cross files (these: sbm_occupancy.hip). Hidden, as the two above and
// unlike the rest of the project's, so that the family's internal names stay out of what the library exports
int occ_read_counters(sbm_occ_map* map, OccCounters* c);
int occ_clear(sbm_occ_map* map);
void occ_probe(const sbm_occ_map* map, uint32_t* mask, uint32_t* max_probe);   // of a walk over the table's slots
int occ_check_insert(const sbm_occ_map* map, int n, const void* disp, int width, int height, int scale, const sbm_stereo_model* model,
                     const float* poses);
hipError_t occ_clock_start(sbm_handle* h, int a, int b);   // a call begins that times stages a and b (the same for one)
int occ_overflow_status(sbm_occ_map* map, int sync);       // what a call that wrote the table returns
// The map's n occupied slots -> dense (key, word) arrays in no order
int occ_compact_run(sbm_occ_map* map, uint32_t n, unsigned long long* d_keys, unsigned* d_vals);
// LSD radix sort of n (48-bit key, 32-bit payload) pairs, 8 bits per pass: from kk[0] / vv[0] through kk[1] / vv[1], and the
// even number of passes ends in kk[0] / vv[0]. hist: 256 counts per tile of kOccTile keys.
int occ_sort_run(sbm_handle* h, unsigned long long* const kk[2], unsigned* const vv[2], uint32_t n, unsigned* hist);
float occ_logodds(double p);   // these three are in sbm_occ_rays.hip
int occ_ray_params_check(const sbm_occ_ray_params* p);
int occ_logodds_alloc(sbm_occ_map* map);   // what the log-odds mode keeps beside the table
bool occ_axis_host(double factor, float coord, unsigned* k);   // occ_axis on the host (sbm_occ_options.hip)
// sbm_occ_grow.hip. The map into a table for `capacity` voxels (more than it has, at most 2^30): everything a slot holds moves with its key,
// and the running scan's touched list is rebuilt from the flag words. A refused allocation leaves the map as it was.
int occ_rehash(sbm_occ_map* map, size_t capacity);
// The same move in two steps, for a caller that must know the new table exists before it changes anything: the buffers of a table
// of `slots` slots beside the map's (a refused allocation frees what it got; the error is in last_hip), then the move itself into a
// table for `capacity` voxels. remove (null: nothing), one byte per old slot: the slots that stay behind, `removed` of them, which
// leave the size counter. *c: the counters after the move. The buffers are released either way.
struct OccMoveBufs { DevBuf keys, vals, flags, touched, change, color, stamp; uint32_t slots; };
int occ_move_alloc(sbm_occ_map* map, uint32_t slots, OccMoveBufs* b);
int occ_move_run(sbm_occ_map* map, size_t capacity, OccMoveBufs* b, const uint8_t* remove, unsigned removed, OccCounters* c);
void occ_move_release(OccMoveBufs* b);
void occ_remove_launch(sbm_handle* h, const OccRehash& r, const uint8_t* remove, unsigned removed, const unsigned* old_stamps, unsigned* stamps);   // sbm_occ_edit.hip: the move that leaves slots behind
bool occ_can_reserve(const sbm_occ_map* map, size_t voxels);   // growth is on and its ceiling admits so many voxels
// A growing map after a launch that claimed keys (MARK, the hit insert's claim pass): reads the counters into *c and grows the
// table if cells were lost (overflow above `before`) or the size has passed the capacity. *again: cells were lost and the table
// grew, the overflow counter is back at `before`, and the caller launches the same claims again and calls this again. Where the
// ceiling or an allocation stops the growth the lost cells stay counted and *again is false.
int occ_grow_settle(sbm_occ_map* map, unsigned long long before, OccCounters* c, bool* again);
int occ_overflow_before(sbm_occ_map* map, unsigned long long* before);   // the overflow counter as a launch on a growing map finds it
int occ_set_overflow(sbm_occ_map* map, unsigned long long value);       // in stream order
// The hit insert's claim pass over m planes (at most the 64 of one insert launch) with their poses: keys claimed, no hit added
int occ_claim_launch(sbm_occ_map* map, const int16_t* d_disp, const OccGeom& g, const sbm_stereo_model* model, const float* poses, int m);
OccLevel occ_tree_level(const sbm_occ_tree* t, int d);   // these two are in sbm_occ_tree.hip: depth d of a built tree (empty levels for
int occ_tree_stats(sbm_occ_tree* t);                     // one that is not), and the counts of the last build into t->host, read once
int occ_ot_rank_run(sbm_occ_tree* t, uint32_t n, const unsigned** order);   // sbm_occ_ot.hip: the node at every pre-order rank of the pruned tree
int occ_color_tree_run(sbm_occ_tree* t);   // sbm_occ_color.hip: a colour word per node of the tree just built, over a map with colours
// A selection of n of the tree's nodes as (first Morton code of the cube, where the node is) pairs appended at the tree's cursor
// (occ_tree_select_kernel and its siblings), between these two: begin places the sort's arrays beside d_keys / d_depth and zeroes
// the cursor, end sorts the pairs and turns them in place into centre keys, depths and values
struct OccSelection {
  unsigned long long* kk[2];
  unsigned* vv[2];
  uint32_t n;
};
int occ_tree_select_begin(sbm_occ_tree* t, uint32_t n, unsigned long long* d_keys, int* d_depth, OccSelection* s);
int occ_tree_select_end(sbm_occ_tree* t, const OccSelection& s, unsigned* d_value);
// The radix sort's second key / payload arrays for n pairs in the handle's sort buffer and, where asked, a first payload array
inline hipError_t occ_sort_carve(sbm_handle* h, size_t n, unsigned long long** keys, unsigned** vals, unsigned** first_vals = nullptr) {
  return carve(h->occ.sort, h->stream, [&](Carve& c) {
    *keys = c.take<unsigned long long>(n), *vals = c.take<unsigned>(n);
    if (first_vals) *first_vals = c.take<unsigned>(n);
  }, occ_pad);
}
#pragma GCC visibility pop

// Times `stage` of a query around `launch` (-> status; the error of its last launch is looked at here). A query changes nothing
// and reports no overflow, so with sync it only waits for the stream.
template <class Launch> int occ_timed_run(sbm_handle* h, int stage, bool any, int sync, Launch launch) {
  StageClock& clk = h->occ.clock;
  HIPCHK(h, occ_clock_start(h, stage, stage));
  if (any) {
    HIPCHK(h, clk.mark(kOccBegin, h->stream));
    const int st = launch();
    if (st != SBM_OK) return st;
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, clk.mark(kOccEnd, h->stream));
    HIPCHK(h, clk.add(stage, kOccBegin, kOccEnd));
  }
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}
// The host form of a point search through the handle's staging: n triples in; n states, n values and (depths: a tree's) n found
// depths out, each copied where the caller wants it. search(d_xyz, d_state, d_value, d_found) enqueues the query (-> status).
template <class Search> int occ_search_host(sbm_handle* h, size_t n, const float* xyz, bool depths, int32_t* state, void* value,
                                            int32_t* found_depth, Search search) {
  struct { float* xyz; int* state; unsigned* value; int* found; } io = {};
  if (n) {
    HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& c) {
      io = {c.take<float>(n * 3), c.take<int>(n), c.take<unsigned>(n), c.take<int>(depths ? n : 0)};
    }, occ_pad));
    HIPCHK(h, hipMemcpyAsync(io.xyz, xyz, n * 12, hipMemcpyHostToDevice, h->stream));
  }
  const int st = search(io.xyz, io.state, io.value, io.found);
  if (st != SBM_OK) return st;
  if (n) {
    HIPCHK(h, hipMemcpyAsync(state, io.state, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (value) HIPCHK(h, hipMemcpyAsync(value, io.value, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (found_depth) HIPCHK(h, hipMemcpyAsync(found_depth, io.found, n * 4, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}
// The body of a written tree through the handle's staging: `bytes` of it from run(d_bytes, &got) (-> status) into *body.
template <class Run> int occ_body_host(sbm_handle* h, size_t bytes, std::vector<uint8_t>* body, Run run) {
  try {
    body->resize(bytes);
  } catch (const std::bad_alloc&) {
    return SBM_ERR_NOMEM;
  }
  if (!bytes) return SBM_OK;
  size_t got = 0;
  HIPCHK(h, h->occ.io.grow(bytes, h->stream));
  const int st = run(h->occ.io.as<uint8_t>(), &got);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpyAsync(body->data(), h->occ.io.p, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}
#endif  // __HIP__

}  // namespace sbm

#ifdef __HIP__
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
  // insert options of the log-odds mode (sbm_occ_options.hip); sbm_occ_reset keeps the switches and the box
  bool use_bbx, detect;         // useBBXLimit, enableChangeDetection
  float bbx_min[3], bbx_max[3];
  unsigned bbx_min_key[3], bbx_max_key[3];
  sbm::DevBuf change;           // from the first enable: one byte of change state per slot
  sbm::DevBuf dedupe;           // from the first discretised insert: one scan's key set, key list and count
  // growth (sbm_occ_grow.hip); sbm_occ_reset keeps the switch and the ceiling
  bool grow;                    // sbm_occ_set_growth
  size_t max_capacity;          // its ceiling in voxels; 0: the create limit
  size_t size_bound;            // hit mode: what the host can say the size does not exceed without reading it (launched points add up)
  bool overflow_known;          // `overflow` below is the device's counter: only a growing map keeps this up
  unsigned long long overflow;
  unsigned long long grown, moved, redone;   // tables grown, slots moved, scans or launches redone so far
  // edits (sbm_occ_edit.hip)
  sbm::DevBuf edit, edit_mask;  // from the first edit or delete: its counts; from the first call that may delete: the removal
                                // mask, one byte per slot, clear between calls
  unsigned long long edit_items;   // of the last edit or delete call
  // colours (sbm_occ_color.hip)
  sbm::DevBuf color, color_counts;   // from the first colour call: one colour word per slot, kOccWhite where none is set; its counts
  unsigned long long color_items;    // of the last colour call
  // time stamps (sbm_occ_stamp.hip)
  sbm::DevBuf stamp, stamp_count;    // from sbm_occ_stamp_enable: one uint32 per slot, 0 where nothing stamped; the degrade's count
  uint32_t clock;                    // the map's clock: what a stamping call writes (sbm_occ_stamp_set_time)
  template <class F> void each(F f) { f(keys); f(hits); f(ctr); f(flags); f(touched); f(change); f(dedupe); f(edit); f(edit_mask); f(color); f(color_counts); f(stamp); f(stamp_count); }
};

struct sbm_occ_tree {
  sbm_handle* h;
  sbm_occ_map* map;            // read by a build only
  bool built, have_stats;      // levels are valid; `host` holds the last build's counts
  bool ot_ranked;              // `ot` holds this build's pre-order ranks: filled by the first .ot call after a build
  bool have_metric;            // `metric` holds this build's metric bounds (sbm_occ_planner.hip): filled by the first call after a build
  double metric[6];            // min x y z, max x y z
  int reading;
  double resolution;
  unsigned cmax;               // float bits of clamp max, what .bt calls occupied
  uint32_t count[17];          // nodes per depth, pruned or not; count[16] is the voxels
  size_t off[16], inner_total; // where depth d begins among the nodes above the leaves, and how many those are
  sbm::OccTreeStats host;
  sbm::DevBuf leaf, node;      // depth 16: code, value, parent, info (20 B per voxel); above: code, value, parent, info, first
                               // child, subtree count, rank (32 B per node)
  sbm::DevBuf stats, tiles;    // OccTreeStats; head counts per tile of the level being built
  sbm::DevBuf ot;              // .ot writes only (sbm_occ_ot.hip): per node above the leaves its subtree's nodes and its pre-order
                               // rank among all nodes of the pruned tree, then the node at every rank
  bool colored;                // `color` holds this build's colour words (sbm_occ_color.hip): the map had colours when it was built
  sbm::DevBuf color;           // a colour word per voxel, then per node above them in the order of `node`
  bool stamped;                // `stamp` holds this build's stamps (sbm_occ_stamp.hip): the map had stamps when it was built, and the
                               // structure is octomap's STAMPED pruned tree
  sbm::DevBuf stamp;           // a stamp per voxel, then per node above them in the order of `node`
  template <class F> void each(F f) { f(leaf); f(node); f(stats); f(tiles); f(ot); f(color); f(stamp); }
};
// where the two parts of a built tree's stamps are (the layout of the build, placed again with its counts)
inline void occ_tree_stamps(const sbm_occ_tree* t, unsigned** leaf, unsigned** node) {
  sbm::Carve c{t->stamp.as<char>(), 0, sbm::occ_pad};
  *leaf = c.take<unsigned>(t->count[sbm::kOccDepth]);
  *node = c.take<unsigned>(t->inner_total);
}
#endif
