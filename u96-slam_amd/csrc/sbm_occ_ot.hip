// sbm_occ_ot.hip -- the .ot stream of the occupancy map on the device (include/sbm.h, "occupancy map: the .ot format"):
// AbstractOcTree::write of a built LOGODDS tree and AbstractOcTree::read into a map.  gfx950.
// Write: the tree ranks only its non-leaf nodes, so the first .ot call of a build ranks every node of the pruned tree in pre-order
// (one bottom-up pass of subtree node counts, one top-down pass that also stores the node of every rank); the body is then
// mapped by rank.
//   occ_ot_count       a level's nodes -> the nodes of the pruned tree in their subtrees
//   occ_ot_rank        one lane per parent: the ranks of its children, and which node stands at each of those ranks
//   occ_ot_body        one node per lane in rank order; a workgroup's 1280 bytes go through LDS and leave as whole dwords
// Load: every record is five bytes at 5 i, so the stream is parsed on the device.
//   occ_ot_sums / occ_ot_tiles / occ_ot_scan   D[i + 1] = D[i] + popcount(mask[i]) - 1, the pending child slots before a record, and
//                      the leaves before it: per tile of 1024 records its sums, one workgroup scans those, each tile scans itself
//   occ_ot_minima      minima of D per 16 records, and of those per 16, up to one value
//   occ_ot_parent      the largest j < i with D[j] <= D[i] through that hierarchy, and the child index of i under it
//   occ_ot_leaf        one lane per leaf record walks up at most 16 parents: first Morton code, depth, value bits, volume
//   occ_ot_vol_sums / occ_ot_tiles / occ_ot_vol_scan   the leaf volumes 8^(16-d) into the prefix array of the expansion
//   occ_ot_expand      occ_load_kernel's shape with the leaf's own float as the stored word
// Every loop has a bound that does not depend on the stream being well formed, and every index is clamped to its array.
#include <stdio.h>
#include <stdlib.h>

#include "sbm_occ.h"

namespace sbm {

constexpr int kOtFan = SBM_OCC_OT_FAN;          // entries per tile of the minima hierarchy
constexpr int kOtTile = SBM_OCC_OT_SCAN_TILE;   // records per workgroup of a scan: 256 threads, 4 records each
constexpr int kOtMaxLevels = 8;                 // 16^7 = 2^28 records, the most the device parse takes
constexpr uint64_t kOtMaxRecords = (uint64_t)1 << 28;
constexpr unsigned long long kOtVolCap = 1ull << 62;   // where the voxel total saturates
enum { kOtMalformed = 1u, kOtBadValue = 2u };

// ---- write ---------------------------------------------------------------------------------------------------------------------
// The nodes of the pruned tree in the subtree of every node of depth `depth` < 16 (one for a collapsed node; what lies under it
// is not in the tree). below: the counts of depth + 1, null where that is depth 16.
__global__ void __launch_bounds__(256) occ_ot_count_kernel(OccLevel l, const unsigned* __restrict__ below, unsigned* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= l.n) return;
  const unsigned info = l.info[i];
  unsigned c = 1;
  if (!(info & kOccCollapsed)) {
    const unsigned kids = __popc(info & 0xFFu), first = l.first[i];
    for (unsigned k = 0; k < kids; k++) c += below ? below[first + k] : 1u;
  }
  cnt[i] = c;
}

// One lane per node of depth `depth` < 16 that has children in the pruned tree: child k stands at the parent's rank + 1 + the
// nodes under the children before it. order[rank] names the node: its index among the voxels, or kOccInnerTag | index among the
// nodes above them. below_cnt / below_rank: of depth + 1, null where that is depth 16.
__global__ void __launch_bounds__(256) occ_ot_rank_kernel(OccLevel l, const unsigned* __restrict__ rank, const unsigned* __restrict__ below_cnt,
                                                           unsigned* __restrict__ below_rank, unsigned below_tag, unsigned* __restrict__ order,
                                                           uint32_t nodes) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= l.n) return;
  const unsigned info = l.info[i];
  if (((info >> kOccTopShift) & 31u) != kOccNoTop) return;   // collapsed, or below a collapsed node
  const unsigned kids = __popc(info & 0xFFu), first = l.first[i];
  unsigned r = rank[i] + 1;
  for (unsigned k = 0; k < kids; k++) {
    const unsigned child = first + k;
    if (below_rank) below_rank[child] = r;
    if (r < nodes) order[r] = below_tag + child;
    r += below_cnt ? below_cnt[child] : 1u;
  }
}

struct OccOtRef {   // where a ranked node's value and child mask are
  const unsigned *leaf_val, *node_val, *node_info;
};

// writeNodesRecurs by rank: lane r writes the float of the node at rank r and its child mask at 5 r. The 1280 bytes of a workgroup
// are put together in LDS and stored as 320 dwords; only the last dword of the body, where 5 * nodes is no multiple of 4, leaves
// as bytes.
__global__ void __launch_bounds__(256) occ_ot_body_kernel(const unsigned* __restrict__ order, uint32_t nodes, OccOtRef t, uint8_t* __restrict__ out) {
  __shared__ unsigned stage[320];
  uint8_t* bytes = (uint8_t*)stage;
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r < nodes) {
    const unsigned at = order[r];
    unsigned v, mask = 0;
    if (at & kOccInnerTag) {
      const unsigned g = at & ~kOccInnerTag, info = t.node_info[g];
      v = t.node_val[g];
      mask = (info & kOccCollapsed) ? 0u : info & 0xFFu;
    } else {
      v = t.leaf_val[at];
    }
    uint8_t* rec = bytes + 5 * threadIdx.x;
    rec[0] = (uint8_t)v;
    rec[1] = (uint8_t)(v >> 8);
    rec[2] = (uint8_t)(v >> 16);
    rec[3] = (uint8_t)(v >> 24);
    rec[4] = (uint8_t)mask;
  }
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * 1280, total = (size_t)nodes * 5;
  for (unsigned w = threadIdx.x; w < 320; w += 256) {
    const size_t o = base + 4 * (size_t)w;
    if (o + 4 <= total) ((unsigned*)(out + base))[w] = stage[w];
    else
      for (size_t b = o; b < total; b++) out[b] = bytes[b - base];
  }
}

struct OccOtRanks {   // the pieces of sbm_occ_tree::ot
  unsigned *cnt, *rank, *order;
};

// The pre-order ranks of the n nodes of the pruned tree (n >= 1): *order names the node at every rank. Ranked by the first call
// after a build, placed alike by the later ones. The coloured stream (sbm_occ_color.hip) maps its body by the same ranks.
int occ_ot_rank_run(sbm_occ_tree* t, uint32_t n, const unsigned** order) {
  sbm_handle* h = t->h;
  OccOtRanks r;
  HIPCHK(h, carve(t->ot, h->stream, [&](Carve& c) {
    r = {c.take<unsigned>(t->inner_total), c.take<unsigned>(t->inner_total), c.take<unsigned>(n)};
  }, occ_pad));
  *order = r.order;
  if (t->ot_ranked) return SBM_OK;
  for (int d = kOccDepth - 1; d >= 0; d--) {   // bottom-up
    const OccLevel l = occ_tree_level(t, d);
    hipLaunchKernelGGL(occ_ot_count_kernel, dim3((l.n + 255) / 256), dim3(256), 0, h->stream, l,
                       d + 1 < kOccDepth ? r.cnt + t->off[d + 1] : nullptr, r.cnt + t->off[d]);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipMemsetAsync(r.rank, 0, 4, h->stream));                  // the root is node 0 above the voxels, at rank 0
  HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)r.order, (int)kOccInnerTag, 1, h->stream));
  for (int d = 0; d < kOccDepth; d++) {        // top-down
    const OccLevel l = occ_tree_level(t, d);
    const bool inner = d + 1 < kOccDepth;
    hipLaunchKernelGGL(occ_ot_rank_kernel, dim3((l.n + 255) / 256), dim3(256), 0, h->stream, l, r.rank + t->off[d],
                       inner ? r.cnt + t->off[d + 1] : nullptr, inner ? r.rank + t->off[d + 1] : nullptr,
                       inner ? kOccInnerTag | (unsigned)t->off[d + 1] : 0u, r.order, n);
    HIPCHK(h, hipGetLastError());
  }
  t->ot_ranked = true;
  return SBM_OK;
}

static int occ_ot_body_run(sbm_occ_tree* t, uint8_t* d_bytes, size_t cap, size_t* nbytes) {
  sbm_handle* h = t->h;
  int st = occ_tree_stats(t);
  if (st != SBM_OK) return st;
  unsigned long long nodes = 0;
  for (int d = 0; d <= kOccDepth; d++) nodes += t->host.nodes_at[d];
  *nbytes = (size_t)(5 * nodes);
  if (*nbytes > cap) return SBM_ERR_SIZE;
  return occ_timed_run(h, kOccTreeQuery, nodes > 0, 1, [&]() -> int {
    const uint32_t n = (uint32_t)nodes;   // below 2^31 + 2^30: a build refuses 2^31 nodes above the voxels
    const unsigned* order;
    const int st = occ_ot_rank_run(t, n, &order);
    if (st != SBM_OK) return st;
    OccOtRef ref;
    ref.leaf_val = occ_tree_level(t, kOccDepth).val;
    ref.node_val = occ_tree_level(t, 0).val;
    ref.node_info = occ_tree_level(t, 0).info;
    hipLaunchKernelGGL(occ_ot_body_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, order, n, ref, d_bytes);
    return SBM_OK;
  });
}

// ---- load: the device parse ----------------------------------------------------------------------------------------------------
struct OccOtResult {            // what the host reads back after the parse, in one copy
  unsigned flags, leaves;
  unsigned long long voxels;    // saturates at kOtVolCap
};

// An exclusive scan of one value per thread over the 256 threads of a workgroup (Hillis-Steele in LDS) -> the thread's prefix;
// *total: the workgroup's sum. Every thread of the workgroup has to call it.
template <class T, class Op> __device__ __forceinline__ T occ_ot_block_scan(T v, T* lds, Op op, T zero, T* total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const T a = t >= o ? lds[t - o] : zero;
    __syncthreads();
    lds[t] = op(a, lds[t]);
    __syncthreads();
  }
  const T before = t ? lds[t - 1] : zero;
  *total = lds[255];
  __syncthreads();   // the caller may use lds again
  return before;
}

struct OtPair { int d; unsigned leaves; };   // what the first scan carries: the change of D, and leaves
struct OtPairAdd {
  __device__ OtPair operator()(OtPair a, OtPair b) const { return OtPair{a.d + b.d, a.leaves + b.leaves}; }
};
struct OtVolAdd {
  __device__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return min(a + b, kOtVolCap); }
};

__device__ __forceinline__ unsigned occ_ot_mask(const uint8_t* __restrict__ rec, uint32_t i) { return rec[5 * (size_t)i + 4]; }

// per tile of kOtTile records: the sum of popcount(mask) - 1 and the number of leaves
__global__ void __launch_bounds__(256) occ_ot_sums_kernel(const uint8_t* __restrict__ rec, uint32_t n, OtPair* __restrict__ tile) {
  __shared__ OtPair lds[256];
  OtPair mine{0, 0};
  for (int k = 0; k < 4; k++) {
    const uint32_t i = blockIdx.x * kOtTile + 4 * threadIdx.x + k;
    if (i < n) {
      const unsigned m = occ_ot_mask(rec, i);
      mine.d += (int)__popc(m) - 1;
      mine.leaves += m ? 0u : 1u;
    }
  }
  OtPair total;
  occ_ot_block_scan(mine, lds, OtPairAdd(), OtPair{0, 0}, &total);
  if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// exclusive scan of the tile sums in place; one workgroup, a run of tiles per thread. *total_out (may be null) receives the total.
template <class T, class Op> __global__ void __launch_bounds__(256) occ_ot_tiles_kernel(T* __restrict__ v, uint32_t tiles, Op op, T zero,
                                                                                         T* __restrict__ total_out) {
  __shared__ T lds[256];
  const uint32_t per = (tiles + 255) / 256;
  const uint32_t lo = min(threadIdx.x * per, tiles), hi = min(lo + per, tiles);
  T sum = zero;
  for (uint32_t t = lo; t < hi; t++) sum = op(sum, v[t]);
  T total;
  T before = occ_ot_block_scan(sum, lds, op, zero, &total);
  for (uint32_t t = lo; t < hi; t++) {
    const T x = v[t];
    v[t] = before;
    before = op(before, x);
  }
  if (threadIdx.x == 0 && total_out) *total_out = total;
}

// D[i] for i in 0..n and leaf_at[i], the leaves before record i. The stream is one complete tree iff D[i] >= 1 for all i < n and
// D[n] == 0.
__global__ void __launch_bounds__(256) occ_ot_scan_kernel(const uint8_t* __restrict__ rec, uint32_t n, const OtPair* __restrict__ tile,
                                                           int* __restrict__ D, unsigned* __restrict__ leaf_at, OccOtResult* __restrict__ res) {
  __shared__ OtPair lds[256];
  OtPair item[4], mine{0, 0};
  for (int k = 0; k < 4; k++) {
    const uint32_t i = blockIdx.x * kOtTile + 4 * threadIdx.x + k;
    item[k] = OtPair{0, 0};
    if (i < n) {
      const unsigned m = occ_ot_mask(rec, i);
      item[k] = OtPair{(int)__popc(m) - 1, m ? 0u : 1u};
    }
    mine = OtPairAdd()(mine, item[k]);
  }
  OtPair total;
  OtPair run = OtPairAdd()(tile[blockIdx.x], occ_ot_block_scan(mine, lds, OtPairAdd(), OtPair{0, 0}, &total));
  bool bad = false;
  for (int k = 0; k < 4; k++) {
    const uint32_t i = blockIdx.x * kOtTile + 4 * threadIdx.x + k;
    if (i < n) {
      D[i] = 1 + run.d;
      leaf_at[i] = run.leaves;
      bad = bad || 1 + run.d < 1;
    }
    run = OtPairAdd()(run, item[k]);
    if (i + 1 == n) {
      D[n] = 1 + run.d;
      bad = bad || 1 + run.d != 0;
      res->leaves = run.leaves;
    }
  }
  if (bad) atomicOr(&res->flags, kOtMalformed);
}

struct OccOtMinima {      // level 0 is D itself; level k + 1 holds the minimum of every kOtFan entries of level k
  const int* v[kOtMaxLevels];
  uint32_t len[kOtMaxLevels];
  int levels;
};

__global__ void __launch_bounds__(256) occ_ot_minima_kernel(const int* __restrict__ in, uint32_t n_in, int* __restrict__ out, uint32_t n_out) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_out) return;
  int m = 0x7FFFFFFF;
  for (int k = 0; k < kOtFan; k++) {
    const uint32_t j = t * kOtFan + k;
    if (j < n_in) m = min(m, in[j]);
  }
  out[t] = m;
}

// link[i] = parent(i) << 3 | child index of i, for i >= 1: the parent is the largest j < i with D[j] <= D[i]. The search looks at
// the entries before i within its tile of each level, going up while there is none, then comes down into the last tile that has
// one: at most kOtFan loads per level either way. Under the parent p, i is child number r = D[p] + c[p] - 1 - D[i] from the
// first, and its child index is the position of the r-th set bit of mask[p].
__global__ void __launch_bounds__(256) occ_ot_parent_kernel(const uint8_t* __restrict__ rec, uint32_t n, OccOtMinima h,
                                                             unsigned* __restrict__ link, OccOtResult* __restrict__ res) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (i == 0) {
    link[0] = 0;
    return;
  }
  const int target = h.v[0][i];
  bool bad = false, found = false;
  uint32_t pos = i, at = 0;
  int level = 0;
  for (; level < h.levels; level++) {                      // up
    const uint32_t start = pos & ~(uint32_t)(kOtFan - 1);
    for (uint32_t j = min(pos, h.len[level]); j > start && !found; j--)
      if (h.v[level][j - 1] <= target) {
        found = true;
        at = j - 1;
      }
    if (found || start == 0) break;
    pos = start / kOtFan;
  }
  bad = !found;
  while (found && level > 0) {                             // down into tile `at` of the level below
    level--;
    const uint32_t start = at * kOtFan, end = min(start + kOtFan, h.len[level]);
    found = false;
    for (uint32_t j = end; j > start && !found; j--)
      if (h.v[level][j - 1] <= target) {
        found = true;
        at = j - 1;
      }
    bad = bad || !found;
  }
  unsigned cidx = 0;
  uint32_t p = 0;
  if (!bad) {
    p = min(at, i - 1);
    const unsigned m = occ_ot_mask(rec, p);
    const int r = h.v[0][p] + (int)__popc(m) - 1 - target;
    bad = r < 0 || r >= (int)__popc(m);
    int seen = 0;
    for (unsigned b = 0; b < 8 && !bad; b++)
      if (m >> b & 1u) {
        if (seen == r) cidx = b;
        seen++;
      }
  }
  link[i] = bad ? 0u : p << 3 | cidx;
  if (bad) atomicOr(&res->flags, kOtMalformed);
}

// One lane per record; a leaf (mask 0) walks up to the root: at most 16 steps, a 17th is a malformed stream (a node below depth
// 16). Leaf j in record order, which is Morton order: word[j] = first code << 8 | depth << 1, val[j] its float bits, vol[j] its
// 8^(16 - depth) voxels. vol is zero beforehand: the entries past the last leaf stay so.
__global__ void __launch_bounds__(256) occ_ot_leaf_kernel(const uint8_t* __restrict__ rec, uint32_t n, const unsigned* __restrict__ link,
                                                           const unsigned* __restrict__ leaf_at, unsigned long long* __restrict__ word,
                                                           unsigned* __restrict__ val, unsigned long long* __restrict__ vol,
                                                           OccOtResult* __restrict__ res) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || occ_ot_mask(rec, i)) return;
  const uint8_t* r = rec + 5 * (size_t)i;
  const unsigned v = r[0] | (unsigned)r[1] << 8 | (unsigned)r[2] << 16 | (unsigned)r[3] << 24;
  unsigned long long code = 0;
  int depth = 0;
  uint32_t cur = i;
  for (int s = 0; s < kOccDepth && cur; s++) {
    const unsigned l = link[cur];
    code |= (unsigned long long)(l & 7u) << (3 * s);
    cur = min(l >> 3, cur - 1);   // a parent lies before its child
    depth++;
  }
  unsigned flags = cur ? (unsigned)kOtMalformed : 0u;
  if ((v & 0x7F800000u) == 0x7F800000u) flags |= kOtBadValue;   // NaN or infinite
  const int level = kOccDepth - depth;
  const uint32_t j = min(leaf_at[i], n - 1);
  word[j] = code << (3 * level) << 8 | (unsigned long long)depth << 1;
  val[j] = v;
  vol[j] = 1ull << (3 * level);
  if (flags) atomicOr(&res->flags, flags);
}

__global__ void __launch_bounds__(256) occ_ot_vol_sums_kernel(const unsigned long long* __restrict__ vol, uint32_t n,
                                                               unsigned long long* __restrict__ tile) {
  __shared__ unsigned long long lds[256];
  unsigned long long mine = 0;
  for (int k = 0; k < 4; k++) {
    const uint32_t i = blockIdx.x * kOtTile + 4 * threadIdx.x + k;
    if (i < n) mine += vol[i];   // four volumes of at most 2^48
  }
  unsigned long long total;
  occ_ot_block_scan(mine, lds, OtVolAdd(), 0ull, &total);
  if (threadIdx.x == 0) tile[blockIdx.x] = total;
}

// first[j]: the voxels of the leaves before j, in 32 bits (a load goes on only when the total is within the capacity, at most 2^30)
__global__ void __launch_bounds__(256) occ_ot_vol_scan_kernel(const unsigned long long* __restrict__ vol, uint32_t n,
                                                               const unsigned long long* __restrict__ tile, unsigned* __restrict__ first) {
  __shared__ unsigned long long lds[256];
  unsigned long long item[4], mine = 0;
  for (int k = 0; k < 4; k++) {
    const uint32_t i = blockIdx.x * kOtTile + 4 * threadIdx.x + k;
    item[k] = i < n ? vol[i] : 0ull;
    mine += item[k];
  }
  unsigned long long total;
  unsigned long long run = OtVolAdd()(tile[blockIdx.x], occ_ot_block_scan(mine, lds, OtVolAdd(), 0ull, &total));
  for (int k = 0; k < 4; k++) {
    const uint32_t i = blockIdx.x * kOtTile + 4 * threadIdx.x + k;
    if (i < n) first[i] = (unsigned)min(run, 0xFFFFFFFFull);
    run = OtVolAdd()(run, item[k]);
  }
}

// ---- load: the expansion -------------------------------------------------------------------------------------------------------
struct OccOtLoad {
  uint32_t leaves, total;
  uint32_t mask, max_probe;
};

// occ_load_kernel's shape (sbm_occ_load.hip) with the leaf's float as the stored word: one output voxel per lane finds its leaf in
// the prefix array, de-interleaves its code and claims its slot. The voxels of one load are distinct: a plain store of the value.
__global__ void __launch_bounds__(256) occ_ot_expand_kernel(const unsigned long long* __restrict__ leaf, const unsigned* __restrict__ first,
                                                             const unsigned* __restrict__ value, OccOtLoad g,
                                                             unsigned long long* __restrict__ keys, unsigned* __restrict__ vals,
                                                             OccCounters* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < g.total;
  bool claimed = false, lost = false;
  if (live) {
    uint32_t lo = 0, hi = g.leaves;   // the last leaf with first[leaf] <= i
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (first[mid] <= i) lo = mid;
      else hi = mid;
    }
    const unsigned long long key = occ_key_of_code((leaf[lo] >> 8) | (unsigned long long)(i - first[lo]));
    uint32_t slot;
    lost = !occ_find_or_claim(keys, key, g.mask, g.max_probe, &slot, &claimed);
    if (!lost) vals[slot] = value[lo];
  }
  const unsigned long long got = __ballot(claimed), over = __ballot(lost);
  if ((threadIdx.x & 63) == 0) {
    if (got) atomicAdd(&ctr->size, (unsigned)__popcll(got));
    if (over) atomicAdd(&ctr->overflow, (unsigned long long)__popcll(over));
  }
}

// ---- load, host side -----------------------------------------------------------------------------------------------------------
struct OccOtArrays {   // of one load in the handle's io buffer: leaf words, prefix, values first, as the expansion reads them
  unsigned long long* word;
  unsigned* first;
  unsigned* val;
  // the device parse only
  unsigned long long *vol, *vol_tile;
  uint8_t* rec;
  int* D;
  int* minima;
  unsigned *leaf_at, *link;
  OtPair* tile;
  OccOtResult* res;
};
// The handle's io buffer grown to the arrays of n leaves or, with parse, n records
static hipError_t occ_ot_arrays(sbm_handle* h, size_t n, bool parse, OccOtArrays* a) {
  memset(a, 0, sizeof(*a));
  return carve(h->occ.io, h->stream, [&](Carve& c) {
    a->word = c.take<unsigned long long>(n);
    a->first = c.take<unsigned>(n);
    a->val = c.take<unsigned>(n);
    if (!parse) return;
    const size_t tiles = (n + kOtTile - 1) / kOtTile;
    a->vol = c.take<unsigned long long>(n);
    a->vol_tile = c.take<unsigned long long>(tiles);
    a->rec = c.take<uint8_t>(5 * n);
    a->D = c.take<int>(n + 1);
    a->minima = c.take<int>(n / (kOtFan - 1) + kOtMaxLevels);   // n/16 + n/256 + ... and one entry of rounding per level
    a->leaf_at = c.take<unsigned>(n);
    a->link = c.take<unsigned>(n);
    a->tile = c.take<OtPair>(tiles);
    a->res = c.take<OccOtResult>(1);
  }, occ_pad);
}

// The first n records (n >= 1) -> the leaves in the io buffer in record order, their prefix array, and what the host checks: the
// flags, the leaf count and the voxel total. One wait, at the end.
static int occ_ot_device_parse(sbm_handle* h, const uint8_t* records, uint32_t n, OccOtArrays* out, OccOtResult* result) {
  OccOtArrays& a = *out;
  HIPCHK(h, occ_ot_arrays(h, n, true, out));
  const uint32_t tiles = (n + kOtTile - 1) / kOtTile, blocks = (n + 255) / 256;
  HIPCHK(h, hipMemcpyAsync(a.rec, records, 5 * (size_t)n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemsetAsync(a.res, 0, sizeof(OccOtResult), h->stream));
  HIPCHK(h, hipMemsetAsync(a.vol, 0, 8 * (size_t)n, h->stream));
  hipLaunchKernelGGL(occ_ot_sums_kernel, dim3(tiles), dim3(256), 0, h->stream, a.rec, n, a.tile);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL((occ_ot_tiles_kernel<OtPair, OtPairAdd>), dim3(1), dim3(256), 0, h->stream, a.tile, tiles, OtPairAdd(), OtPair{0, 0},
                     (OtPair*)nullptr);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(occ_ot_scan_kernel, dim3(tiles), dim3(256), 0, h->stream, a.rec, n, a.tile, a.D, a.leaf_at, a.res);
  HIPCHK(h, hipGetLastError());
  OccOtMinima m;
  memset(&m, 0, sizeof(m));
  m.v[0] = a.D;
  m.len[0] = n;
  m.levels = 1;
  int* next = a.minima;
  while (m.len[m.levels - 1] > 1 && m.levels < kOtMaxLevels) {
    const uint32_t n_in = m.len[m.levels - 1], n_out = (n_in + kOtFan - 1) / kOtFan;
    hipLaunchKernelGGL(occ_ot_minima_kernel, dim3((n_out + 255) / 256), dim3(256), 0, h->stream, m.v[m.levels - 1], n_in, next, n_out);
    HIPCHK(h, hipGetLastError());
    m.v[m.levels] = next;
    m.len[m.levels] = n_out;
    m.levels++;
    next += n_out;
  }
  hipLaunchKernelGGL(occ_ot_parent_kernel, dim3(blocks), dim3(256), 0, h->stream, a.rec, n, m, a.link, a.res);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(occ_ot_leaf_kernel, dim3(blocks), dim3(256), 0, h->stream, a.rec, n, a.link, a.leaf_at, a.word, a.val, a.vol, a.res);
  HIPCHK(h, hipGetLastError());
  // the volumes are scanned over all n entries: the leaf count is on the device still, and the entries past it are zero
  hipLaunchKernelGGL(occ_ot_vol_sums_kernel, dim3(tiles), dim3(256), 0, h->stream, a.vol, n, a.vol_tile);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL((occ_ot_tiles_kernel<unsigned long long, OtVolAdd>), dim3(1), dim3(256), 0, h->stream, a.vol_tile, tiles, OtVolAdd(), 0ull,
                     &a.res->voxels);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(occ_ot_vol_scan_kernel, dim3(tiles), dim3(256), 0, h->stream, a.vol, n, a.vol_tile, a.first);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(result, a.res, sizeof(OccOtResult), hipMemcpyDeviceToHost, h->stream));   // nothing between this copy
  HIPCHK(h, hipStreamSynchronize(h->stream));                                                        // and its wait can return
  return SBM_OK;
}

// AbstractOcTree::read into the map. Everything that can refuse the stream comes before the map is touched; *touched tells.
static int occ_ot_load_body(sbm_occ_map* map, const uint8_t* bytes, size_t n, int sync, bool* touched, bool stamped) {
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  const double want = occ_printed_resolution(map->p.resolution);
  sbm_occ_ot_header info;
  size_t body = 0;
  int st = occ_ot_head(bytes, n, want, &info, &body, stamped);
  if (st != SBM_OK) return st;
  const bool host_parse = env_switch("SBM_OCC_OT_HOST_PARSE", 0) != 0 || info.size > kOtMaxRecords;
  if (!info.size) {                           // size 0: clear() and nothing else
    *touched = true;
    st = occ_clear(map);
    if (st == SBM_OK && sync) HIPCHK(h, hipStreamSynchronize(h->stream));
    return st;
  }
  OccOtArrays a;
  uint64_t leaves = 0, voxels = 0;
  if (host_parse) {
    std::vector<OccBtLeaf> words;
    std::vector<uint32_t> values;
    std::vector<unsigned> first;
    st = occ_ot_parse(bytes, n, want, &info, &words, &values, false, stamped);
    if (st != SBM_OK) return st;
    if (info.voxels > map->capacity && !occ_can_reserve(map, info.voxels)) return SBM_ERR_OCC_FULL;
    leaves = words.size();
    voxels = info.voxels;
    try {
      first.resize(words.size());
    } catch (const std::bad_alloc&) {
      return SBM_ERR_NOMEM;
    }
    uint64_t run = 0;
    for (size_t i = 0; i < words.size(); i++) {
      first[i] = (unsigned)run;               // below the capacity, which is at most 2^30
      run += (uint64_t)1 << (3 * (16 - occ_bt_depth(words[i])));
    }
    HIPCHK(h, occ_ot_arrays(h, words.size(), false, &a));
    HIPCHK(h, hipMemcpyAsync(a.word, words.data(), words.size() * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(a.first, first.data(), first.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(a.val, values.data(), values.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the host arrays end with this block
  } else {
    const uint32_t records = (uint32_t)info.size;
    OccOtResult r;
    HIPCHK(h, clk.mark(kOccMid, h->stream));
    st = occ_ot_device_parse(h, bytes + body, records, &a, &r);
    if (st != SBM_OK) return st;
    if (r.flags & kOtMalformed) return SBM_ERR_SIZE;
    if (r.flags & kOtBadValue) return SBM_ERR_UNSUPPORTED;
    leaves = r.leaves;
    voxels = r.voxels;
    if (!leaves || leaves > records) return SBM_ERR_HIP;   // cannot happen: a complete tree has a leaf
    if (voxels > map->capacity && !occ_can_reserve(map, voxels)) return SBM_ERR_OCC_FULL;
  }
  st = occ_logodds_alloc(map);
  if (st != SBM_OK) return st;
  *touched = true;
  OccOtLoad g;
  g.leaves = (uint32_t)leaves;
  g.total = (uint32_t)voxels;
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  st = occ_clear(map);
  if (st != SBM_OK) return st;
  map->mode = kOccModeLogOdds;
  if (voxels > map->capacity) {            // a growing map reserves the stream's voxels: the emptied table moves nothing
    st = occ_rehash(map, voxels);
    if (st != SBM_OK && st != SBM_ERR_NOMEM) return st;   // refused: the load goes on into the table it has and counts what it loses
    map->overflow_known = st == SBM_OK;
  }
  occ_probe(map, &g.mask, &g.max_probe);
  hipLaunchKernelGGL(occ_ot_expand_kernel, dim3((g.total + 255) / 256), dim3(256), 0, h->stream, a.word, a.first, a.val, g,
                     map->keys.as<unsigned long long>(), map->hits.as<unsigned>(), map->ctr.as<OccCounters>());
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(kOccLoad, host_parse ? kOccBegin : kOccMid, kOccEnd));
  return occ_overflow_status(map, sync);
}

// The device parse is part of the timed stage, so the clock starts before the stream is judged; a load that is refused puts the
// last load's time back, as it leaves the map.
static int occ_ot_load_run(sbm_occ_map* map, const uint8_t* bytes, size_t n, int sync, bool stamped = false) {
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  const float last = h->occ.clock.ms[kOccLoad];
  HIPCHK(h, occ_clock_start(h, kOccLoad, kOccLoad));
  bool touched = false;
  const int st = occ_ot_load_body(map, bytes, n, sync, &touched, stamped);
  if (!touched) h->occ.clock.ms[kOccLoad] = last;
  return st;
}

}  // namespace sbm
using namespace sbm;

extern "C" {
int sbm_occ_ot_body_device(sbm_occ_tree* tree, void* d_bytes, size_t cap, size_t* nbytes) {
  if (!tree || !nbytes || (cap > 0 && !d_bytes)) return SBM_ERR_NULL;
  if (tree->reading != SBM_OCC_TREE_LOGODDS && tree->built) return SBM_ERR_UNSUPPORTED;
  if ((uintptr_t)d_bytes & 3) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  return occ_ot_body_run(tree, (uint8_t*)d_bytes, cap, nbytes);
}

static int occ_ot_write_to(sbm_occ_tree* tree, const char* path, bool stamped) {
  if (!tree || !path) return SBM_ERR_NULL;
  if (tree->reading != SBM_OCC_TREE_LOGODDS && tree->built) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = tree->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  int st = occ_tree_stats(tree);
  if (st != SBM_OK) return st;
  unsigned long long nodes = 0;
  for (int d = 0; d <= kOccDepth; d++) nodes += tree->host.nodes_at[d];
  const size_t bytes = (size_t)(5 * nodes);
  std::vector<uint8_t> body;
  st = occ_body_host(h, bytes, &body, [&](uint8_t* d_bytes, size_t* got) { return occ_ot_body_run(tree, d_bytes, bytes, got); });
  return st != SBM_OK ? st : occ_ot_write_file(body, (size_t)nodes, tree->resolution, path, stamped ? "OcTreeStamped" : "OcTree");
}

int sbm_occ_ot_write(sbm_occ_tree* tree, const char* path) { return occ_ot_write_to(tree, path, false); }

// AbstractOcTree::write of an OcTreeStamped: the plain writer's ranks and five-byte records over the stamped structure, the other id
int sbm_occ_stamp_ot_write(sbm_occ_tree* tree, const char* path) {
  if (!tree || !path) return SBM_ERR_NULL;
  if (tree->built && !tree->stamped) return SBM_ERR_UNSUPPORTED;   // a snapshot of a map without stamps is a plain OcTree
  return occ_ot_write_to(tree, path, true);
}

int sbm_occ_stamp_ot_load(sbm_occ_map* map, const void* bytes, size_t n, int sync) {
  if (!map || (n > 0 && !bytes)) return SBM_ERR_NULL;
  return occ_ot_load_run(map, (const uint8_t*)bytes, n, sync, true);
}

int sbm_occ_stamp_ot_read(sbm_occ_map* map, const char* path, int sync) {
  if (!map || !path) return SBM_ERR_NULL;
  std::vector<uint8_t> data;
  const int st = occ_read_file(path, &data);
  if (st != SBM_OK) return st;
  return occ_ot_load_run(map, data.data(), data.size(), sync, true);
}

int sbm_occ_ot_load(sbm_occ_map* map, const void* bytes, size_t n, int sync) {
  if (!map || (n > 0 && !bytes)) return SBM_ERR_NULL;
  return occ_ot_load_run(map, (const uint8_t*)bytes, n, sync);
}

int sbm_occ_ot_read(sbm_occ_map* map, const char* path, int sync) {
  if (!map || !path) return SBM_ERR_NULL;
  std::vector<uint8_t> data;
  const int st = occ_read_file(path, &data);
  if (st != SBM_OK) return st;
  return occ_ot_load_run(map, data.data(), data.size(), sync);
}
}  // extern "C"
