// sbm_occ_tree.hip -- the octree above the occupancy map's voxels (include/sbm.h, "occupancy map: the octree above the voxels"):
// octomap's inner nodes, pruning, search at a depth, begin_leafs and the body of writeBinary.  gfx950.
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
#include "sbm_occ.h"

namespace sbm {

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
// kStamp (sbm.h, "occupancy map: time stamps per voxel"): octomap's STAMPED pruned tree. OcTreeNodeStamped::operator== compares value
// and stamp, so eight siblings collapse only if their stamps are equal too; the collapsed node has the common stamp (copyData), every
// other inner node the map's clock at build time (updateInnerOccupancy). cs / ps: the stamps of the child and the parent level.
// Without kStamp this is the kernel of a map without stamps, statement for statement.
template <bool kStamp>
__device__ __forceinline__ void occ_tree_parents(const OccLevel& c, const OccLevel& p, const unsigned* __restrict__ tile_off, int leaves,
                                                 const unsigned* __restrict__ cs, unsigned* __restrict__ ps, uint32_t clock) {
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
      if (kStamp) equal = equal && cs[j] == cs[i];                             // ... and the stamp
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
    if (kStamp) ps[at] = collapsed ? cs[i] : clock;
  }
}
__global__ void __launch_bounds__(256) occ_tree_parents_kernel(OccLevel c, OccLevel p, const unsigned* __restrict__ tile_off, int leaves) {
  occ_tree_parents<false>(c, p, tile_off, leaves, nullptr, nullptr, 0u);
}
__global__ void __launch_bounds__(256) occ_tree_parents_stamped_kernel(OccLevel c, OccLevel p, const unsigned* __restrict__ tile_off, int leaves,
                                                                       const unsigned* __restrict__ cs, unsigned* __restrict__ ps, uint32_t clock) {
  occ_tree_parents<true>(c, p, tile_off, leaves, cs, ps, clock);
}
// depth 16 of a stamped build: the voxel's own stamp, looked up by its key (the tree holds Morton codes)
__global__ void __launch_bounds__(256) occ_tree_leaf_stamps_kernel(const unsigned long long* __restrict__ code, uint32_t n,
                                                                   const unsigned long long* __restrict__ keys, const unsigned* __restrict__ stamps,
                                                                   uint32_t mask, uint32_t max_probe, unsigned* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t slot;
  out[i] = occ_find(keys, occ_key_of_code(code[i]), mask, max_probe, &slot) ? stamps[slot] : 0u;
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
  const uint32_t o = occ_wave_append(take, &st->cursor);   // every lane is here
  if (!take || o >= cap) return;
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
  keys[i] = occ_pack(occ_unspread(code) | half, occ_unspread(code >> 1) | half, occ_unspread(code >> 2) | half);
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

// ---- the tree, host side -------------------------------------------------------------------------------------------------
// t->leaf: the voxels' codes, values, parents and info words. t->node (inner): seven arrays over all the depths above 16, depth 0 first.
static void occ_level_layout(Carve& c, size_t n, bool inner, OccLevel* l) {
  l->code = c.take<unsigned long long>(n);
  l->val = c.take<unsigned>(n);
  l->parent = c.take<unsigned>(n);
  l->info = c.take<unsigned>(n);
  if (!inner) return;
  l->first = c.take<unsigned>(n);
  l->inner = c.take<unsigned>(n);
  l->rank = c.take<unsigned>(n);
}

// Depth d of a built tree, from the two layouts and the build's counts; a tree that was never built, or whose build failed, has
// empty levels.
OccLevel occ_tree_level(const sbm_occ_tree* t, int d) {
  OccLevel l;
  memset(&l, 0, sizeof(l));
  if (!t->built) return l;
  const bool inner = d < kOccDepth;   // the layout of the build, placed again with its counts
  Carve c{(inner ? t->node : t->leaf).as<char>(), 0, occ_pad};
  occ_level_layout(c, inner ? t->inner_total : t->count[d], inner, &l);
  const size_t o = inner ? t->off[d] : 0;   // the leaves' three missing arrays stay null
  l.code += o, l.val += o, l.parent += o, l.info += o, l.first += o, l.inner += o, l.rank += o;
  l.n = t->count[d];
  return l;
}

static int occ_tree_build_run(sbm_occ_tree* t, int reading, const sbm_occ_ray_params* rp, int sync) {
  sbm_occ_map* map = t->map;
  sbm_handle* h = t->h;
  StageClock& clk = h->occ.clock;
  HIPCHK(h, occ_clock_start(h, kOccTreeBuild, kOccTreeBuild));
  t->built = false;
  t->have_stats = false;
  t->ot_ranked = false;
  t->have_metric = false;
  t->colored = false;
  t->stamped = false;
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
  OccLevel leaf;
  HIPCHK(h, carve(t->leaf, h->stream, [&](Carve& c) { occ_level_layout(c, n, false, &leaf); }, occ_pad));
  unsigned long long* kk[2] = {leaf.code};
  unsigned* vv[2] = {leaf.val};
  HIPCHK(h, occ_sort_carve(h, n, &kk[1], &vv[1]));
  HIPCHK(h, h->occ.hist.grow((size_t)256 * tiles * 4, h->stream));
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  st = occ_compact_run(map, n, kk[0], vv[0]);
  if (st != SBM_OK) return st;
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
  const auto node_layout = [&](Carve& c) { OccLevel all; occ_level_layout(c, t->inner_total, true, &all); };   // occ_tree_level places it
  HIPCHK(h, t->node.grow(carve_bytes(node_layout, occ_pad), h->stream));
  HIPCHK(h, t->tiles.grow((size_t)tiles * 4, h->stream));
  const bool stamped = map->stamp.p != nullptr;   // only over a map with stamps: the stamped pruned tree
  unsigned *leaf_stamp = nullptr, *node_stamp = nullptr;
  if (stamped) {
    HIPCHK(h, carve(t->stamp, h->stream, [&](Carve& c) { c.take<unsigned>(n), c.take<unsigned>(t->inner_total); }, occ_pad));
    occ_tree_stamps(t, &leaf_stamp, &node_stamp);
    uint32_t mask, max_probe;
    occ_probe(map, &mask, &max_probe);
    hipLaunchKernelGGL(occ_tree_leaf_stamps_kernel, dim3(blocks), dim3(256), 0, h->stream, kk[0], n, map->keys.as<unsigned long long>(),
                       map->stamp.as<unsigned>(), mask, max_probe, leaf_stamp);
    HIPCHK(h, hipGetLastError());
  }
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
      if (stamped)
        hipLaunchKernelGGL(occ_tree_parents_stamped_kernel, dim3(ct), dim3(256), 0, h->stream, child, parent, tile_off, d + 1 == kOccDepth ? 1 : 0,
                           d + 1 == kOccDepth ? leaf_stamp : node_stamp + t->off[d + 1], node_stamp + t->off[d], map->clock);
      else
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
  if (st == SBM_OK && map->color.p) st = occ_color_tree_run(t);   // only over a map with colours
  if (st == SBM_OK) t->stamped = stamped;
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
int occ_tree_stats(sbm_occ_tree* t) {
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

static int occ_tree_search_run(sbm_occ_tree* t, size_t n, const float* d_xyz, int depth, float thres, int* d_state, unsigned* d_value,
                               int* d_found, int sync) {
  sbm_handle* h = t->h;
  const OccLevel l = occ_tree_level(t, depth);
  return occ_timed_run(h, kOccTreeQuery, n > 0, sync, [&]() -> int {
    hipLaunchKernelGGL(occ_tree_search_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, d_xyz, n, 1. / t->resolution, l,
                       depth, thres, d_state, d_value, d_found);
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
  return occ_timed_run(h, kOccTreeQuery, n > 0, 1, [&]() -> int {
    OccSelection s;
    int st = occ_tree_select_begin(t, n, d_keys, d_depth, &s);
    if (st != SBM_OK) return st;
    OccTreeStats* stats = t->stats.as<OccTreeStats>();
    for (int d = 0; d <= max_depth; d++) {
      const OccLevel l = occ_tree_level(t, d);
      const unsigned tag = d == kOccDepth ? 0u : kOccInnerTag | (unsigned)t->off[d];
      hipLaunchKernelGGL(occ_tree_select_kernel, dim3((l.n + 255) / 256), dim3(256), 0, h->stream, l, d, max_depth, tag, n, s.kk[0], s.vv[0], stats);
      HIPCHK(h, hipGetLastError());
    }
    return occ_tree_select_end(t, s, d_value);
  });
}

int occ_tree_select_begin(sbm_occ_tree* t, uint32_t n, unsigned long long* d_keys, int* d_depth, OccSelection* s) {
  sbm_handle* h = t->h;
  const uint32_t tiles = (n + kOccTile - 1) / kOccTile;
  s->n = n;
  s->kk[0] = d_keys;
  s->vv[0] = (unsigned*)d_depth;
  HIPCHK(h, occ_sort_carve(h, n, &s->kk[1], &s->vv[1]));
  HIPCHK(h, h->occ.hist.grow((size_t)256 * tiles * 4, h->stream));
  HIPCHK(h, hipMemsetAsync(&t->stats.as<OccTreeStats>()->cursor, 0, sizeof(unsigned), h->stream));
  return SBM_OK;
}

int occ_tree_select_end(sbm_occ_tree* t, const OccSelection& s, unsigned* d_value) {
  sbm_handle* h = t->h;
  OccTreeRef ref;
  memset(&ref, 0, sizeof(ref));
  ref.leaf_val = occ_tree_level(t, kOccDepth).val;
  ref.node_val = occ_tree_level(t, 0).val;
  for (int d = 0; d < kOccDepth; d++) ref.off[d] = (uint32_t)t->off[d];
  const int st = occ_sort_run(h, s.kk, s.vv, s.n, h->occ.hist.as<unsigned>());
  if (st != SBM_OK) return st;
  hipLaunchKernelGGL(occ_tree_gather_kernel, dim3((s.n + 255) / 256), dim3(256), 0, h->stream, s.kk[0], (int*)s.vv[0], d_value, s.n, ref);
  return SBM_OK;
}

static int occ_tree_binary_run(sbm_occ_tree* t, uint8_t* d_bytes, size_t cap, size_t* nbytes) {
  sbm_handle* h = t->h;
  int st = occ_tree_stats(t);
  if (st != SBM_OK) return st;
  unsigned long long inner = 0;
  for (int d = 0; d < kOccDepth; d++) inner += t->host.nodes_at[d] - t->host.leaves_at[d];
  *nbytes = (size_t)(2 * inner);
  if (*nbytes > cap) return SBM_ERR_SIZE;
  return occ_timed_run(h, kOccTreeQuery, inner > 0, 1, [&]() -> int {
    for (int d = 0; d < kOccDepth; d++) {
      const OccLevel l = occ_tree_level(t, d), below = occ_tree_level(t, d + 1);
      hipLaunchKernelGGL(occ_tree_binary_kernel, dim3((l.n + 255) / 256), dim3(256), 0, h->stream, l, below, d, t->cmax, d_bytes, *nbytes);
      HIPCHK(h, hipGetLastError());
    }
    return SBM_OK;
  });
}

static int occ_tree_depth_check(int depth) { return depth < 0 || depth > kOccDepth ? SBM_ERR_SIZE : SBM_OK; }

}  // namespace sbm
using namespace sbm;

extern "C" {
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
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  return occ_search_host(tree->h, n, xyz, true, state, value, found_depth, [&](const float* d_xyz, int* d_state, unsigned* d_value, int* d_found) {
    return occ_tree_search_run(tree, n, d_xyz, depth ? depth : kOccDepth, occupancy_thres_log, d_state, d_value, d_found, 0);
  });
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
  struct { unsigned long long* keys; int* depth; unsigned* value; } io;
  HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& c) { io = {c.take<unsigned long long>(n), c.take<int>(n), c.take<unsigned>(n)}; }, occ_pad));
  st = occ_tree_leaves_run(tree, max_depth, io.keys, io.depth, io.value, n, count);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpyAsync(keys, io.keys, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(depth, io.depth, n * 4, hipMemcpyDeviceToHost, h->stream));
  if (value) HIPCHK(h, hipMemcpyAsync(value, io.value, n * 4, hipMemcpyDeviceToHost, h->stream));
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
  st = occ_body_host(h, bytes, &body, [&](uint8_t* d_bytes, size_t* got) { return occ_tree_binary_run(tree, d_bytes, bytes, got); });
  return st != SBM_OK ? st : occ_write_file(body, (size_t)nodes, tree->resolution, path);
}
}  // extern "C"
