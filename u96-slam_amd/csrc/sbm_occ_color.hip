// sbm_occ_color.hip -- a colour per voxel of the log-odds map, octomap's ColorOcTree::setNodeColor and averageNodeColor
// (ColorOcTree.cpp:96-105, 146-161) on batches of items, and the reads that return it: search by points, and the sorted fetch.
// gfx950. include/sbm.h ("occupancy map: colour per voxel") states the contract; a map that never makes a colour call allocates
// and launches nothing of this file. The arithmetic is integer; nothing here contracts a multiply-add.
//
//   occ_color_find_kernel    FIND: one lane per item forms the key and looks its slot up (never a claim: an unknown voxel is a
//                            no-op), notes key, index and slot per item and counts found and skipped items.
//   occ_color_apply_kernel   APPLY, after the map's radix sort of (key, item index): one lane per run head walks its run in item
//                            order from the slot's colour word to its final one. The walk is sequential whatever the run's length:
//                            averaging is order-dependent, and a chain that passes through white starts over.
//   occ_color_search_kernel  one lane per point: state, log-odds and colour word.
//   occ_color_slots_kernel / occ_color_gather_kernel   the fetch: occupied slots -> (key, slot) pairs, sorted by the map's radix
//                            sort, then log-odds and colour word of each slot in key order.
//   occ_color_tree_leaf_kernel / occ_color_tree_level_kernel   the colours of a built tree, octomap's after prune();
//                            updateInnerOccupancy(): the voxels' words by key, then one launch per depth bottom-up, one lane per node.
//   occ_color_tree_lookup_kernel   the colour of each entry of a leaves call, by a binary search over its depth's codes.
//   occ_color_body_kernel    the ColorOcTree body by the .ot writer's ranks (occ_ot_rank_run): two dwords per node.
//   occ_color_expand_kernel  the loader's expansion with the leaf's colour; the stream is parsed on the host (sbm_occ_color_host.hip).
#include "sbm_occ.h"

namespace sbm {
#pragma clang fp contract(off)

struct OccColorCounts { unsigned long long found, skipped; };

struct OccColor {
  const unsigned long long* item_keys;   // the chunk's items: packed keys, or (null) float triples
  const float* xyz;
  const unsigned* rgb;                    // per item r | g << 8 | b << 16; the top byte is ignored
  uint32_t n;
  int op;
  double factor;                          // 1. / resolution
  uint32_t mask, max_probe;
  const unsigned long long* keys;         // the table
  unsigned* colors;
  OccColorCounts* counts;
  unsigned long long* sort_keys;          // per item: its key, kOccEmpty for one without a voxel; sorted before APPLY
  unsigned* index;                        // its index, the sort's payload
  uint32_t* slot_of;                      // per item (unsorted): its slot, or kOccNoSlot
};

__global__ void __launch_bounds__(256) occ_color_find_kernel(OccColor e) {
#pragma clang fp contract(off)
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  unsigned long long key = kOccEmpty;
  if (i < e.n) {
    if (e.item_keys) {
      const unsigned long long k = e.item_keys[i];
      if (!(k >> 48)) key = k;
    } else {   // coordToKeyChecked
      unsigned k0, k1, k2;
      if (occ_axis(e.factor, e.xyz[3 * (size_t)i], &k0) && occ_axis(e.factor, e.xyz[3 * (size_t)i + 1], &k1) &&
          occ_axis(e.factor, e.xyz[3 * (size_t)i + 2], &k2))
        key = occ_pack(k0, k1, k2);
    }
  }
  const bool skipped = i < e.n && key == kOccEmpty;
  uint32_t slot = kOccNoSlot;
  if (key != kOccEmpty && !occ_find(e.keys, key, e.mask, e.max_probe, &slot)) {
    slot = kOccNoSlot;
    key = kOccEmpty;   // search(key) == NULL: nothing to do
  }
  if (i < e.n) {
    e.sort_keys[i] = key;
    e.index[i] = i;
    e.slot_of[i] = slot;
  }
  occ_wave_count(slot != kOccNoSlot, &e.counts->found);   // every lane is here
  occ_wave_count(skipped, &e.counts->skipped);
}

// setColor / averageNodeColor's (prev + new) / 2 per channel in int, from white: the colour itself
__device__ __forceinline__ unsigned occ_color_step(unsigned prev, unsigned rgb, int op) {
  if (op == SBM_OCC_COLOR_SET || prev == kOccWhite) return rgb;
  const unsigned r = ((prev & 255) + (rgb & 255)) / 2, g = ((prev >> 8 & 255) + (rgb >> 8 & 255)) / 2,
                 b = ((prev >> 16 & 255) + (rgb >> 16 & 255)) / 2;
  return r | g << 8 | b << 16;
}

__global__ void __launch_bounds__(256) occ_color_apply_kernel(OccColor e) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= e.n) return;
  // A run is the sorted positions whose 48 key bits agree; an item without a voxel (kOccEmpty) sorts into the all-ones key's run
  // and is passed over there. The head is found from the keys: a run may cross wavefronts and tiles.
  const unsigned long long low = e.sort_keys[j] & kOccKeyBits;
  if (j != 0 && (e.sort_keys[j - 1] & kOccKeyBits) == low) return;
  uint32_t slot = kOccNoSlot;
  unsigned c = 0;
  for (uint32_t k = j; k < e.n; k++) {
    const unsigned long long key = e.sort_keys[k];
    if ((key & kOccKeyBits) != low) break;
    if (key == kOccEmpty) continue;
    const uint32_t item = e.index[k];
    if (slot == kOccNoSlot) {   // every item of the run that has a slot has the same
      slot = e.slot_of[item];
      c = e.colors[slot];
    }
    c = occ_color_step(c, e.rgb[item] & kOccWhite, e.op);
  }
  if (slot != kOccNoSlot) e.colors[slot] = c;
}

struct OccColorRead {
  double factor;
  float thres;
  uint32_t mask, max_probe;
  const unsigned long long* keys;
  const unsigned* vals;
  const unsigned* colors;   // null: a map without colours, every voxel white
};

__global__ void __launch_bounds__(256) occ_color_search_kernel(const float* __restrict__ xyz, size_t n, OccColorRead g, int* __restrict__ state,
                                                                unsigned* __restrict__ value, unsigned* __restrict__ color) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned k0, k1, k2, word = 0x7FC00000u, c = kOccWhite;
  int st = SBM_OCC_CELL_OUT;
  if (occ_axis(g.factor, xyz[3 * i], &k0) && occ_axis(g.factor, xyz[3 * i + 1], &k1) && occ_axis(g.factor, xyz[3 * i + 2], &k2)) {
    uint32_t slot;
    st = SBM_OCC_CELL_UNKNOWN;
    if (occ_find(g.keys, occ_pack(k0, k1, k2), g.mask, g.max_probe, &slot)) {
      word = g.vals[slot];
      st = __uint_as_float(word) >= g.thres ? SBM_OCC_CELL_OCCUPIED : SBM_OCC_CELL_FREE;   // isNodeOccupied
      if (g.colors) c = g.colors[slot];
    }
  }
  state[i] = st;
  if (value) value[i] = word;
  if (color) color[i] = c;
}

__global__ void __launch_bounds__(256) occ_color_slots_kernel(const unsigned long long* __restrict__ keys, uint32_t slots, uint32_t cap,
                                                               unsigned long long* __restrict__ out_keys, unsigned* __restrict__ out_slot,
                                                               OccCounters* __restrict__ ctr) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long k = i < slots ? keys[i] : kOccEmpty;
  const uint32_t o = occ_wave_append(k != kOccEmpty, &ctr->cursor);   // every lane is here
  if (k == kOccEmpty || o >= cap) return;   // the host sized the outputs from ctr->size
  out_keys[o] = k;
  out_slot[o] = i;
}

__global__ void __launch_bounds__(256) occ_color_gather_kernel(const unsigned* __restrict__ slot_of, uint32_t n, uint32_t slots,
                                                                const unsigned* __restrict__ vals, const unsigned* __restrict__ colors,
                                                                unsigned* __restrict__ out_vals, unsigned* __restrict__ out_colors) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint32_t slot = slot_of[j];
  if (slot >= slots) return;
  if (out_vals) out_vals[j] = vals[slot];
  if (out_colors) out_colors[j] = colors ? colors[slot] : kOccWhite;
}

// ---- the tree's colours: octomap's after prune(); updateInnerOccupancy(); -------------------------------------------------------
// depth 16: the voxel's own word, looked up by its key (the tree holds Morton codes)
__global__ void __launch_bounds__(256) occ_color_tree_leaf_kernel(const unsigned long long* __restrict__ code, uint32_t n, OccColorRead g,
                                                                   unsigned* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t slot;
  out[i] = occ_find(g.keys, occ_key_of_code(code[i]), g.mask, g.max_probe, &slot) ? g.colors[slot] : kOccWhite;
}

// One depth above, bottom-up: getAverageChildColor() -- int sums over the children whose colour is set, divided by their count,
// white if none is -- for a node that is not collapsed (updateColorChildren) and for a collapsed one whose child 0 is set
// (pruneNode: copyData of child 0, then the average if isColorSet()); a collapsed node whose child 0 is white is white.
__global__ void __launch_bounds__(256) occ_color_tree_level_kernel(OccLevel l, const unsigned* __restrict__ child, uint32_t child_n,
                                                                    unsigned* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= l.n) return;
  const unsigned info = l.info[i], kids = __popc(info & 0xFFu), first = l.first[i];
  unsigned r = 0, g = 0, b = 0, cnt = 0, c0 = kOccWhite;
  for (unsigned k = 0; k < kids && first + k < child_n; k++) {
    const unsigned c = child[first + k];
    if (k == 0) c0 = c;
    if (c != kOccWhite) {
      r += c & 255, g += c >> 8 & 255, b += c >> 16 & 255;
      cnt++;
    }
  }
  unsigned c = kOccWhite;
  if (cnt && !((info & kOccCollapsed) && c0 == kOccWhite)) c = (r / cnt) | (g / cnt) << 8 | (b / cnt) << 16;
  out[i] = c;
}

struct OccColorLevels {   // every depth of a built tree: its codes and its colour words
  const unsigned long long* code[kOccDepth + 1];
  const unsigned* color[kOccDepth + 1];   // null: a tree without colours
  uint32_t n[kOccDepth + 1];
};

// the colour of each entry of a leaves call: (centre key, depth) -> the node, by a binary search over its depth's codes
__global__ void __launch_bounds__(256) occ_color_tree_lookup_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ depth,
                                                                     uint32_t n, OccColorLevels t, unsigned* __restrict__ out) {
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
  out[i] = (t.color[d] && lo < t.n[d] && codes[lo] == code) ? t.color[d][lo] : kOccWhite;
}

// writeNodesRecurs of a ColorOcTree by rank: the node at rank r writes two dwords at 8 r, its float, then r, g, b and its child mask
__global__ void __launch_bounds__(256) occ_color_body_kernel(const unsigned* __restrict__ order, uint32_t nodes, const unsigned* __restrict__ leaf_val,
                                                              const unsigned* __restrict__ node_val, const unsigned* __restrict__ node_info,
                                                              const unsigned* __restrict__ leaf_color, const unsigned* __restrict__ node_color,
                                                              unsigned* __restrict__ out) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= nodes) return;
  const unsigned at = order[r];
  unsigned v, c, mask = 0;
  if (at & kOccInnerTag) {
    const unsigned g = at & ~kOccInnerTag, info = node_info[g];
    v = node_val[g];
    c = node_color ? node_color[g] : kOccWhite;
    mask = (info & kOccCollapsed) ? 0u : info & 0xFFu;
  } else {
    v = leaf_val[at];
    c = leaf_color ? leaf_color[at] : kOccWhite;
  }
  out[2 * (size_t)r] = v;
  out[2 * (size_t)r + 1] = (c & kOccWhite) | mask << 24;
}

struct OccColorLoad { uint32_t leaves, total, mask, max_probe; };
// The loader's expansion (occ_ot_expand_kernel's shape) with a colour: voxel i of the stream's cubes takes its leaf's float and
// its leaf's colour word
__global__ void __launch_bounds__(256) occ_color_expand_kernel(const unsigned long long* __restrict__ leaf, const unsigned* __restrict__ first,
                                                                const unsigned* __restrict__ value, const unsigned* __restrict__ color, OccColorLoad g,
                                                                unsigned long long* __restrict__ keys, unsigned* __restrict__ vals,
                                                                unsigned* __restrict__ colors, OccCounters* __restrict__ ctr) {
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
    if (!lost) {
      vals[slot] = value[lo];
      colors[slot] = color[lo];
    }
  }
  occ_wave_count(claimed, &ctr->size);   // every lane is here
  occ_wave_count(lost, &ctr->overflow);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
constexpr size_t kOccColorMax = (size_t)1 << 30;

// the word per slot, white, and the counts: at the first colour call
static int occ_color_alloc(sbm_occ_map* map) {
  sbm_handle* h = map->h;
  HIPCHK(h, map->color_counts.grow(sizeof(OccColorCounts), h->stream));
  if (!map->color.p) {
    HIPCHK(h, map->color.grow((size_t)map->slots * 4, h->stream));
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)map->color.p, (int)kOccWhite, map->slots, h->stream));
  }
  return SBM_OK;
}

struct OccColorInput {   // one call's items, in host or device memory
  const unsigned long long* keys;
  const float* xyz;
  const unsigned* rgb;
  bool host;
};

static int occ_color_chunk_run(sbm_occ_map* map, uint32_t n, OccColor& e) {
  sbm_handle* h = map->h;
  const uint32_t tiles = (n + kOccTile - 1) / kOccTile;
  unsigned long long* kk[2];
  unsigned* vv[2];
  HIPCHK(h, carve(h->occ.sort, h->stream, [&](Carve& c) {
    kk[0] = c.take<unsigned long long>(n), kk[1] = c.take<unsigned long long>(n);
    vv[0] = c.take<unsigned>(n), vv[1] = c.take<unsigned>(n);
    e.slot_of = c.take<uint32_t>(n);
  }, occ_pad));
  HIPCHK(h, h->occ.hist.grow((size_t)256 * tiles * 4, h->stream));
  e.n = n;
  e.sort_keys = kk[0], e.index = vv[0];
  occ_probe(map, &e.mask, &e.max_probe);
  e.keys = map->keys.as<unsigned long long>();
  e.colors = map->color.as<unsigned>();
  e.counts = map->color_counts.as<OccColorCounts>();
  hipLaunchKernelGGL(occ_color_find_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, e);
  HIPCHK(h, hipGetLastError());
  const int st = occ_sort_run(h, kk, vv, n, h->occ.hist.as<unsigned>());
  if (st != SBM_OK) return st;
  hipLaunchKernelGGL(occ_color_apply_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, e);
  HIPCHK(h, hipGetLastError());
  return SBM_OK;
}

static int occ_color_call(sbm_occ_map* map, size_t n, const OccColorInput& in, int op, int sync) {
  if (!map || (n > 0 && (!(in.keys || in.xyz) || !in.rgb))) return SBM_ERR_NULL;
  if (op != SBM_OCC_COLOR_SET && op != SBM_OCC_COLOR_AVERAGE) return SBM_ERR_UNSUPPORTED;
  if (n > kOccColorMax || map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  if (map->stamp.p) return SBM_ERR_UNSUPPORTED;   // a map is one octomap class: a stamped map takes no colour (sbm_occ_stamp.hip)
  if (!in.host && (((uintptr_t)in.keys & 7) || ((uintptr_t)in.xyz & 3) || ((uintptr_t)in.rgb & 3))) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  int st = occ_logodds_alloc(map);   // a colour call fixes the mode of a fresh map, as an edit does: colours live on log-odds maps only
  if (st == SBM_OK) st = occ_color_alloc(map);
  if (st != SBM_OK) return st;
  map->mode = kOccModeLogOdds;
  HIPCHK(h, hipMemsetAsync(map->color_counts.p, 0, sizeof(OccColorCounts), h->stream));
  map->color_items = n;
  OccColor e;
  memset(&e, 0, sizeof(e));
  e.factor = 1. / map->p.resolution;
  e.op = op;
  HIPCHK(h, occ_clock_start(h, kOccRaysApply, kOccRaysApply));
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  const size_t item_bytes = in.keys ? 8 : 12;
  for (size_t c = 0; c < occ_edit_chunks(n); c++) {   // chunk order is item order
    size_t begin, count;
    occ_edit_chunk(n, c, &begin, &count);
    e.item_keys = in.keys ? in.keys + begin : nullptr;
    e.xyz = in.xyz ? in.xyz + 3 * begin : nullptr;
    e.rgb = in.rgb + begin;
    if (in.host) {   // the chunk through the handle's staging
      char* d_items;
      unsigned* d_rgb;
      HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& cv) { d_items = cv.take<char>(count * item_bytes), d_rgb = cv.take<unsigned>(count); }, occ_pad));
      HIPCHK(h, hipMemcpyAsync(d_items, in.keys ? (const void*)e.item_keys : (const void*)e.xyz, count * item_bytes, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(d_rgb, e.rgb, count * 4, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));   // the caller's arrays are read
      e.item_keys = in.keys ? (const unsigned long long*)d_items : nullptr;
      e.xyz = in.keys ? nullptr : (const float*)d_items;
      e.rgb = d_rgb;
    }
    if ((st = occ_color_chunk_run(map, (uint32_t)count, e)) != SBM_OK) return st;
    if (in.host) HIPCHK(h, hipStreamSynchronize(h->stream));   // the staging is free for the next chunk
  }
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(kOccRaysApply, kOccBegin, kOccEnd));
  if (sync || in.host) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

static OccColorRead occ_color_read(const sbm_occ_map* map, float thres) {
  OccColorRead g;
  g.factor = 1. / map->p.resolution;
  g.thres = thres;
  occ_probe(map, &g.mask, &g.max_probe);
  g.keys = map->keys.as<unsigned long long>();
  g.vals = map->hits.as<unsigned>();
  g.colors = map->color.as<unsigned>();
  return g;
}

static int occ_color_search_run(sbm_occ_map* map, size_t n, const float* d_xyz, float thres, int* d_state, unsigned* d_value,
                                unsigned* d_color, int sync) {
  sbm_handle* h = map->h;
  return occ_timed_run(h, kOccSearch, n > 0, sync, [&]() -> int {
    hipLaunchKernelGGL(occ_color_search_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, d_xyz, n, occ_color_read(map, thres),
                       d_state, d_value, d_color);
    return SBM_OK;
  });
}

// Sorted keys of the map into d_keys, with the log-odds and the colour word of each (either may be null)
static int occ_color_fetch_run(sbm_occ_map* map, unsigned long long* d_keys, unsigned* d_vals, unsigned* d_colors, size_t cap, size_t* count) {
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
    hipLaunchKernelGGL(occ_color_slots_kernel, dim3((map->slots + 255) / 256), dim3(256), 0, h->stream, map->keys.as<unsigned long long>(), map->slots,
                       n, kk[0], vv[0], map->ctr.as<OccCounters>());
    HIPCHK(h, hipGetLastError());
    st = occ_sort_run(h, kk, vv, n, h->occ.hist.as<unsigned>());
    if (st != SBM_OK) return st;
    hipLaunchKernelGGL(occ_color_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, vv[0], n, map->slots, map->hits.as<unsigned>(),
                       map->color.as<unsigned>(), d_vals, d_colors);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, clk.mark(kOccEnd, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, clk.add(kOccFetch, kOccBegin, kOccEnd));
  }
  return c.overflow ? SBM_ERR_OCC_FULL : SBM_OK;
}

static void occ_color_tree_place(sbm_occ_tree* t, unsigned** leaf, unsigned** node) {
  Carve c{t->color.as<char>(), 0, occ_pad};
  *leaf = c.take<unsigned>(t->count[kOccDepth]);
  *node = c.take<unsigned>(t->inner_total);
}

// The colour words of the tree just built (the levels are valid and the map is the one they were made from)
int occ_color_tree_run(sbm_occ_tree* t) {
  sbm_handle* h = t->h;
  sbm_occ_map* map = t->map;
  const uint32_t n = t->count[kOccDepth];
  if (!n || !map->color.p) return SBM_OK;
  HIPCHK(h, carve(t->color, h->stream, [&](Carve& c) { c.take<unsigned>(n), c.take<unsigned>(t->inner_total); }, occ_pad));
  unsigned *leaf, *node;
  occ_color_tree_place(t, &leaf, &node);
  hipLaunchKernelGGL(occ_color_tree_leaf_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, occ_tree_level(t, kOccDepth).code, n,
                     occ_color_read(map, 0.f), leaf);
  HIPCHK(h, hipGetLastError());
  for (int d = kOccDepth - 1; d >= 0; d--) {   // bottom-up
    const OccLevel l = occ_tree_level(t, d);
    hipLaunchKernelGGL(occ_color_tree_level_kernel, dim3((l.n + 255) / 256), dim3(256), 0, h->stream, l,
                       d + 1 == kOccDepth ? leaf : node + t->off[d + 1], t->count[d + 1], node + t->off[d]);
    HIPCHK(h, hipGetLastError());
  }
  t->colored = true;
  return SBM_OK;
}

static int occ_color_leaves_run(sbm_occ_tree* t, const unsigned long long* d_keys, const int* d_depth, unsigned* d_color, uint32_t n) {
  sbm_handle* h = t->h;
  if (!n) return SBM_OK;
  OccColorLevels lv;
  memset(&lv, 0, sizeof(lv));
  unsigned *leaf = nullptr, *node = nullptr;
  if (t->built && t->colored) occ_color_tree_place(t, &leaf, &node);
  for (int d = 0; d <= kOccDepth; d++) {
    const OccLevel l = occ_tree_level(t, d);
    lv.code[d] = l.code;
    lv.n[d] = l.n;
    lv.color[d] = !leaf ? nullptr : d == kOccDepth ? leaf : node + t->off[d];
  }
  hipLaunchKernelGGL(occ_color_tree_lookup_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, d_keys, d_depth, n, lv, d_color);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

static int occ_color_nodes(sbm_occ_tree* t, unsigned long long* nodes) {
  const int st = occ_tree_stats(t);
  *nodes = 0;
  for (int d = 0; st == SBM_OK && d <= kOccDepth; d++) *nodes += t->host.nodes_at[d];
  return st;
}

static int occ_color_body_run(sbm_occ_tree* t, uint8_t* d_bytes, size_t cap, size_t* nbytes) {
  sbm_handle* h = t->h;
  unsigned long long nodes;
  const int st = occ_color_nodes(t, &nodes);
  if (st != SBM_OK) return st;
  *nbytes = (size_t)(8 * nodes);
  if (*nbytes > cap) return SBM_ERR_SIZE;
  return occ_timed_run(h, kOccTreeQuery, nodes > 0, 1, [&]() -> int {
    const uint32_t n = (uint32_t)nodes;
    const unsigned* order;
    const int st = occ_ot_rank_run(t, n, &order);
    if (st != SBM_OK) return st;
    unsigned *leaf = nullptr, *node = nullptr;
    if (t->colored) occ_color_tree_place(t, &leaf, &node);
    const OccLevel top = occ_tree_level(t, 0);
    hipLaunchKernelGGL(occ_color_body_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, order, n, occ_tree_level(t, kOccDepth).val, top.val,
                       top.info, leaf, node, (unsigned*)d_bytes);
    return SBM_OK;
  });
}

// AbstractOcTree::read of a ColorOcTree into the map. Everything that can refuse the stream comes before the map is touched.
static int occ_color_load_body(sbm_occ_map* map, const uint8_t* bytes, size_t n, bool* touched) {
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  sbm_occ_ot_header info;
  std::vector<OccBtLeaf> words;
  std::vector<uint32_t> values, colors;
  std::vector<unsigned> first;
  int st = occ_color_ot_parse(bytes, n, occ_printed_resolution(map->p.resolution), &info, &words, &values, &colors, false);
  if (st != SBM_OK) return st;
  if (info.voxels > map->capacity && !occ_can_reserve(map, info.voxels)) return SBM_ERR_OCC_FULL;
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
  struct { unsigned long long* word; unsigned *first, *val, *col; } a = {};
  const size_t leaves = words.size();
  if (leaves) {
    HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& c) {
      a = {c.take<unsigned long long>(leaves), c.take<unsigned>(leaves), c.take<unsigned>(leaves), c.take<unsigned>(leaves)};
    }, occ_pad));
    HIPCHK(h, hipMemcpyAsync(a.word, words.data(), leaves * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(a.first, first.data(), leaves * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(a.val, values.data(), leaves * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(a.col, colors.data(), leaves * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the host arrays end with this function
  }
  st = occ_logodds_alloc(map);
  if (st == SBM_OK) st = occ_color_alloc(map);
  if (st != SBM_OK) return st;
  *touched = true;
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  st = occ_clear(map);   // every voxel white
  if (st != SBM_OK) return st;
  map->mode = kOccModeLogOdds;
  if (leaves) {
    if (info.voxels > map->capacity) {       // a growing map reserves the stream's voxels: the emptied table moves nothing
      st = occ_rehash(map, info.voxels);
      if (st != SBM_OK && st != SBM_ERR_NOMEM) return st;   // refused: the load goes on into the table it has and counts what it loses
      map->overflow_known = st == SBM_OK;
    }
    OccColorLoad g;
    g.leaves = (uint32_t)leaves;
    g.total = (uint32_t)info.voxels;
    occ_probe(map, &g.mask, &g.max_probe);
    hipLaunchKernelGGL(occ_color_expand_kernel, dim3((g.total + 255) / 256), dim3(256), 0, h->stream, a.word, a.first, a.val, a.col, g,
                       map->keys.as<unsigned long long>(), map->hits.as<unsigned>(), map->color.as<unsigned>(), map->ctr.as<OccCounters>());
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(kOccLoad, kOccBegin, kOccEnd));
  return occ_overflow_status(map, 1);   // the staging is the handle's: the expansion has read it when the call returns
}

static int occ_color_load_run(sbm_occ_map* map, const uint8_t* bytes, size_t n) {
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  if (map->stamp.p) return SBM_ERR_UNSUPPORTED;   // a stamped map takes no colour: the map is as it was
  const float last = h->occ.clock.ms[kOccLoad];
  HIPCHK(h, occ_clock_start(h, kOccLoad, kOccLoad));
  bool touched = false;
  const int st = occ_color_load_body(map, bytes, n, &touched);
  if (!touched) h->occ.clock.ms[kOccLoad] = last;
  return st;
}

}  // namespace sbm
using namespace sbm;

extern "C" {

int sbm_occ_color_keys_device(sbm_occ_map* map, size_t n, const void* d_keys, const void* d_rgb, int op, int sync) {
  return occ_color_call(map, n, {(const unsigned long long*)d_keys, nullptr, (const unsigned*)d_rgb, false}, op, sync);
}

int sbm_occ_color_keys(sbm_occ_map* map, size_t n, const uint64_t* keys, const uint32_t* rgb, int op) {
  return occ_color_call(map, n, {(const unsigned long long*)keys, nullptr, (const unsigned*)rgb, true}, op, 1);
}

int sbm_occ_color_points_device(sbm_occ_map* map, size_t n, const void* d_xyz, const void* d_rgb, int op, int sync) {
  return occ_color_call(map, n, {nullptr, (const float*)d_xyz, (const unsigned*)d_rgb, false}, op, sync);
}

int sbm_occ_color_points(sbm_occ_map* map, size_t n, const float* xyz, const uint32_t* rgb, int op) {
  return occ_color_call(map, n, {nullptr, xyz, (const unsigned*)rgb, true}, op, 1);
}

int sbm_occ_color_last(sbm_occ_map* map, sbm_occ_color_info* out) {
  if (!map || !out) return SBM_ERR_NULL;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  OccColorCounts c = {};
  if (map->color_counts.p) {
    HIPCHK(h, hipMemcpyAsync(&c, map->color_counts.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  out->items = map->color_counts.p ? map->color_items : 0;
  out->found = c.found;
  out->skipped = c.skipped;
  out->unknown = out->items - c.found - c.skipped;
  return SBM_OK;
}

int sbm_occ_color_search_device(sbm_occ_map* map, size_t n, const void* d_xyz, float occupancy_thres_log, void* d_state, void* d_value,
                                void* d_color, int sync) {
  if (!map || (n > 0 && (!d_xyz || !d_state))) return SBM_ERR_NULL;
  if (std::isnan(occupancy_thres_log)) return SBM_ERR_SIZE;
  if (n > kOccColorMax || map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  if (((uintptr_t)d_xyz | (uintptr_t)d_state | (uintptr_t)d_value | (uintptr_t)d_color) & 3) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_color_search_run(map, n, (const float*)d_xyz, occupancy_thres_log, (int*)d_state, (unsigned*)d_value, (unsigned*)d_color, sync);
}

int sbm_occ_color_search(sbm_occ_map* map, size_t n, const float* xyz, float occupancy_thres_log, int32_t* state, void* value, uint32_t* color) {
  if (!map || (n > 0 && (!xyz || !state))) return SBM_ERR_NULL;
  if (std::isnan(occupancy_thres_log)) return SBM_ERR_SIZE;
  if (n > kOccColorMax || map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  // the colours ride in the staging's fourth array, the one a tree's search uses for its depths
  return occ_search_host(h, n, xyz, true, state, value, (int32_t*)color, [&](float* d_xyz, int* d_state, unsigned* d_value, int* d_found) {
    return occ_color_search_run(map, n, d_xyz, occupancy_thres_log, d_state, d_value, (unsigned*)d_found, 0);
  });
}

int sbm_occ_color_fetch_device(sbm_occ_map* map, void* d_keys, void* d_logodds, void* d_colors, size_t cap, size_t* count) {
  if (!map || !count || (cap > 0 && !d_keys)) return SBM_ERR_NULL;
  if (((uintptr_t)d_keys & 7) || (((uintptr_t)d_logodds | (uintptr_t)d_colors) & 3) || map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_color_fetch_run(map, (unsigned long long*)d_keys, (unsigned*)d_logodds, (unsigned*)d_colors, cap, count);
}

int sbm_occ_color_fetch(sbm_occ_map* map, uint64_t* keys, float* logodds, uint32_t* colors, size_t cap, size_t* count) {
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
  unsigned *d_v, *d_c;
  HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& cv) {
    d_k = cv.take<unsigned long long>(c.size), d_v = cv.take<unsigned>(c.size), d_c = cv.take<unsigned>(c.size);
  }, occ_pad));
  st = occ_color_fetch_run(map, d_k, d_v, d_c, c.size, count);
  if (st != SBM_OK && st != SBM_ERR_OCC_FULL) return st;
  HIPCHK(h, hipMemcpyAsync(keys, d_k, *count * 8, hipMemcpyDeviceToHost, h->stream));
  if (logodds) HIPCHK(h, hipMemcpyAsync(logodds, d_v, *count * 4, hipMemcpyDeviceToHost, h->stream));
  if (colors) HIPCHK(h, hipMemcpyAsync(colors, d_c, *count * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return st;
}

int sbm_occ_color_leaves_device(sbm_occ_tree* tree, int max_depth, void* d_keys, void* d_depth, void* d_value, void* d_color, size_t cap,
                                size_t* count) {
  if (!tree || !count || (cap > 0 && (!d_keys || !d_depth))) return SBM_ERR_NULL;   // the order of sbm_occ_tree_leaves_device
  if (max_depth < 0 || max_depth > kOccDepth) return SBM_ERR_SIZE;
  if ((uintptr_t)d_color & 3) return SBM_ERR_UNSUPPORTED;
  const int st = sbm_occ_tree_leaves_device(tree, max_depth, d_keys, d_depth, d_value, cap, count);
  if (st != SBM_OK || !d_color) return st;
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  return occ_color_leaves_run(tree, (const unsigned long long*)d_keys, (const int*)d_depth, (unsigned*)d_color, (uint32_t)*count);
}

int sbm_occ_color_leaves(sbm_occ_tree* tree, int max_depth, uint64_t* keys, int32_t* depth, float* value, uint32_t* color, size_t cap,
                         size_t* count) {
  if (!tree || !count || (cap > 0 && (!keys || !depth || !color))) return SBM_ERR_NULL;
  sbm_handle* h = tree->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  size_t n = 0;
  int st = sbm_occ_tree_leaves_device(tree, max_depth, nullptr, nullptr, nullptr, 0, &n);   // the count alone
  if (st != SBM_OK && st != SBM_ERR_SIZE) return st;
  *count = n;
  if (n > cap) return SBM_ERR_SIZE;
  if (!n) return SBM_OK;
  struct { unsigned long long* keys; int* depth; unsigned *value, *color; } io;
  HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& c) {
    io = {c.take<unsigned long long>(n), c.take<int>(n), c.take<unsigned>(n), c.take<unsigned>(n)};
  }, occ_pad));
  st = sbm_occ_color_leaves_device(tree, max_depth, io.keys, io.depth, io.value, io.color, n, count);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpyAsync(keys, io.keys, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(depth, io.depth, n * 4, hipMemcpyDeviceToHost, h->stream));
  if (value) HIPCHK(h, hipMemcpyAsync(value, io.value, n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(color, io.color, n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_occ_color_ot_body_device(sbm_occ_tree* tree, void* d_bytes, size_t cap, size_t* nbytes) {
  if (!tree || !nbytes || (cap > 0 && !d_bytes)) return SBM_ERR_NULL;
  if (tree->reading != SBM_OCC_TREE_LOGODDS && tree->built) return SBM_ERR_UNSUPPORTED;
  if ((uintptr_t)d_bytes & 3) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(tree->h->device);
  HIPCHK(tree->h, dscope.enter());
  return occ_color_body_run(tree, (uint8_t*)d_bytes, cap, nbytes);
}

int sbm_occ_color_ot_write(sbm_occ_tree* tree, const char* path) {
  if (!tree || !path) return SBM_ERR_NULL;
  if (tree->reading != SBM_OCC_TREE_LOGODDS && tree->built) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = tree->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  unsigned long long nodes;
  int st = occ_color_nodes(tree, &nodes);
  if (st != SBM_OK) return st;
  const size_t bytes = (size_t)(8 * nodes);
  std::vector<uint8_t> body;
  st = occ_body_host(h, bytes, &body, [&](uint8_t* d_bytes, size_t* got) { return occ_color_body_run(tree, d_bytes, bytes, got); });
  return st != SBM_OK ? st : occ_color_ot_write_file(body, (size_t)nodes, tree->resolution, path);
}

int sbm_occ_color_ot_load(sbm_occ_map* map, const void* bytes, size_t n, int sync) {
  if (!map || (n > 0 && !bytes)) return SBM_ERR_NULL;
  (void)sync;   // the parse is the host's: the load is synchronous
  return occ_color_load_run(map, (const uint8_t*)bytes, n);
}

int sbm_occ_color_ot_read(sbm_occ_map* map, const char* path, int sync) {
  if (!map || !path) return SBM_ERR_NULL;
  std::vector<uint8_t> data;
  const int st = occ_read_file(path, &data);
  if (st != SBM_OK) return st;
  (void)sync;
  return occ_color_load_run(map, data.data(), data.size());
}

}  // extern "C"
