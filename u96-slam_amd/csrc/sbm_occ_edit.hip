// sbm_occ_edit.hip -- the occupancy map edited by key: octomap's updateNode(key, float), setNodeValue and deleteNode
// (OccupancyOcTreeBase.hxx:273-285, 307-327, 373-433, 1097-1107; OcTreeBaseImpl.hxx:501-509, 681-716) on batches of items, and
// the deletes over a key range or a key box.  gfx950. include/sbm.h ("occupancy map: edit voxels by key") states the contract; a
// map that never edits launches nothing of this file. Nothing here contracts a multiply-add.
//
//   occ_edit_claim_kernel   CLAIM: one lane per item forms the key, finds or claims its slot (delete items only look), notes the
//                           slot per item and "created by this batch" in the slot's flag word, and counts skips and losses. It
//                           changes no value, so it runs again on a larger table (occ_grow_settle), flags moved with the keys.
//   occ_edit_apply_kernel   APPLY, after the map's radix sort of (key, item index): one lane per run head -- a sorted position
//                           whose left neighbour holds another key -- walks its run in item order from the slot's word to its
//                           final one, steps the change byte, and marks the slot in the removal mask if the voxel ends absent.
//   occ_delete_prep_kernel / occ_mark_keys_kernel / occ_mark_box_kernel   REMOVE: the given keys under deleteNode's depth mask,
//                           sorted; then one lane per slot marks by predicate (a binary search, or the key box).
//   occ_remove_kernel       the move of sbm_occ_grow.hip (occ_move_lane) behind the removal mask, into a table of the same size.
#include "sbm_occ.h"

namespace sbm {
#pragma clang fp contract(off)

struct OccEditCounts {
  unsigned claim_skipped, claim_lost;   // of the last CLAIM launch, which may run again: APPLY adds them to the totals
  unsigned deletes;                     // delete items of a chunk whose ops are in device memory
  unsigned all_ones;                    // range delete: a given key is, under the depth mask, the all-ones key (see occ_mark_keys_kernel)
  unsigned long long skipped, lost, created, removed;
};

struct OccEdit {
  const unsigned long long* item_keys;   // the chunk's items: packed keys, or (null) float triples
  const float* xyz;
  const uint8_t* ops;                     // null: all updates
  const float* values;
  uint32_t n;
  double factor;                          // 1. / resolution
  float cmin, cmax, thres;
  bool detect;
  uint32_t mask, max_probe;
  unsigned long long* keys;               // the table
  float* logodds;
  unsigned* flags;
  uint8_t* change;                        // null where detection was never enabled
  unsigned* colors;                       // null on a map without colours (sbm_occ_color.hip)
  uint8_t* remove;                        // null without ops: nothing can delete
  OccCounters* ctr;
  OccEditCounts* counts;
  unsigned long long* sort_keys;          // per item: its key, kOccEmpty for a skipped one; sorted before APPLY
  unsigned* index;                        // its index, the sort's payload
  uint32_t* slot_of;                      // per item (unsorted): its slot, or kOccNoSlot
};

__global__ void __launch_bounds__(256) occ_count_deletes_kernel(const uint8_t* __restrict__ ops, uint32_t n, OccEditCounts* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  occ_wave_count(i < n && ops[i] == SBM_OCC_EDIT_DELETE, &counts->deletes);
}

__global__ void __launch_bounds__(256) occ_edit_claim_kernel(OccEdit e) {
#pragma clang fp contract(off)
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  unsigned long long key = kOccEmpty;
  unsigned op = SBM_OCC_EDIT_UPDATE;
  if (i < e.n) {
    if (e.ops) op = e.ops[i];
    if (op <= SBM_OCC_EDIT_DELETE) {
      if (e.item_keys) {
        const unsigned long long k = e.item_keys[i];
        if (!(k >> 48)) key = k;
      } else {
        unsigned k0, k1, k2;
        if (occ_axis(e.factor, e.xyz[3 * (size_t)i], &k0) && occ_axis(e.factor, e.xyz[3 * (size_t)i + 1], &k1) &&
            occ_axis(e.factor, e.xyz[3 * (size_t)i + 2], &k2))
          key = occ_pack(k0, k1, k2);
      }
    }
  }
  uint32_t slot = kOccNoSlot;
  bool lost = false;
  if (key != kOccEmpty) {
    uint32_t at;
    if (op == SBM_OCC_EDIT_DELETE) {
      if (occ_find(e.keys, key, e.mask, e.max_probe, &at)) slot = at;
    } else {
      bool claimed = false;
      if (occ_find_or_claim(e.keys, key, e.mask, e.max_probe, &at, &claimed)) {
        slot = at;
        if (claimed) {   // the one lane that claimed it says so to APPLY: the voxel was absent when the batch began
          atomicAdd(&e.ctr->size, 1u);
          e.flags[at] = kOccCreated;
        }
      } else {
        lost = true;
      }
    }
  }
  if (i < e.n) {
    e.sort_keys[i] = key;
    e.index[i] = i;
    e.slot_of[i] = slot;
  }
  occ_wave_count(i < e.n && key == kOccEmpty, &e.counts->claim_skipped);   // every lane is here
  occ_wave_count(lost, &e.counts->claim_lost);
  occ_wave_count(lost, &e.ctr->overflow);
}

// kStamp (sbm.h, "occupancy map: time stamps per voxel"): the run's walk also carries the slot's stamp word -- the clock if any
// update item of the run passed the early-return test at its turn, else the old stamp, restarted at 0 by a delete; setNodeValue
// never stamps. One plain store by the run's one walker. Without kStamp this is the kernel of a map without stamps.
template <bool kStamp> __device__ __forceinline__ void occ_edit_apply(const OccEdit& e, unsigned* __restrict__ stamps, uint32_t clock) {
#pragma clang fp contract(off)
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0) {   // the counts of the CLAIM launch that stood
    e.counts->skipped += e.counts->claim_skipped;
    e.counts->lost += e.counts->claim_lost;
  }
  // A run is the sorted positions whose 48 key bits agree; a skipped item (kOccEmpty) sorts into the all-ones key's run and is
  // passed over there. The head is found from the keys: a run may cross wavefronts and tiles.
  const unsigned long long low = j < e.n ? e.sort_keys[j] & kOccKeyBits : 0;
  const bool head = j < e.n && (j == 0 || (e.sort_keys[j - 1] & kOccKeyBits) != low);
  bool created = false, removed = false;
  if (head) {
    uint32_t slot = kOccNoSlot;   // of the run's voxel: every item that has one has the same
    for (uint32_t k = j; k < e.n && slot == kOccNoSlot; k++) {
      const unsigned long long key = e.sort_keys[k];
      if ((key & kOccKeyBits) != low) break;
      if (key != kOccEmpty) slot = e.slot_of[e.index[k]];
    }
    if (slot != kOccNoSlot) {   // else: skipped items, deletes of an absent voxel, or a voxel that found no slot
      created = (e.flags[slot] & kOccCreated) != 0;
      bool present = !created, reborn = false;
      float v = e.logodds[slot];   // a claimed slot holds 0
      uint8_t state = e.change ? e.change[slot] : (uint8_t)kOccChangeNone;
      uint32_t stamp = 0;
      if (kStamp) stamp = stamps[slot];   // a claimed slot holds 0
      for (uint32_t k = j; k < e.n; k++) {
        const unsigned long long key = e.sort_keys[k];
        if ((key & kOccKeyBits) != low) break;
        if (key == kOccEmpty) continue;
        const uint32_t item = e.index[k];
        const unsigned op = e.ops ? e.ops[item] : (unsigned)SBM_OCC_EDIT_UPDATE;
        if (op == SBM_OCC_EDIT_DELETE) {   // deleteNode: the voxel goes with all it holds
          present = false;
          reborn = true;   // whatever the run makes of the voxel after this is a new node: white
          state = kOccChangeNone;
          if (kStamp) stamp = 0;
          continue;
        }
        float x = e.values[item];
        const bool born = !present;
        if (born) v = 0.f;
        const float before = v;
        if (op == SBM_OCC_EDIT_UPDATE) {   // updateNode(key, float): the early abort, then updateNodeLogOdds
          if (present && ((x >= 0.f && v >= e.cmax) || (x <= 0.f && v <= e.cmin))) continue;
          v = v + x;
          if (v < e.cmin) v = e.cmin;
          else if (v > e.cmax) v = e.cmax;
          if (kStamp) stamp = clock;       // OcTreeStamped::updateNodeLogOdds: updateTimestamp()
        } else {                           // setNodeValue: std::min(std::max(x, cmin), cmax)
          x = x < e.cmin ? e.cmin : x;
          x = e.cmax < x ? e.cmax : x;
          v = x;
        }
        present = true;
        if (e.detect) {
          if (born) state = kOccChangeCreated;
          else if ((before >= e.thres) != (v >= e.thres) && state != kOccChangeCreated)
            state = state == kOccChangeNone ? kOccChangeFlipped : kOccChangeNone;
        }
      }
      if (created) e.flags[slot] = 0;
      if (present) {
        e.logodds[slot] = v;
        if (e.change) e.change[slot] = state;
        if (kStamp) stamps[slot] = stamp;
        if (reborn && e.colors) e.colors[slot] = kOccWhite;   // deleted and created again inside the run: no move drops the word
      } else if (e.remove) {   // only a delete item makes a voxel absent, and a chunk with one has a mask
        e.remove[slot] = 1;
        removed = true;
      }
    }
  }
  occ_wave_count(created, &e.counts->created);   // every lane is here
  occ_wave_count(removed, &e.counts->removed);
}
__global__ void __launch_bounds__(256) occ_edit_apply_kernel(OccEdit e) { occ_edit_apply<false>(e, nullptr, 0u); }
__global__ void __launch_bounds__(256) occ_edit_apply_stamped_kernel(OccEdit e, unsigned* __restrict__ stamps, uint32_t clock) {
  occ_edit_apply<true>(e, stamps, clock);
}

// The given keys of a range delete under the depth mask, as the sort takes them; a key above bit 47 is skipped (kOccEmpty).
__global__ void __launch_bounds__(256) occ_delete_prep_kernel(const unsigned long long* __restrict__ keys, uint32_t n, unsigned long long mask,
                                                               unsigned long long* __restrict__ out_keys, unsigned* __restrict__ out_index,
                                                               OccEditCounts* __restrict__ counts) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool skip = false;
  if (i < n) {
    const unsigned long long k = keys[i];
    skip = (k >> 48) != 0;
    const unsigned long long m = skip ? kOccEmpty : k & mask;
    out_keys[i] = m;
    out_index[i] = i;
    if (m == kOccKeyBits) counts->all_ones = 1;   // every writer writes the same word
  }
  occ_wave_count(skip, &counts->skipped);   // every lane is here
}

// What the lanes of a workgroup counted, added to `counter` with one atomic: a marking pass runs over every slot of the table, and
// a hundred thousand wavefronts adding to one word would cost more than the pass. EVERY lane of the workgroup has to reach this call.
__device__ __forceinline__ void occ_block_count(unsigned mine, unsigned long long* counter) {
  __shared__ unsigned total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  if (threadIdx.x == 0 && total) atomicAdd(counter, (unsigned long long)total);
}
constexpr unsigned kOccMarkBlocks = 2048;   // of a marking pass: its lanes stride over the slots

// One lane per slot (in strides): its key under the depth mask is looked up among the sorted given keys. The sort orders 48 bits,
// so the skipped items (all 64 bits set) lie among the entries of the all-ones key, the last ones, in no order: below them a
// binary search on the whole word is exact, and whether the all-ones key itself was given is what the prep pass noted.
__global__ void __launch_bounds__(256) occ_mark_keys_kernel(const unsigned long long* __restrict__ keys, uint32_t slots,
                                                             const unsigned long long* __restrict__ given, uint32_t n, unsigned long long mask,
                                                             uint8_t* __restrict__ remove, OccEditCounts* __restrict__ counts) {
  unsigned marked = 0;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < slots; i += gridDim.x * 256) {
    const unsigned long long key = keys[i];
    if (key == kOccEmpty || remove[i]) continue;
    const unsigned long long want = key & mask;
    bool marks;
    if (want == kOccKeyBits) {
      marks = counts->all_ones != 0;
    } else {
      uint32_t lo = 0, hi = n;   // the first entry not below `want`
      while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (given[mid] < want) lo = mid + 1;
        else hi = mid;
      }
      marks = lo < n && given[lo] == want;
    }
    if (marks) {
      remove[i] = 1;
      marked++;
    }
  }
  occ_block_count(marked, &counts->removed);   // every lane is here
}

struct OccKeyBox { unsigned kmin[3], kmax[3]; int outside; };
__global__ void __launch_bounds__(256) occ_mark_box_kernel(const unsigned long long* __restrict__ keys, uint32_t slots, OccKeyBox b,
                                                            uint8_t* __restrict__ remove, OccEditCounts* __restrict__ counts) {
  unsigned marked = 0;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < slots; i += gridDim.x * 256) {
    const unsigned long long key = keys[i];
    if (key != kOccEmpty && occ_key_in_box(key, b.kmin, b.kmax) != (b.outside != 0)) {
      remove[i] = 1;
      marked++;
    }
  }
  occ_block_count(marked, &counts->removed);   // every lane is here
}

// Forget by age (sbm_occ_stamp_forget): a voxel whose stamp is more than time_thres behind the clock, in octomap's 32-bit wrap
__global__ void __launch_bounds__(256) occ_mark_older_kernel(const unsigned long long* __restrict__ keys, uint32_t slots,
                                                              const unsigned* __restrict__ stamps, uint32_t clock, uint32_t time_thres,
                                                              uint8_t* __restrict__ remove, OccEditCounts* __restrict__ counts) {
  unsigned marked = 0;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < slots; i += gridDim.x * 256) {
    if (keys[i] != kOccEmpty && (uint32_t)(clock - stamps[i]) > time_thres) {
      remove[i] = 1;
      marked++;
    }
  }
  occ_block_count(marked, &counts->removed);   // every lane is here
}

// The move behind the mask: a marked slot stays behind, the others move as a growth moves them. `removed`, the marked slots as the
// marking passes counted them, leaves the size counter in one step.
__global__ void __launch_bounds__(256) occ_remove_kernel(OccRehash r, const uint8_t* __restrict__ remove, unsigned removed) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) atomicSub(&r.ctr->size, removed);
  unsigned long long key = i < r.old_slots ? r.old_keys[i] : kOccEmpty;
  if (key != kOccEmpty && remove[i]) key = kOccEmpty;
  occ_move_lane(r, i, key);   // every lane is here
}

// the same on a stamped map: the stamp word moves with the key
__global__ void __launch_bounds__(256) occ_remove_stamped_kernel(OccRehash r, const uint8_t* __restrict__ remove, unsigned removed,
                                                                  const unsigned* __restrict__ old_stamps, unsigned* __restrict__ stamps) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) atomicSub(&r.ctr->size, removed);
  unsigned long long key = i < r.old_slots ? r.old_keys[i] : kOccEmpty;
  if (key != kOccEmpty && remove[i]) key = kOccEmpty;
  occ_move_lane(r, i, key, old_stamps, stamps);   // every lane is here
}

void occ_remove_launch(sbm_handle* h, const OccRehash& r, const uint8_t* remove, unsigned removed, const unsigned* old_stamps, unsigned* stamps) {
  const dim3 grid((r.old_slots + 255) / 256);
  if (old_stamps) hipLaunchKernelGGL(occ_remove_stamped_kernel, grid, dim3(256), 0, h->stream, r, remove, removed, old_stamps, stamps);
  else hipLaunchKernelGGL(occ_remove_kernel, grid, dim3(256), 0, h->stream, r, remove, removed);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
constexpr size_t kOccEditMax = (size_t)1 << 30;

// The counts of a call that begins, zero, and where a call may delete the clear mask of the table as it is now
static int occ_edit_begin(sbm_occ_map* map, size_t items) {
  sbm_handle* h = map->h;
  HIPCHK(h, map->edit.grow(sizeof(OccEditCounts), h->stream));
  HIPCHK(h, hipMemsetAsync(map->edit.p, 0, sizeof(OccEditCounts), h->stream));
  map->edit_items = items;
  return SBM_OK;
}
static int occ_edit_mask(sbm_occ_map* map) {
  sbm_handle* h = map->h;
  HIPCHK(h, map->edit_mask.grow(map->slots, h->stream));
  HIPCHK(h, hipMemsetAsync(map->edit_mask.p, 0, map->slots, h->stream));
  return SBM_OK;
}
static int occ_edit_counts(sbm_occ_map* map, OccEditCounts* c) {
  sbm_handle* h = map->h;
  HIPCHK(h, hipMemcpyAsync(c, map->edit.p, sizeof(*c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

// What a call that marked ends with: if it removed more than `removed_before`, the move into the table that was allocated before
// anything was applied (b, released either way); the mask is clear again afterwards.
static int occ_edit_settle_removal(sbm_occ_map* map, OccMoveBufs* b, unsigned long long removed_before) {
  OccEditCounts ec;
  int st = occ_edit_counts(map, &ec);
  if (st != SBM_OK || ec.removed == removed_before) {
    occ_move_release(b);
    return st;
  }
  OccCounters c;
  st = occ_move_run(map, map->capacity, b, map->edit_mask.as<uint8_t>(), (unsigned)(ec.removed - removed_before), &c);
  if (st != SBM_OK) return st;
  map->size_bound = c.size;
  return SBM_OK;
}

struct OccEditInput {            // one call's items, in host or device memory
  const unsigned long long* keys;
  const float* xyz;
  const uint8_t* ops;
  const float* values;
  bool host;
};

// One chunk of an edit: `in` points at its first item, all in device memory; deletes: how many delete items it holds
static int occ_edit_chunk_run(sbm_occ_map* map, const OccEditInput& in, uint32_t n, unsigned deletes, OccEdit& e) {
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  OccMoveBufs move = {};
  int st = SBM_OK;
  if (deletes) {   // the move's table before anything is applied
    if ((st = occ_edit_mask(map)) != SBM_OK || (st = occ_move_alloc(map, map->slots, &move)) != SBM_OK) return st;
  }
  const uint32_t tiles = (n + kOccTile - 1) / kOccTile;
  unsigned long long* kk[2];
  unsigned* vv[2];
  hipError_t he = carve(h->occ.sort, h->stream, [&](Carve& c) {
    kk[0] = c.take<unsigned long long>(n), kk[1] = c.take<unsigned long long>(n);
    vv[0] = c.take<unsigned>(n), vv[1] = c.take<unsigned>(n);
    e.slot_of = c.take<uint32_t>(n);
  }, occ_pad);
  if (he == hipSuccess) he = h->occ.hist.grow((size_t)256 * tiles * 4, h->stream);
  if (he != hipSuccess) {
    occ_move_release(&move);
    HIPCHK(h, he);
  }
  e.item_keys = in.keys, e.xyz = in.xyz, e.ops = in.ops, e.values = in.values, e.n = n;
  e.sort_keys = kk[0], e.index = vv[0];
  OccEditCounts* counts = map->edit.as<OccEditCounts>();
  e.counts = counts;
  OccEditCounts before_counts = {};
  if (deletes && (st = occ_edit_counts(map, &before_counts)) != SBM_OK) {
    occ_move_release(&move);
    return st;
  }
  unsigned long long before = 0;
  if (map->grow && (st = occ_overflow_before(map, &before)) != SBM_OK) {
    occ_move_release(&move);
    return st;
  }
  auto fail = [&](int code) {
    occ_move_release(&move);
    return code;
  };
  auto chk = [&](hipError_t err) {
    if (err == hipSuccess) return SBM_OK;
    h->last_hip = (int)err;
    return err == hipErrorOutOfMemory ? SBM_ERR_NOMEM : SBM_ERR_HIP;
  };
  if ((st = chk(clk.mark(kOccBegin, h->stream))) != SBM_OK) return fail(st);
  for (bool again = true; again;) {
    occ_probe(map, &e.mask, &e.max_probe);
    e.keys = map->keys.as<unsigned long long>();
    e.logodds = map->hits.as<float>();
    e.flags = map->flags.as<unsigned>();
    e.change = map->change.as<uint8_t>();
    e.colors = map->color.as<unsigned>();
    e.remove = deletes ? map->edit_mask.as<uint8_t>() : nullptr;
    e.ctr = map->ctr.as<OccCounters>();
    if ((st = chk(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned), h->stream))) != SBM_OK) return fail(st);   // claim_skipped, claim_lost
    hipLaunchKernelGGL(occ_edit_claim_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, e);
    if ((st = chk(hipGetLastError())) != SBM_OK) return fail(st);
    again = false;
    if (map->grow) {
      OccCounters c;
      const uint32_t slots = map->slots;
      if ((st = occ_grow_settle(map, before, &c, &again)) != SBM_OK) return fail(st);
      if (deletes && map->slots != slots) {   // the table grew: the mask and the move's table follow it, still before APPLY
        occ_move_release(&move);
        if ((st = occ_edit_mask(map)) != SBM_OK || (st = occ_move_alloc(map, map->slots, &move)) != SBM_OK) return st;
      }
      if (!again && map->slots != slots) {   // the size alone asked: the slots moved, so the items look theirs up again
        again = true;
        map->redone++;
      }
    }
  }
  if ((st = chk(clk.mark(kOccMid, h->stream))) != SBM_OK) return fail(st);
  if ((st = occ_sort_run(h, kk, vv, n, h->occ.hist.as<unsigned>())) != SBM_OK) return fail(st);
  if (map->stamp.p) hipLaunchKernelGGL(occ_edit_apply_stamped_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, e, map->stamp.as<unsigned>(), map->clock);
  else hipLaunchKernelGGL(occ_edit_apply_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, e);
  if ((st = chk(hipGetLastError())) != SBM_OK) return fail(st);
  if (deletes && (st = occ_edit_settle_removal(map, &move, before_counts.removed)) != SBM_OK) return st;
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(kOccRaysMark, kOccBegin, kOccMid));
  HIPCHK(h, clk.add(kOccRaysApply, kOccMid, kOccEnd));
  return SBM_OK;
}

static int occ_edit_check(const sbm_occ_map* map, size_t n, const void* items, const void* values, const sbm_occ_ray_params* p) {
  if (!map || !p || (n > 0 && (!items || !values))) return SBM_ERR_NULL;
  const int st = occ_ray_params_check(p);
  if (st != SBM_OK) return st;
  if (n > kOccEditMax) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

static int occ_edit_call(sbm_occ_map* map, size_t n, const OccEditInput& in, const sbm_occ_ray_params* p, int sync) {
  if (map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  int st = occ_logodds_alloc(map);
  if (st == SBM_OK) st = occ_edit_begin(map, n);
  if (st != SBM_OK) return st;
  map->mode = kOccModeLogOdds;
  OccEdit e;
  memset(&e, 0, sizeof(e));
  e.factor = 1. / map->p.resolution;
  e.cmin = occ_logodds(p->clamp_min);
  e.cmax = occ_logodds(p->clamp_max);
  e.thres = occ_logodds(p->occupancy_thres);
  e.detect = map->detect && map->change.p;
  HIPCHK(h, occ_clock_start(h, kOccRaysMark, kOccRaysApply));
  const size_t item_bytes = in.keys ? 8 : 12;
  for (size_t c = 0; c < occ_edit_chunks(n); c++) {   // chunk order is item order
    size_t begin, count;
    occ_edit_chunk(n, c, &begin, &count);
    OccEditInput at = {in.keys ? in.keys + begin : nullptr, in.xyz ? in.xyz + 3 * begin : nullptr, in.ops ? in.ops + begin : nullptr,
                       in.values + begin, false};
    unsigned deletes = 0;
    if (in.host) {   // the chunk through the handle's staging
      for (size_t i = 0; in.ops && i < count; i++) deletes += at.ops[i] == SBM_OCC_EDIT_DELETE;
      char* d_items;
      uint8_t* d_ops;
      float* d_values;
      HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& cv) {
        d_items = cv.take<char>(count * item_bytes), d_values = cv.take<float>(count), d_ops = cv.take<uint8_t>(in.ops ? count : 0);
      }, occ_pad));
      HIPCHK(h, hipMemcpyAsync(d_items, in.keys ? (const void*)at.keys : (const void*)at.xyz, count * item_bytes, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(d_values, at.values, count * 4, hipMemcpyHostToDevice, h->stream));
      if (in.ops) HIPCHK(h, hipMemcpyAsync(d_ops, at.ops, count, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));   // the caller's arrays are read
      at = {in.keys ? (const unsigned long long*)d_items : nullptr, in.keys ? nullptr : (const float*)d_items, in.ops ? d_ops : nullptr,
            d_values, false};
    } else if (in.ops) {   // the host has to know whether the chunk may remove before anything is applied
      OccEditCounts* counts = map->edit.as<OccEditCounts>();
      HIPCHK(h, hipMemsetAsync(&counts->deletes, 0, sizeof(unsigned), h->stream));
      hipLaunchKernelGGL(occ_count_deletes_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, at.ops, (uint32_t)count, counts);
      HIPCHK(h, hipGetLastError());
      OccEditCounts ec;
      if ((st = occ_edit_counts(map, &ec)) != SBM_OK) return st;
      deletes = ec.deletes;
    }
    if ((st = occ_edit_chunk_run(map, at, (uint32_t)count, deletes, e)) != SBM_OK) return st;
  }
  // a growth inside the call listed the slots whose flag word said "created"; APPLY cleared the words, and the next scan begins
  // with an empty list, as every scan does
  if (map->grow && n) HIPCHK(h, hipMemsetAsync(&map->ctr.as<OccCounters>()->touched[map->scan & 1], 0, sizeof(unsigned), h->stream));
  return occ_overflow_status(map, sync || in.ops);
}

// The tail of a delete call: clock, the move's table first, `mark` launches the marking, then the move if anything was marked
template <class Mark> static int occ_delete_call(sbm_occ_map* map, size_t items, Mark mark) {
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  const int stage = map->mode == kOccModeHits ? kOccInsert : kOccRaysApply;
  int st = occ_edit_begin(map, items);
  if (st != SBM_OK) return st;
  HIPCHK(h, occ_clock_start(h, stage, stage));
  OccMoveBufs move;
  if ((st = occ_edit_mask(map)) != SBM_OK || (st = occ_move_alloc(map, map->slots, &move)) != SBM_OK) return st;
  hipError_t he = clk.mark(kOccBegin, h->stream);
  if (he == hipSuccess) {
    st = mark();
    if (st == SBM_OK) he = hipGetLastError();
  }
  if (he != hipSuccess || st != SBM_OK) {
    occ_move_release(&move);
    HIPCHK(h, he);
    return st;
  }
  if ((st = occ_edit_settle_removal(map, &move, 0)) != SBM_OK) return st;
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(stage, kOccBegin, kOccEnd));
  return SBM_OK;
}

static int occ_delete_keys(sbm_occ_map* map, size_t n, const unsigned long long* keys, bool host, int depth) {
  uint64_t mask;
  if (!occ_depth_mask(depth, &mask)) return SBM_ERR_UNSUPPORTED;
  if (n > kOccEditMax) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  return occ_delete_call(map, n, [&]() -> int {
    OccEditCounts* counts = map->edit.as<OccEditCounts>();
    for (size_t c = 0; c < occ_edit_chunks(n); c++) {
      size_t begin, count;
      occ_edit_chunk(n, c, &begin, &count);
      const unsigned long long* d_keys = keys + begin;
      if (host) {
        HIPCHK(h, h->occ.io.grow(count * 8, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->occ.io.p, keys + begin, count * 8, hipMemcpyHostToDevice, h->stream));
        d_keys = h->occ.io.as<unsigned long long>();
      }
      const uint32_t m = (uint32_t)count, tiles = (m + kOccTile - 1) / kOccTile;
      unsigned long long* kk[2];
      unsigned* vv[2];
      HIPCHK(h, carve(h->occ.sort, h->stream, [&](Carve& cv) {
        kk[0] = cv.take<unsigned long long>(m), kk[1] = cv.take<unsigned long long>(m), vv[0] = cv.take<unsigned>(m), vv[1] = cv.take<unsigned>(m);
      }, occ_pad));
      HIPCHK(h, h->occ.hist.grow((size_t)256 * tiles * 4, h->stream));
      hipLaunchKernelGGL(occ_delete_prep_kernel, dim3((m + 255) / 256), dim3(256), 0, h->stream, d_keys, m, (unsigned long long)mask, kk[0], vv[0], counts);
      HIPCHK(h, hipGetLastError());
      const int st = occ_sort_run(h, kk, vv, m, h->occ.hist.as<unsigned>());
      if (st != SBM_OK) return st;
      hipLaunchKernelGGL(occ_mark_keys_kernel, dim3(std::min((map->slots + 255) / 256, kOccMarkBlocks)), dim3(256), 0, h->stream, map->keys.as<unsigned long long>(),
                         map->slots, kk[0], m, (unsigned long long)mask, map->edit_mask.as<uint8_t>(), counts);
      HIPCHK(h, hipGetLastError());
      if (host) HIPCHK(h, hipStreamSynchronize(h->stream));   // the staging is free for the next chunk
    }
    return SBM_OK;
  });
}

}  // namespace sbm
using namespace sbm;

extern "C" {

int sbm_occ_edit_device(sbm_occ_map* map, size_t n, const void* d_keys, const void* d_ops, const void* d_values,
                        const sbm_occ_ray_params* params, int sync) {
  const int st = occ_edit_check(map, n, d_keys, d_values, params);
  if (st != SBM_OK) return st;
  if (((uintptr_t)d_keys & 7) || ((uintptr_t)d_values & 3)) return SBM_ERR_UNSUPPORTED;
  return occ_edit_call(map, n, {(const unsigned long long*)d_keys, nullptr, (const uint8_t*)d_ops, (const float*)d_values, false}, params, sync);
}

int sbm_occ_edit(sbm_occ_map* map, size_t n, const uint64_t* keys, const uint8_t* ops, const float* values, const sbm_occ_ray_params* params) {
  const int st = occ_edit_check(map, n, keys, values, params);
  if (st != SBM_OK) return st;
  return occ_edit_call(map, n, {(const unsigned long long*)keys, nullptr, ops, values, true}, params, 1);
}

int sbm_occ_edit_points_device(sbm_occ_map* map, size_t n, const void* d_xyz, const void* d_ops, const void* d_values,
                               const sbm_occ_ray_params* params, int sync) {
  const int st = occ_edit_check(map, n, d_xyz, d_values, params);
  if (st != SBM_OK) return st;
  if (((uintptr_t)d_xyz & 3) || ((uintptr_t)d_values & 3)) return SBM_ERR_UNSUPPORTED;
  return occ_edit_call(map, n, {nullptr, (const float*)d_xyz, (const uint8_t*)d_ops, (const float*)d_values, false}, params, sync);
}

int sbm_occ_edit_points(sbm_occ_map* map, size_t n, const float* xyz, const uint8_t* ops, const float* values, const sbm_occ_ray_params* params) {
  const int st = occ_edit_check(map, n, xyz, values, params);
  if (st != SBM_OK) return st;
  return occ_edit_call(map, n, {nullptr, xyz, ops, values, true}, params, 1);
}

int sbm_occ_delete_device(sbm_occ_map* map, size_t n, const void* d_keys, int depth) {
  if (!map || (n > 0 && !d_keys)) return SBM_ERR_NULL;
  if ((uintptr_t)d_keys & 7) return SBM_ERR_UNSUPPORTED;
  return occ_delete_keys(map, n, (const unsigned long long*)d_keys, false, depth);
}

int sbm_occ_delete(sbm_occ_map* map, size_t n, const uint64_t* keys, int depth) {
  if (!map || (n > 0 && !keys)) return SBM_ERR_NULL;
  return occ_delete_keys(map, n, (const unsigned long long*)keys, true, depth);
}

int sbm_occ_delete_box(sbm_occ_map* map, const uint16_t min_key[3], const uint16_t max_key[3], int outside) {
  if (!map || !min_key || !max_key) return SBM_ERR_NULL;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  OccKeyBox b;
  for (int i = 0; i < 3; i++) b.kmin[i] = min_key[i], b.kmax[i] = max_key[i];
  b.outside = outside;
  return occ_delete_call(map, 0, [&]() -> int {
    hipLaunchKernelGGL(occ_mark_box_kernel, dim3(std::min((map->slots + 255) / 256, kOccMarkBlocks)), dim3(256), 0, h->stream, map->keys.as<unsigned long long>(), map->slots,
                       b, map->edit_mask.as<uint8_t>(), map->edit.as<OccEditCounts>());
    return SBM_OK;
  });
}

int sbm_occ_stamp_forget(sbm_occ_map* map, uint32_t time_thres, uint64_t* removed) {
  if (!map) return SBM_ERR_NULL;
  if (!map->stamp.p) return SBM_ERR_UNSUPPORTED;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  int st = occ_delete_call(map, 0, [&]() -> int {
    hipLaunchKernelGGL(occ_mark_older_kernel, dim3(std::min((map->slots + 255) / 256, kOccMarkBlocks)), dim3(256), 0, h->stream, map->keys.as<unsigned long long>(),
                       map->slots, map->stamp.as<unsigned>(), map->clock, time_thres, map->edit_mask.as<uint8_t>(), map->edit.as<OccEditCounts>());
    return SBM_OK;
  });
  if (st != SBM_OK || !removed) return st;
  OccEditCounts c;
  if ((st = occ_edit_counts(map, &c)) == SBM_OK) *removed = c.removed;
  return st;
}

int sbm_occ_last_edit(sbm_occ_map* map, sbm_occ_edit_info* out) {
  if (!map || !out) return SBM_ERR_NULL;
  sbm_handle* h = map->h;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  OccEditCounts c = {};
  if (map->edit.p) {
    const int st = occ_edit_counts(map, &c);
    if (st != SBM_OK) return st;
  }
  out->items = map->edit_items;
  out->skipped = c.skipped;
  out->lost = c.lost;
  out->created = c.created;
  out->removed = c.removed;
  return SBM_OK;
}

}  // extern "C"
