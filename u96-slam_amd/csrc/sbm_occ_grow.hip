// sbm_occ_grow.hip -- the occupancy map's growth: the table rehashed into a larger one on the device, the policy that says how
// large, and the claim pass that lets the hit insert, whose counts cannot be added twice, learn that a launch fits before it
// runs.  gfx950. include/sbm.h ("occupancy map: growth") states the contract; a map that never enables growth and never
// reserves launches nothing of this file.
//
//   occ_rehash_kernel   one lane per old slot (occ_move_lane, sbm_occ.h): a stored key takes its place in the new table
//                       (occ_find_or_claim: keys are distinct, so every compare-and-swap on an empty slot claims) and carries its
//                       32-bit word, its flag word and its change byte; a slot whose flag word is set enters the running scan's
//                       touched list. The edits' move (sbm_occ_edit.hip) is the same lane behind a removal mask.
//   occ_claim_kernel    the hit insert's front half: pixel -> point -> gate -> key, the wavefront's leaders claim their keys and
//                       count those that found no slot. It adds no hit, so it can run again on a larger table.
#include "sbm_occ.h"

namespace sbm {
#pragma clang fp contract(off)

constexpr size_t kOccGrowMax = (size_t)1 << 30;   // sbm_occ_create's limit
constexpr int kOccClaimChunk = 64;                // as the insert's launches: the poses travel as kernel arguments
struct OccClaimPoses { float t[kOccClaimChunk][12]; };

__global__ void __launch_bounds__(256) occ_rehash_kernel(OccRehash r) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  occ_move_lane(r, i, i < r.old_slots ? r.old_keys[i] : kOccEmpty);
}
// the same on a stamped map (sbm_occ_stamp.hip): the stamp word moves with the key
__global__ void __launch_bounds__(256) occ_rehash_stamped_kernel(OccRehash r, const unsigned* __restrict__ old_stamps, unsigned* __restrict__ stamps) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  occ_move_lane(r, i, i < r.old_slots ? r.old_keys[i] : kOccEmpty, old_stamps, stamps);
}

__global__ void __launch_bounds__(256) occ_claim_kernel(const int16_t* __restrict__ disp, OccGeom g, sbm_stereo_model m, OccClaimPoses poses,
                                                         unsigned long long* __restrict__ keys, OccCounters* __restrict__ ctr) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  unsigned long long key = kOccEmpty;
  const float* pose = poses.t[blockIdx.y];
  Pt3 p;
  if (i < g.W * g.H && occ_world_point(disp + (size_t)blockIdx.y * g.W * g.H, i, g, m, pose, &p)) {
    const float vx = p.x - pose[3], vy = p.y - pose[7], vz = p.z - pose[11];
    const float nsq = vx * vx + vy * vy + vz * vz;          // the gate of occ_insert_kernel, expression for expression
    unsigned k0, k1, k2;
    if (__dsqrt_rn((double)nsq) <= (double)g.range_max_sqrd && occ_axis(g.factor, p.x, &k0) && occ_axis(g.factor, p.y, &k1) &&
        occ_axis(g.factor, p.z, &k2))
      key = occ_pack(k0, k1, k2);
  }
  // the wavefront's distinct keys: the lowest lane of each value leads
  const int lane = threadIdx.x & 63;
  const unsigned lo = (unsigned)key, hi = (unsigned)(key >> 32);
  unsigned long long todo = __ballot(key != kOccEmpty);
  bool leads = false;
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned llo = __builtin_amdgcn_readlane(lo, leader), lhi = __builtin_amdgcn_readlane(hi, leader);
    const unsigned long long same = __ballot(lo == llo && hi == lhi);
    if (lane == leader) leads = true;
    todo &= ~same;
  }
  if (!leads) return;
  uint32_t slot;
  bool claimed = false;
  const bool found = occ_find_or_claim(keys, key, g.mask, g.max_probe, &slot, &claimed);
  if (claimed) atomicAdd(&ctr->size, 1u);
  if (!found) atomicAdd(&ctr->overflow, 1ull);
}

static size_t occ_ceiling(const sbm_occ_map* map) { return map->max_capacity ? map->max_capacity : kOccGrowMax; }

bool occ_can_reserve(const sbm_occ_map* map, size_t voxels) { return map->grow && voxels <= occ_ceiling(map); }

int occ_overflow_before(sbm_occ_map* map, unsigned long long* before) {
  if (!map->overflow_known) {
    OccCounters c;
    const int st = occ_read_counters(map, &c);
    if (st != SBM_OK) return st;
    map->overflow = c.overflow;
    map->overflow_known = true;
  }
  *before = map->overflow;
  return SBM_OK;
}

int occ_set_overflow(sbm_occ_map* map, unsigned long long value) {
  sbm_handle* h = map->h;
  map->overflow = value;       // the copy reads the map's own word, which outlives it
  map->overflow_known = true;
  HIPCHK(h, hipMemcpyAsync(&map->ctr.as<OccCounters>()->overflow, &map->overflow, sizeof(value), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

void occ_move_release(OccMoveBufs* b) {
  for (DevBuf* d : {&b->keys, &b->vals, &b->flags, &b->touched, &b->change, &b->color}) d->release();
  if (b->stamp.p) b->stamp.release();   // a map without stamps makes the calls it made before
}

// the new buffers beside the old ones: a refused allocation frees what it got and leaves the map as it was
int occ_move_alloc(sbm_occ_map* map, uint32_t slots, OccMoveBufs* b) {
  sbm_handle* h = map->h;
  *b = OccMoveBufs{};
  b->slots = slots;
  hipError_t e = b->keys.grow((size_t)slots * 8, h->stream);
  if (e == hipSuccess) e = b->vals.grow((size_t)slots * 4, h->stream);
  if (e == hipSuccess && map->flags.p) e = b->flags.grow((size_t)slots * 4, h->stream);
  if (e == hipSuccess && map->touched.p) e = b->touched.grow((size_t)slots * 4, h->stream);
  if (e == hipSuccess && map->change.p) e = b->change.grow(slots, h->stream);
  if (e == hipSuccess && map->color.p) e = b->color.grow((size_t)slots * 4, h->stream);
  if (e == hipSuccess && map->stamp.p) e = b->stamp.grow((size_t)slots * 4, h->stream);
  if (e == hipSuccess) return SBM_OK;
  occ_move_release(b);
  h->last_hip = (int)e;
  return e == hipErrorOutOfMemory ? SBM_ERR_NOMEM : SBM_ERR_HIP;
}

int occ_move_run(sbm_occ_map* map, size_t capacity, OccMoveBufs* b, const uint8_t* remove, unsigned removed, OccCounters* c) {
  sbm_handle* h = map->h;
  const uint32_t slots = b->slots;
  DevBuf &keys = b->keys, &vals = b->vals, &flags = b->flags, &touched = b->touched, &change = b->change, &color = b->color, &stamp = b->stamp;
  hipError_t e = hipMemsetAsync(keys.p, 0xFF, (size_t)slots * 8, h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(vals.p, 0, (size_t)slots * 4, h->stream);
  if (e == hipSuccess && flags.p) e = hipMemsetAsync(flags.p, 0, (size_t)slots * 4, h->stream);
  if (e == hipSuccess && change.p) e = hipMemsetAsync(change.p, 0, slots, h->stream);
  if (e == hipSuccess && color.p) e = hipMemsetD32Async((hipDeviceptr_t)color.p, (int)kOccWhite, slots, h->stream);
  if (e == hipSuccess && stamp.p) e = hipMemsetAsync(stamp.p, 0, (size_t)slots * 4, h->stream);
  OccRehash r;
  r.parity = map->scan & 1;
  OccCounters* ctr = map->ctr.as<OccCounters>();
  if (e == hipSuccess) e = hipMemsetAsync(&ctr->touched[r.parity], 0, sizeof(unsigned), h->stream);   // the kernel counts the list anew
  if (e == hipSuccess) {
    r.old_keys = map->keys.as<unsigned long long>();
    r.old_vals = map->hits.as<unsigned>();
    r.old_flags = map->flags.as<unsigned>();
    r.old_change = map->change.as<uint8_t>();
    r.old_colors = color.p ? map->color.as<unsigned>() : nullptr;
    r.old_slots = map->slots;
    r.keys = keys.as<unsigned long long>();
    r.vals = vals.as<unsigned>();
    r.flags = flags.as<unsigned>();
    r.change = change.as<uint8_t>();
    r.colors = color.as<unsigned>();
    r.touched = touched.as<unsigned>();
    r.mask = slots - 1;
    r.max_probe = std::min(slots, kOccMaxProbe);
    r.slots = slots;
    r.ctr = ctr;
    if (!r.touched) r.old_flags = nullptr;   // no list, no flags: the log-odds mode allocates both
    const unsigned* old_stamps = stamp.p ? map->stamp.as<unsigned>() : nullptr;   // the word moves only where it exists
    if (remove) occ_remove_launch(h, r, remove, removed, old_stamps, stamp.as<unsigned>());
    else if (old_stamps) hipLaunchKernelGGL(occ_rehash_stamped_kernel, dim3((map->slots + 255) / 256), dim3(256), 0, h->stream, r, old_stamps, stamp.as<unsigned>());
    else hipLaunchKernelGGL(occ_rehash_kernel, dim3((map->slots + 255) / 256), dim3(256), 0, h->stream, r);
    e = hipGetLastError();
  }
  *c = OccCounters{};
  if (e == hipSuccess) e = hipMemcpyAsync(c, ctr, sizeof(*c), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);   // the old table is read no more
  if (e != hipSuccess) {
    occ_move_release(b);
    h->last_hip = (int)e;
    return e == hipErrorOutOfMemory ? SBM_ERR_NOMEM : SBM_ERR_HIP;
  }
  std::swap(map->keys, keys);
  std::swap(map->hits, vals);
  if (flags.p) std::swap(map->flags, flags);
  if (touched.p) std::swap(map->touched, touched);
  if (change.p) std::swap(map->change, change);
  if (color.p) std::swap(map->color, color);
  if (stamp.p) std::swap(map->stamp, stamp);
  occ_move_release(b);
  map->capacity = capacity;
  map->slots = slots;
  if (map->overflow_known && c->overflow != map->overflow) map->overflow_known = false;
  return SBM_OK;
}

int occ_rehash(sbm_occ_map* map, size_t capacity) {
  uint32_t slots = 2;
  while ((size_t)slots < 2 * capacity) slots <<= 1;
  OccMoveBufs b;
  OccCounters c;
  int st = occ_move_alloc(map, slots, &b);
  if (st == SBM_OK) st = occ_move_run(map, capacity, &b, nullptr, 0, &c);
  if (st != SBM_OK) return st;
  map->grown++;
  map->moved += c.size;
  return SBM_OK;
}

int occ_grow_settle(sbm_occ_map* map, unsigned long long before, OccCounters* c, bool* again) {
  *again = false;
  int st = occ_read_counters(map, c);
  if (st != SBM_OK) return st;
  const bool lost = c->overflow > before;
  map->overflow = c->overflow;
  map->overflow_known = true;
  if (!lost && c->size <= map->capacity) return SBM_OK;
  // A lost cell says the scan is still adding voxels: twice the size it has reached, which a full table (size = slots) turns
  // into four times the capacity, and which stays within four times whatever the size ends at.
  size_t next;
  if (sbm_occ_growth_step(map->capacity, lost ? 2 * (size_t)c->size : c->size, map->max_capacity, &next) != SBM_OK) return SBM_OK;   // at the ceiling
  st = occ_rehash(map, next);
  if (st == SBM_ERR_NOMEM) return SBM_OK;   // refused: the call goes on with the table it has, the error is in last_hip
  if (st != SBM_OK || !lost) return st;     // the size alone asked: flags and list moved with the keys, nothing is redone
  st = occ_set_overflow(map, before);
  if (st != SBM_OK) return st;
  map->redone++;
  *again = true;
  return SBM_OK;
}

// The hit insert's claim pass over m planes (sbm_occupancy.hip launches it where a growing map cannot show that they fit)
int occ_claim_launch(sbm_occ_map* map, const int16_t* d_disp, const OccGeom& g, const sbm_stereo_model* model, const float* poses, int m) {
  sbm_handle* h = map->h;
  OccClaimPoses ps;
  memset(&ps, 0, sizeof(ps));
  memcpy(ps.t, poses, sizeof(float) * 12 * m);
  const size_t plane = (size_t)g.W * g.H;
  hipLaunchKernelGGL(occ_claim_kernel, dim3((unsigned)((plane + 255) / 256), m), dim3(256), 0, h->stream, d_disp, g, *model, ps,
                     map->keys.as<unsigned long long>(), map->ctr.as<OccCounters>());
  HIPCHK(h, hipGetLastError());
  return SBM_OK;
}

}  // namespace sbm
using namespace sbm;

extern "C" {

int sbm_occ_growth_step(size_t capacity, size_t need, size_t max_capacity, size_t* next) {
  if (!next) return SBM_ERR_NULL;
  const size_t ceiling = max_capacity && max_capacity < kOccGrowMax ? max_capacity : kOccGrowMax;
  if (capacity >= ceiling) return SBM_ERR_OCC_FULL;
  size_t n = std::max<size_t>(2 * capacity, 1);
  if (n < need) n = need;
  *next = std::min(n, ceiling);
  return SBM_OK;
}

int sbm_occ_capacity(sbm_occ_map* map, size_t* capacity) {
  if (!map || !capacity) return SBM_ERR_NULL;
  *capacity = map->capacity;
  return SBM_OK;
}

int sbm_occ_reserve(sbm_occ_map* map, size_t capacity) {
  if (!map) return SBM_ERR_NULL;
  if (capacity <= map->capacity) return SBM_OK;
  if (capacity > kOccGrowMax) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_rehash(map, capacity);
}

int sbm_occ_set_growth(sbm_occ_map* map, int enable, size_t max_capacity) {
  if (!map) return SBM_ERR_NULL;
  if (max_capacity > kOccGrowMax) return SBM_ERR_UNSUPPORTED;
  map->grow = enable != 0;
  map->max_capacity = max_capacity;
  map->overflow_known = false;   // inserts with growth off do not keep the host's copy
  return SBM_OK;
}

int sbm_occ_get_growth(sbm_occ_map* map, sbm_occ_growth_info* out) {
  if (!map || !out) return SBM_ERR_NULL;
  memset(out, 0, sizeof(*out));
  out->enabled = map->grow ? 1 : 0;
  out->capacity = map->capacity;
  out->slots = map->slots;
  out->max_capacity = occ_ceiling(map);
  out->grown = map->grown;
  out->moved = map->moved;
  out->redone = map->redone;
  return SBM_OK;
}

}  // extern "C"
