// sbm_occ_rays.hip -- the occupancy map's log-odds mode, octomap's insertPointCloud per scan (OccupancyOcTreeBase.hxx:86-102,
// computeUpdate :169-270), for a cloud or for the planes of the hit insert.  gfx950. Nothing here contracts a multiply-add.
//
//   occ_rays_mark_*_kernel   one lane per ray walks computeRayKeys' 3-D DDA in registers and ORs "free" / "occupied this scan" into the
//                       flag word of every cell's slot; the lane whose OR found the word clear appends the slot to the touched list.
//   occ_rays_apply_kernel   gives every touched slot its ONE update (occupied wins) and clears the flags.
// The insert options (include/sbm.h, "occupancy map: insert options") are template parameters of these kernels: kBox tests
// every cell against the bounding box before it is marked, kTrack carries "created this scan" from the claiming lane to APPLY,
// which steps the slot's change state. The <false, false> instantiations are the kernels without options.
//   occ_dedupe_*_kernel     discretize: one lane per point claims its wrapped key in the scan's scratch set; the claiming lane
//                       appends the key to a list, from which occ_rays_mark_list_kernel casts one ray per voxel centre.
#include <type_traits>

#include "sbm_occ.h"

namespace sbm {
#pragma clang fp contract(off)

struct OccRay {                 // one call's constants
  double max_range;             // < 0: no limit
  double resolution, factor;    // factor = 1. / resolution
  float hit, miss, cmin, cmax;  // log-odds
  uint32_t mask, max_probe, slots;
  uint32_t parity;              // which of OccCounters::touched counts this scan
  float thres;                  // kTrack: isNodeOccupied is logodds >= thres
  float bmin[3], bmax[3];       // kBox: inBBX(point), in float
  unsigned kmin[3], kmax[3];    //       inBBX(key)
};
struct OccTable {
  unsigned long long* keys;
  float* logodds;
  unsigned* flags;
  unsigned* touched;
  OccCounters* ctr;
  uint8_t* change;              // kTrack: a change state per slot
};
struct OccDedupe {                // one discretised scan's scratch
  unsigned long long* set;        // open addressing over `slots` entries (a power of two, at least twice the points)
  unsigned long long* list;       // the distinct keys, in no order
  unsigned* count;
  uint32_t slots, cap;            // entries of the set, of the list (the scan's points)
};

// The whole wavefront calls this once per step (have: this lane has a cell). Finds or claims the cell's slot and ORs `bit` into
// its flag word -- after reading it: thousands of rays share their first cells, and a set bit needs no atomic. The lanes whose OR
// found the word clear append their slots to the scan's touched list, one atomic on the list's counter per wavefront. A cell
// that finds no slot within the probe bound is counted as overflow.
template <bool kTrack>
__device__ __forceinline__ void occ_mark_cell(unsigned long long key, unsigned bit, bool have, const OccRay& g, const OccTable& t) {
  bool fresh = false;
  uint32_t slot = 0;
  if (have) {
    bool claimed = false;
    const bool found = occ_find_or_claim(t.keys, key, g.mask, g.max_probe, &slot, &claimed);
    if (claimed) atomicAdd(&t.ctr->size, 1u);
    if (found) {
      // kTrack: the claiming lane brings "created" with its bit. Another lane may have found the key and set its own bit first;
      // then that lane is the fresh one, and this OR still lands before APPLY.
      const unsigned bits = kTrack && claimed ? bit | kOccCreated : bit;
      unsigned old = __hip_atomic_load(&t.flags[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((old & bits) != bits) {
        old = atomicOr(&t.flags[slot], bits);
        fresh = old == 0;
      }
    } else {
      atomicAdd(&t.ctr->overflow, 1ull);
    }
  }
  const uint32_t at = occ_wave_append(fresh, &t.ctr->touched[g.parity]);
  if (fresh && at < g.slots) t.touched[at] = slot;   // a slot is appended once per scan: the list of `slots` entries always has room
}

// One ray of computeUpdate, by the whole wavefront (valid: this lane has a point): the range gate, the truncated end beyond it,
// computeRayKeys (OcTreeBaseImpl.hxx:542-648) with every cell marked free as the DDA reaches it, and the end point marked occupied.
// kBox (computeUpdate's second branch, OccupancyOcTreeBase.hxx:222-259): the end point also has to be in the float box, and the
// first cell outside the key box, the origin's included, ends the ray.
template <bool kBox, bool kTrack>
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
    if (kBox) ends = ends && p.x >= g.bmin[0] && p.y >= g.bmin[1] && p.z >= g.bmin[2] && p.x <= g.bmax[0] && p.y <= g.bmax[1] && p.z <= g.bmax[2];
    if (end_ok && occ_axis(g.factor, ox, &c0) && occ_axis(g.factor, oy, &c1) && occ_axis(g.factor, oz, &c2) &&
        !(c0 == e0 && c1 == e1 && c2 == e2)) {
      walking = true;
      float dx = end.x - ox, dy = end.y - oy, dz = end.z - oz;
      const float len = (float)__dsqrt_rn((double)(dx * dx + dy * dy + dz * dz));
      dx /= len;
      dy /= len;
      dz /= len;
      length = (double)len;
      occ_dda_axis<true>(dx, c0, ox, g.resolution, &s0, &t0, &d0);   // computeRayKeys, OcTreeBaseImpl.hxx:577-596: the half
      occ_dda_axis<true>(dy, c1, oy, g.resolution, &s1, &t1, &d1);   // cell is rounded to float
      occ_dda_axis<true>(dz, c2, oz, g.resolution, &s2, &t2, &d2);
    }
  }
  // The origin cell first, then one cell per step until the end cell's key or the ray's length is reached; the end cell is not
  // part of the ray. The step count is bounded whatever the input: the wavefront leaves the loop when its last lane has.
  int steps = 0;
  while (__ballot(walking)) {
    if (kBox && walking && !(c0 >= g.kmin[0] && c1 >= g.kmin[1] && c2 >= g.kmin[2] && c0 <= g.kmax[0] && c1 <= g.kmax[1] && c2 <= g.kmax[2]))
      walking = false;   // the lane stays in the loop's shape: every lane of the wavefront reaches the append below
    occ_mark_cell<kTrack>(occ_pack(c0, c1, c2), kOccFree, walking, g, t);
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
  occ_mark_cell<kTrack>(occ_pack(e0, e1, e2), kOccOccupied, ends, g, t);
}

// mark, cloud form: one lane per point of d_xyz
template <bool kBox, bool kTrack>
__global__ void __launch_bounds__(256) occ_rays_mark_cloud_kernel(const float* __restrict__ xyz, size_t n, OccPose origin, OccRay g,
                                                                   OccTable t) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  Pt3 p = nan3();
  if (i < n) p = Pt3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  const float o[3] = {origin.t[3], origin.t[7], origin.t[11]};
  occ_cast_ray<kBox, kTrack>(i < n, p, o, g, t);
}

// mark, plane form: one lane per pixel of one plane, through the front half of the hit insert; the origin is the pose's translation
template <bool kBox, bool kTrack>
__global__ void __launch_bounds__(256) occ_rays_mark_plane_kernel(const int16_t* __restrict__ plane, OccGeom pg, sbm_stereo_model m,
                                                                   OccPose pose, OccRay g, OccTable t) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  Pt3 p = nan3();
  const bool valid = i < pg.W * pg.H && occ_world_point(plane, i, pg, m, pose.t, &p);
  const float o[3] = {pose.t[3], pose.t[7], pose.t[11]};
  occ_cast_ray<kBox, kTrack>(valid, p, o, g, t);
}

// discretize (computeDiscreteUpdate, OccupancyOcTreeBase.hxx:148-165). The whole wavefront calls this (valid: this lane has a
// point): the point's wrapped key is claimed in the scan's set, and the lanes that claimed append it to the list. The set has at
// least twice as many entries as the scan has points and is empty when the scan begins, so the walk over all of it finds a place.
__device__ __forceinline__ void occ_dedupe_point(bool valid, Pt3 p, double factor, const OccDedupe& d) {
  bool claimed = false;
  unsigned k0 = 0, k1 = 0, k2 = 0;
  if (valid && occ_axis_wrapped(factor, p.x, &k0) && occ_axis_wrapped(factor, p.y, &k1) && occ_axis_wrapped(factor, p.z, &k2)) {
    uint32_t at;
    occ_find_or_claim(d.set, occ_pack(k0, k1, k2), d.slots - 1, d.slots, &at, &claimed);
  }
  const uint32_t at = occ_wave_append(claimed, d.count);
  if (claimed && at < d.cap) d.list[at] = occ_pack(k0, k1, k2);
}
__global__ void __launch_bounds__(256) occ_dedupe_cloud_kernel(const float* __restrict__ xyz, size_t n, double factor, OccDedupe d) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  Pt3 p = nan3();
  if (i < n) p = Pt3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  occ_dedupe_point(i < n, p, factor, d);
}
__global__ void __launch_bounds__(256) occ_dedupe_plane_kernel(const int16_t* __restrict__ plane, OccGeom pg, sbm_stereo_model m,
                                                                OccPose pose, double factor, OccDedupe d) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  Pt3 p = nan3();
  const bool valid = i < pg.W * pg.H && occ_world_point(plane, i, pg, m, pose.t, &p);
  occ_dedupe_point(valid, p, factor, d);
}
// mark, list form: one lane per distinct key of a discretised scan, the voxel's centre (keyToCoord) as its point. The grid is
// sized for the scan's points; the lanes beyond the list's count idle.
template <bool kBox, bool kTrack>
__global__ void __launch_bounds__(256) occ_rays_mark_list_kernel(OccDedupe d, OccPose origin, OccRay g, OccTable t) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < min(*d.count, d.cap);
  Pt3 p = nan3();
  if (valid) {
    const unsigned long long k = d.list[i];
    p = Pt3{occ_key_coord((unsigned)(k >> 32) & 0xFFFF, g.resolution), occ_key_coord((unsigned)(k >> 16) & 0xFFFF, g.resolution),
            occ_key_coord((unsigned)k & 0xFFFF, g.resolution)};
  }
  const float o[3] = {origin.t[3], origin.t[7], origin.t[11]};
  occ_cast_ray<kBox, kTrack>(valid, p, o, g, t);
}

// apply: every slot the scan touched gets its one update (updateNodeLogOdds, OccupancyOcTreeBase.hxx:1097-1106; an absent voxel
// starts at 0, which is what a fresh slot holds), occupied before free, and its flag word is cleared for the next scan. The
// early return of updateNode for a leaf at its clamp gives what the clamp gives. No atomics: a slot is in the list once. The
// two counts of OccCounters::touched take turns, so that no scan needs a memset between its two launches and the next scan's.
// kTrack (updateNodeRecurs, OccupancyOcTreeBase.hxx:415-427): a slot the scan claimed becomes `created`; another whose
// isNodeOccupied differs before and after the update goes none -> flipped -> none, and a created one stays.
// kStamp (OcTreeStamped::updateNodeLogOdds; sbm.h, "occupancy map: time stamps per voxel"): the slot's stamp word becomes the map's
// clock unless updateNode's early return applies -- the voxel existed before the scan (MARK's "created" bit is clear) and sits at
// the clamp in the direction of its update. A plain store by the one lane that owns the slot. The instantiations without kStamp are
// the kernels of a map without stamps, statement for statement.
template <bool kTrack, bool kStamp>
__device__ __forceinline__ void occ_rays_apply(const OccRay& g, const OccTable& t, unsigned* __restrict__ stamps, uint32_t clock) {
#pragma clang fp contract(off)
  const uint32_t n = min(t.ctr->touched[g.parity], g.slots);
  if (blockIdx.x == 0 && threadIdx.x == 0) t.ctr->touched[g.parity ^ 1] = 0;   // the next scan's count; nobody reads it now
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t slot = t.touched[i];
    if (slot >= g.slots) continue;
    const unsigned f = t.flags[slot];
    const float before = t.logodds[slot];
    float v = before + ((f & kOccOccupied) ? g.hit : g.miss);
    if (v < g.cmin) v = g.cmin;
    else if (v > g.cmax) v = g.cmax;
    t.logodds[slot] = v;
    t.flags[slot] = 0;
    if (kStamp) {
      const float u = (f & kOccOccupied) ? g.hit : g.miss;
      const bool early = !(f & kOccCreated) && ((u >= 0.f && before >= g.cmax) || (u <= 0.f && before <= g.cmin));
      if (!early) stamps[slot] = clock;
    }
    if (kTrack) {
      if (f & kOccCreated) {
        t.change[slot] = kOccChangeCreated;
      } else if ((before >= g.thres) != (v >= g.thres)) {
        const uint8_t s = t.change[slot];
        if (s != kOccChangeCreated) t.change[slot] = s == kOccChangeNone ? kOccChangeFlipped : kOccChangeNone;
      }
    }
  }
}
template <bool kTrack> __global__ void __launch_bounds__(256) occ_rays_apply_kernel(OccRay g, OccTable t) {
  occ_rays_apply<kTrack, false>(g, t, nullptr, 0u);
}
template <bool kTrack>
__global__ void __launch_bounds__(256) occ_rays_apply_stamped_kernel(OccRay g, OccTable t, unsigned* __restrict__ stamps, uint32_t clock) {
  occ_rays_apply<kTrack, true>(g, t, stamps, clock);
}

// ---- log-odds mode, host side ----------------------------------------------------------------------------------------------
float occ_logodds(double p) { return (float)log(p / (1. - p)); }   // octomap_utils.h

int occ_ray_params_check(const sbm_occ_ray_params* p) {
  if (!p) return SBM_ERR_NULL;
  const double prob[5] = {p->prob_hit, p->prob_miss, p->clamp_min, p->clamp_max, p->occupancy_thres};
  for (double v : prob)
    if (!(v > 0. && v < 1.)) return SBM_ERR_SIZE;   // NaN fails both
  if (p->prob_hit < 0.5 || p->prob_miss > 0.5 || !(p->clamp_min < p->clamp_max) || std::isnan(p->max_range)) return SBM_ERR_SIZE;
  return SBM_OK;
}

// What the log-odds mode keeps beside the table, 8 B per slot: the flag words, clear between scans, and the touched list
int occ_logodds_alloc(sbm_occ_map* map) {
  sbm_handle* h = map->h;
  if (!map->flags.p) {
    HIPCHK(h, map->flags.grow((size_t)map->slots * 4, h->stream));
    HIPCHK(h, hipMemsetAsync(map->flags.p, 0, (size_t)map->slots * 4, h->stream));
  }
  HIPCHK(h, map->touched.grow((size_t)map->slots * 4, h->stream));
  return SBM_OK;
}

// The table as a scan's launches see it: its walk and its arrays. A growing map states it again after every growth.
static void occ_rays_table(sbm_occ_map* map, OccRay* g, OccTable* t) {
  occ_probe(map, &g->mask, &g->max_probe);
  g->slots = map->slots;
  t->keys = map->keys.as<unsigned long long>();
  t->logodds = map->hits.as<float>();
  t->flags = map->flags.as<unsigned>();
  t->touched = map->touched.as<unsigned>();
  t->ctr = map->ctr.as<OccCounters>();
  t->change = map->change.as<uint8_t>();
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
  g->parity = 0;
  g->thres = occ_logodds(p->occupancy_thres);
  for (int i = 0; i < 3; i++) {
    g->bmin[i] = map->bbx_min[i], g->bmax[i] = map->bbx_max[i];
    g->kmin[i] = map->bbx_min_key[i], g->kmax[i] = map->bbx_max_key[i];
  }
  occ_rays_table(map, g, t);
  return SBM_OK;
}

// f(box, track) with the map's two switches as compile-time constants: which instantiation of a mark or apply kernel runs
template <class F> static void occ_with_options(const sbm_occ_map* map, F f) {
  if (map->use_bbx) {
    if (map->detect) f(std::true_type{}, std::true_type{});
    else f(std::true_type{}, std::false_type{});
  } else {
    if (map->detect) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
  }
}

// The same for a MARK launch. On a stamped map MARK always carries "created this scan" (the kTrack instantiations, which exist
// already): the stamped APPLY needs it for updateNode's early return, and the plain APPLY clears the bit with the others.
template <class F> static void occ_with_mark_options(const sbm_occ_map* map, F f) {
  if (!map->stamp.p) return occ_with_options(map, f);
  if (map->use_bbx) f(std::true_type{}, std::true_type{});
  else f(std::false_type{}, std::true_type{});
}

// The scratch of one discretised scan of n points, placed in the map's dedupe buffer: the set, the list and its count
static int occ_dedupe_begin(sbm_occ_map* map, size_t n, OccDedupe* d) {
  sbm_handle* h = map->h;
  d->cap = (uint32_t)n;
  d->slots = 2;
  while ((size_t)d->slots < 2 * n) d->slots <<= 1;
  HIPCHK(h, carve(map->dedupe, h->stream, [&](Carve& c) {
    d->set = c.take<unsigned long long>(d->slots), d->list = c.take<unsigned long long>(n), d->count = c.take<unsigned>(1);
  }, occ_pad));
  return SBM_OK;
}
// A discretised scan's first steps, inside the mark stage's time: the set and the count are cleared in stream order, then `dedupe`
// launches its kernel
template <class Dedupe> static void occ_dedupe_run(sbm_handle* h, const OccDedupe& d, Dedupe dedupe) {
  if (hipMemsetAsync(d.set, 0xFF, (size_t)d.slots * 8, h->stream) != hipSuccess) return;   // occ_rays_scan looks at the last error
  if (hipMemsetAsync(d.count, 0, sizeof(unsigned), h->stream) != hipSuccess) return;
  dedupe();
}

// One scan: `mark` launches its mark kernel; the apply launch follows in stream order. On a growing map the host reads the
// counters in between: MARK only claims keys and ORs bits, and a slot enters the touched list only when its flag word was clear,
// so the same MARK runs again on a larger table, which brought the flags along, until no cell is lost.
template <class Mark> static int occ_rays_scan(sbm_occ_map* map, OccRay& g, OccTable& t, Mark mark) {
  sbm_handle* h = map->h;
  StageClock& clk = h->occ.clock;
  g.parity = map->scan & 1;
  unsigned long long before = 0;
  if (map->grow) {
    const int st = occ_overflow_before(map, &before);
    if (st != SBM_OK) return st;
  }
  HIPCHK(h, clk.mark(kOccBegin, h->stream));
  mark();
  HIPCHK(h, hipGetLastError());
  for (bool again = map->grow; again;) {
    OccCounters c;
    const int st = occ_grow_settle(map, before, &c, &again);
    if (st != SBM_OK) return st;
    occ_rays_table(map, &g, &t);
    if (again) {
      mark();
      HIPCHK(h, hipGetLastError());
    }
  }
  HIPCHK(h, clk.mark(kOccMid, h->stream));
  occ_with_options(map, [&](auto, auto track) {
    const dim3 grid(std::min((map->slots + 255) / 256, 1024u));
    if (map->stamp.p)   // the clock as it is at this call
      hipLaunchKernelGGL((occ_rays_apply_stamped_kernel<decltype(track)::value>), grid, dim3(256), 0, h->stream, g, t, map->stamp.as<unsigned>(), map->clock);
    else
      hipLaunchKernelGGL((occ_rays_apply_kernel<decltype(track)::value>), grid, dim3(256), 0, h->stream, g, t);
  });
  HIPCHK(h, hipGetLastError());
  map->scan++;
  HIPCHK(h, clk.mark(kOccEnd, h->stream));
  HIPCHK(h, clk.add(kOccRaysMark, kOccBegin, kOccMid));
  HIPCHK(h, clk.add(kOccRaysApply, kOccMid, kOccEnd));
  return SBM_OK;
}

static int occ_check_cloud(const sbm_occ_map* map, size_t n, const void* xyz, const float* origin, const sbm_occ_ray_params* p) {
  if (!map || !origin || !p || (n > 0 && !xyz)) return SBM_ERR_NULL;
  const int st = occ_ray_params_check(p);
  if (st != SBM_OK) return st;
  if (n > ((size_t)1 << 30)) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

static int occ_cloud_run(sbm_occ_map* map, size_t n, const float* d_xyz, const float* origin, const sbm_occ_ray_params* p, int sync,
                         bool discrete = false) {
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
    const dim3 grid((unsigned)((n + 255) / 256));
    OccDedupe d;
    if (discrete && (st = occ_dedupe_begin(map, n, &d)) != SBM_OK) return st;
    st = occ_rays_scan(map, g, t, [&] {
      if (discrete) occ_dedupe_run(h, d, [&] { hipLaunchKernelGGL(occ_dedupe_cloud_kernel, grid, dim3(256), 0, h->stream, d_xyz, n, g.factor, d); });
      occ_with_mark_options(map, [&](auto box, auto track) {
        constexpr bool kBox = decltype(box)::value, kTrack = decltype(track)::value;
        if (discrete) hipLaunchKernelGGL((occ_rays_mark_list_kernel<kBox, kTrack>), grid, dim3(256), 0, h->stream, d, o, g, t);
        else hipLaunchKernelGGL((occ_rays_mark_cloud_kernel<kBox, kTrack>), grid, dim3(256), 0, h->stream, d_xyz, n, o, g, t);
      });
    });
    if (st != SBM_OK) return st;
  }
  return occ_overflow_status(map, sync);
}

static int occ_planes_run(sbm_occ_map* map, int n, const int16_t* d_disp, int W, int H, int scale, const sbm_stereo_model* model,
                          const float* poses, const sbm_occ_ray_params* p, int sync, bool discrete = false) {
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
    const dim3 grid((unsigned)((plane + 255) / 256));
    OccDedupe d;
    if (discrete && (st = occ_dedupe_begin(map, plane, &d)) != SBM_OK) return st;
    st = occ_rays_scan(map, g, t, [&] {
      if (discrete)
        occ_dedupe_run(h, d, [&] {
          hipLaunchKernelGGL(occ_dedupe_plane_kernel, grid, dim3(256), 0, h->stream, d_disp + plane * i, pg, *model, pose, g.factor, d);
        });
      occ_with_mark_options(map, [&](auto box, auto track) {
        constexpr bool kBox = decltype(box)::value, kTrack = decltype(track)::value;
        if (discrete) hipLaunchKernelGGL((occ_rays_mark_list_kernel<kBox, kTrack>), grid, dim3(256), 0, h->stream, d, pose, g, t);
        else hipLaunchKernelGGL((occ_rays_mark_plane_kernel<kBox, kTrack>), grid, dim3(256), 0, h->stream, d_disp + plane * i, pg, *model, pose, g, t);
      });
    });
    if (st != SBM_OK) return st;
  }
  return occ_overflow_status(map, sync);
}

}  // namespace sbm
using namespace sbm;

extern "C" {
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

static int occ_insert_cloud_device(sbm_occ_map* map, size_t n_points, const void* d_xyz, const float* origin,
                                   const sbm_occ_ray_params* params, int sync, bool discrete) {
  const int st = occ_check_cloud(map, n_points, d_xyz, origin, params);
  if (st != SBM_OK) return st;
  if ((uintptr_t)d_xyz & 3) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_cloud_run(map, n_points, (const float*)d_xyz, origin, params, sync, discrete);
}

static int occ_insert_cloud_host(sbm_occ_map* map, size_t n_points, const float* xyz, const float* origin, const sbm_occ_ray_params* params,
                                 bool discrete) {
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
  return occ_cloud_run(map, n_points, h->occ.io.as<float>(), origin, params, 1, discrete);
}

static int occ_insert_rays_device(sbm_occ_map* map, int n, const void* d_disp, int width, int height, int scale,
                                  const sbm_stereo_model* model, const float* poses, const sbm_occ_ray_params* params, int sync, bool discrete) {
  int st = occ_check_insert(map, n, d_disp, width, height, scale, model, poses);
  if (st == SBM_OK) st = occ_ray_params_check(params);
  if (st != SBM_OK) return st;
  if ((uintptr_t)d_disp & 1) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_planes_run(map, n, (const int16_t*)d_disp, width, height, scale, model, poses, params, sync, discrete);
}

static int occ_insert_rays_host(sbm_occ_map* map, int n, const int16_t* disp, int width, int height, int scale, const sbm_stereo_model* model,
                                const float* poses, const sbm_occ_ray_params* params, bool discrete) {
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
  return occ_planes_run(map, n, h->occ.io.as<int16_t>(), width, height, scale, model, poses, params, 1, discrete);
}

int sbm_occ_insert_cloud_device(sbm_occ_map* map, size_t n_points, const void* d_xyz, const float* origin,
                                const sbm_occ_ray_params* params, int sync) {
  return occ_insert_cloud_device(map, n_points, d_xyz, origin, params, sync, false);
}
int sbm_occ_insert_cloud(sbm_occ_map* map, size_t n_points, const float* xyz, const float* origin, const sbm_occ_ray_params* params) {
  return occ_insert_cloud_host(map, n_points, xyz, origin, params, false);
}
int sbm_occ_insert_rays_device(sbm_occ_map* map, int n, const void* d_disp, int width, int height, int scale,
                               const sbm_stereo_model* model, const float* poses, const sbm_occ_ray_params* params, int sync) {
  return occ_insert_rays_device(map, n, d_disp, width, height, scale, model, poses, params, sync, false);
}
int sbm_occ_insert_rays(sbm_occ_map* map, int n, const int16_t* disp, int width, int height, int scale, const sbm_stereo_model* model,
                        const float* poses, const sbm_occ_ray_params* params) {
  return occ_insert_rays_host(map, n, disp, width, height, scale, model, poses, params, false);
}
int sbm_occ_insert_cloud_discrete_device(sbm_occ_map* map, size_t n_points, const void* d_xyz, const float* origin,
                                         const sbm_occ_ray_params* params, int sync) {
  return occ_insert_cloud_device(map, n_points, d_xyz, origin, params, sync, true);
}
int sbm_occ_insert_cloud_discrete(sbm_occ_map* map, size_t n_points, const float* xyz, const float* origin,
                                  const sbm_occ_ray_params* params) {
  return occ_insert_cloud_host(map, n_points, xyz, origin, params, true);
}
int sbm_occ_insert_rays_discrete_device(sbm_occ_map* map, int n, const void* d_disp, int width, int height, int scale,
                                        const sbm_stereo_model* model, const float* poses, const sbm_occ_ray_params* params, int sync) {
  return occ_insert_rays_device(map, n, d_disp, width, height, scale, model, poses, params, sync, true);
}
int sbm_occ_insert_rays_discrete(sbm_occ_map* map, int n, const int16_t* disp, int width, int height, int scale,
                                 const sbm_stereo_model* model, const float* poses, const sbm_occ_ray_params* params) {
  return occ_insert_rays_host(map, n, disp, width, height, scale, model, poses, params, true);
}
}  // extern "C"
