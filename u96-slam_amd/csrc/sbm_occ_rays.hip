// sbm_occ_rays.hip -- the occupancy map's log-odds mode, octomap's insertPointCloud per scan (OccupancyOcTreeBase.hxx:86-102,
// computeUpdate :169-270), for a cloud or for the planes of the hit insert.  gfx950. Nothing here contracts a multiply-add.
//
//   occ_rays_mark_*_kernel   one lane per ray walks computeRayKeys' 3-D DDA in registers and ORs "free" / "occupied this scan" into the
//                       flag word of every cell's slot; the lane whose OR found the word clear appends the slot to the touched list.
//   occ_rays_apply_kernel   gives every touched slot its ONE update (occupied wins) and clears the flags.
#include "sbm_occ.h"

namespace sbm {
#pragma clang fp contract(off)

struct OccRay {                 // one call's constants
  double max_range;             // < 0: no limit
  double resolution, factor;    // factor = 1. / resolution
  float hit, miss, cmin, cmax;  // log-odds
  uint32_t mask, max_probe, slots;
  uint32_t parity;              // which of OccCounters::touched counts this scan
};
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
    bool claimed = false;
    const bool found = occ_find_or_claim(t.keys, key, g.mask, g.max_probe, &slot, &claimed);
    if (claimed) atomicAdd(&t.ctr->size, 1u);
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
  const uint32_t at = occ_wave_append(fresh, &t.ctr->touched[g.parity]);
  if (fresh && at < g.slots) t.touched[at] = slot;   // a slot is appended once per scan: the list of `slots` entries always has room
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
      occ_dda_axis<true>(dx, c0, ox, g.resolution, &s0, &t0, &d0);   // computeRayKeys, OcTreeBaseImpl.hxx:577-596: the half
      occ_dda_axis<true>(dy, c1, oy, g.resolution, &s1, &t1, &d1);   // cell is rounded to float
      occ_dda_axis<true>(dz, c2, oz, g.resolution, &s2, &t2, &d2);
    }
  }
  // The origin cell first, then one cell per step until the end cell's key or the ray's length is reached; the end cell is not
  // part of the ray. The step count is bounded whatever the input: the wavefront leaves the loop when its last lane has.
  int steps = 0;
  while (__ballot(walking)) {
    occ_mark_cell(occ_pack(c0, c1, c2), kOccFree, walking, g, t);
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
  occ_mark_cell(occ_pack(e0, e1, e2), kOccOccupied, ends, g, t);
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
  occ_probe(map, &g->mask, &g->max_probe);
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
  return occ_overflow_status(map, sync);
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
}  // extern "C"
