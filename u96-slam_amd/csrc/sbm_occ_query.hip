// sbm_occ_query.hip -- the occupancy map's read side, octomap's search and castRay (OcTreeBaseImpl.hxx:408-470,
// OccupancyOcTreeBase.hxx:645-765), for points, rays and a virtual camera's pixels.  gfx950. Nothing here contracts a multiply-add.
//
//   occ_search_kernel / occ_cast_rays_kernel / occ_cast_view_kernel   one lane per point, ray or pixel probes the table and walks
//                       castRay's DDA in registers. Read-only and stream-ordered after the inserts: plain cached loads, no
//                       atomics; a lane that has its answer leaves its loop, nothing needs the whole wavefront.
#include "sbm_occ.h"

namespace sbm {
#pragma clang fp contract(off)

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

// castRay, in the order of the source -> status, *end
__device__ __forceinline__ int occ_query_ray(Pt3 o, Pt3 d, const OccQuery& g, Pt3* end) {
#pragma clang fp contract(off)
  *end = nan3();
  unsigned c0, c1, c2, word;
  if (!(occ_axis(g.factor, o.x, &c0) && occ_axis(g.factor, o.y, &c1) && occ_axis(g.factor, o.z, &c2))) return SBM_OCC_RAY_NONE;
  int cell = occ_lookup(occ_pack(c0, c1, c2), g, &word);
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
  occ_dda_axis<false>(d.x, c0, o.x, g.resolution, &s0, &t0, &d0);   // castRay, OccupancyOcTreeBase.hxx:677-696: the half cell
  occ_dda_axis<false>(d.y, c1, o.y, g.resolution, &s1, &t1, &d1);   // is added in double
  occ_dda_axis<false>(d.z, c2, o.z, g.resolution, &s2, &t2, &d2);
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
    cell = occ_lookup(occ_pack(c0, c1, c2), g, &word);
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
    st = occ_lookup(occ_pack(k0, k1, k2), g, &word);
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
  occ_probe(map, &g->mask, &g->max_probe);
  g->keys = map->keys.as<unsigned long long>();
  g->vals = map->hits.as<unsigned>();
}

static int occ_search_run(sbm_occ_map* map, size_t n, const float* d_xyz, float thres, int* d_state, unsigned* d_value, int sync) {
  OccQuery g;
  occ_query_begin(map, -1., thres, 0, &g);
  return occ_timed_run(map->h, kOccSearch, n > 0, sync, [&]() -> int {
    hipLaunchKernelGGL(occ_search_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, map->h->stream, d_xyz, n, g, d_state, d_value);
    return SBM_OK;
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
  return occ_timed_run(map->h, kOccCast, n > 0, sync, [&]() -> int {
    hipLaunchKernelGGL(occ_cast_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, map->h->stream, d_origins, d_dirs, n, v, g,
                       d_status, d_end);
    return SBM_OK;
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

}  // namespace sbm
using namespace sbm;

extern "C" {
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
  DeviceScope dscope(map->h->device);
  HIPCHK(map->h, dscope.enter());
  return occ_search_host(map->h, n, xyz, false, state, value, nullptr, [&](const float* d_xyz, int* d_state, unsigned* d_value, int*) {
    return occ_search_run(map, n, d_xyz, occupancy_thres_log, d_state, d_value, 0);
  });
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
  struct { float *dirs, *origins; int* status; float* end; } io = {};
  if (n) {
    HIPCHK(h, carve(h->occ.io, h->stream, [&](Carve& c) {
      io = {c.take<float>(n * 3), c.take<float>(n * 3), c.take<int>(n), c.take<float>(n * 3)};
    }, occ_pad));
    HIPCHK(h, hipMemcpyAsync(io.dirs, dirs, n * 12, hipMemcpyHostToDevice, h->stream));
    if (!shared_origin) HIPCHK(h, hipMemcpyAsync(io.origins, origins, n * 12, hipMemcpyHostToDevice, h->stream));
  }
  st = occ_cast_run(map, n, shared_origin ? nullptr : io.origins, shared_origin ? origins : nullptr, io.dirs, params, io.status, io.end, 0);
  if (st != SBM_OK) return st;
  if (n) {
    HIPCHK(h, hipMemcpyAsync(status, io.status, n * 4, hipMemcpyDeviceToHost, h->stream));
    if (end) HIPCHK(h, hipMemcpyAsync(end, io.end, n * 12, hipMemcpyDeviceToHost, h->stream));
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
  return occ_timed_run(h, kOccCast, true, sync, [&]() -> int {
    hipLaunchKernelGGL(occ_cast_view_kernel, dim3(blocks), dim3(256), 0, h->stream, v, *model, t, g, (int*)d_status, (float*)d_end);
    return SBM_OK;
  });
}
}  // extern "C"
